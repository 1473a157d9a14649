"""GPU (-m gpu): replayable levels — MultiGridEnv.set_levels / LevelBank (mg_level_seed, mg_level_apply) against the level oracle
(tests/level_ref.py: an env that resets onto level s becomes `OracleEnv(spec, seed=s, construct=False)` and is reset), on every
step path.  Batch sizes are wave geometry: 67, 130 and 131 envs are full and partial waves, rows 0 and 129 lie in different
waves; max_steps is small so that every env resets many times in a few dozen steps."""
import numpy as np
import pytest

import canon
import level_ref
import product_envs
import scenarios
from oracle import oracle as O

pytestmark = pytest.mark.gpu
REW_TOL = 1e-6          # per step: tests/test_core_hostemu.py
P_ACT = [.15, .15, .5, .05, .05, .05, .05]
BENCH = "MarlGrid-3AgentCluttered15x15-v0"
INFO_KEYS = {"terminated", "truncated", "episode_return", "episode_length", "reset", "level"}


def _spec(max_steps):
    return dict(scenarios.registered(BENCH), max_steps=max_steps)


def _np(x):
    """a tensor, or a list of per-shard tensors in global order -> numpy"""
    if isinstance(x, (list, tuple)):
        return np.concatenate([p.cpu().numpy() for p in x])
    return x.cpu().numpy()


def _same_obs(obs, want, what):
    got = _np(obs)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere((got != want).reshape(len(got), -1).any(axis=1))
    assert bad.size == 0, (what, "envs", bad[:8].ravel().tolist())
    return got


def _check_step(out, want_out, what, info_keys=INFO_KEYS):
    obs, r, d, info = out
    want_obs, r2, d2, want = want_out
    got = _same_obs(obs, want_obs, what)
    assert np.abs(_np(r).astype(np.float64) - r2).max() <= REW_TOL, what
    assert np.array_equal(_np(d), d2), what
    if info_keys:
        assert set(info.keys()) == info_keys, what
        ginfo = {k: _np(v) for k, v in info.items()}
        assert ginfo["level"].dtype == np.int64
        level_ref.assert_info(ginfo, want, what)
        tol = REW_TOL * np.maximum(want["episode_length"], 1)[:, None]
        assert (np.abs(ginfo["episode_return"] - want["episode_return"]) <= tol).all(), what
    return got


def _same_rng(env, ref, what, rows=None):
    for b in (range(ref.B) if rows is None else rows):
        assert seeding_same(env.numpy_rng_state(b), ref.envs[b].mt_state()), "%s: RNG of env %d" % (what, b)


def seeding_same(a, b):
    from marlgrid_amd import seeding
    return seeding.same_stream(a, b)


def _same_state(env, ref, what):
    st = product_envs.canonical(env)
    for b in range(ref.B):
        canon.assert_same(st[b], canon.oracle_canonical(ref.envs[b]), "%s env %d" % (what, b))


class Relevel(object):
    """what a finished env is given next — fresh seeds, repeats of earlier ones, and once per env at the most none —, the same
    draws for whoever asks"""

    def __init__(self, B, first, seed=5):
        self.B, self.rng, self.fresh = B, np.random.RandomState(seed), 50000
        self.pool = [7, 2 ** 32 + 5, 2 ** 63 - 1, 0]
        self.had_free = np.asarray(first) < 0

    def seeds(self, done):
        nxt = np.full(self.B, -1, np.int64)
        for b in np.nonzero(done)[0]:
            kind = self.rng.randint(0, 10)
            if kind < 5:
                nxt[b] = self.fresh
                self.fresh += 1
            elif kind < 9 or self.had_free[b]:
                nxt[b] = self.pool[self.rng.randint(len(self.pool))]
            self.had_free[b] |= nxt[b] < 0
            if nxt[b] >= 0 and len(self.pool) < 64:
                self.pool.append(int(nxt[b]))
        return nxt

    def slots(self, done, L):
        ids = np.full(self.B, -1, np.int64)
        for b in np.nonzero(done)[0]:
            ids[b] = self.rng.randint(0, L) if self.had_free[b] or self.rng.randint(0, 10) else -1
            self.had_free[b] |= ids[b] < 0
        return ids


# ---- 6. a reset by hand -------------------------------------------------------------------------------------------------------
def test_manual_reset_plays_the_named_levels():
    import torch
    B = 67
    seeds = [0, 1, 2 ** 32, 2 ** 63 - 1] + list(range(1000, 1063))
    assert len(seeds) == B
    env = product_envs.build(BENCH, batch_size=B, seeds=4200 + np.arange(B), place_obs=False, auto_reset=False)
    ref = level_ref.LevelOracle(scenarios.registered(BENCH), 4200 + np.arange(B), mode=None, render="image")
    assert env._level_launches == 0
    env.set_levels(seeds=seeds)
    ref.set_levels(seeds)
    assert (env.episode_level == -1).all()           # nothing happens before the reset
    _same_obs(env.reset(), ref.reset(), "reset")
    assert env.episode_level.tolist() == seeds and env._level_launches == 1
    _same_state(env, ref, "reset")
    _same_rng(env, ref, "reset")
    # (an engine that ignored the seeds could not pass by accident: the oracle's layouts of these seeds all differ, as do
    # those of 1000 .. 1063; and they are the layouts of freshly made envs, not of the batch's own streams)
    def layout(e):
        c = canon.oracle_canonical(e)
        return c["base_enc"].tobytes() + c["pos"].tobytes()
    assert len({layout(e) for e in ref.envs}) == B
    more = [O.OracleEnv(scenarios.registered(BENCH), seed=s, construct=False, _like=ref._proto[0]) for s in range(1000, 1064)]
    for e in more:
        e.reset()
    assert len({layout(e) for e in more}) == 64
    assert [layout(e) for e in more[:63]] == [layout(e) for e in ref.envs[4:]]
    rng = np.random.RandomState(6)
    for t in range(9):
        a = rng.choice(7, size=(B, 3), p=P_ACT)
        _check_step(env.step(torch.from_numpy(a)), ref.step(a), "step %d" % t, info_keys=None)
    # new seeds for some: the others keep running their stream
    mask = np.zeros(B, bool)
    mask[[0, 3, 63, 64, 66]] = True
    new = np.where(mask, 3000 + np.arange(B), -5)            # (the values of unselected rows are not looked at ... by the oracle)
    env.set_levels(seeds=torch.from_numpy(np.where(mask, new, 0)).to(env.device), env_mask=torch.from_numpy(mask).to(env.device))
    ref.set_levels(new, mask)
    _same_obs(env.reset(env_mask=torch.from_numpy(mask)), ref.reset_envs(mask), "masked reset")
    assert env.episode_level.tolist() == np.where(mask, new, seeds).tolist()
    _same_state(env, ref, "masked reset")
    for t in range(3):
        a = rng.choice(7, size=(B, 3), p=P_ACT)
        _check_step(env.step(torch.from_numpy(a)), ref.step(a), "step %d after the masked reset" % t, info_keys=None)
    _same_rng(env, ref, "end")
    env.check_errors()


# ---- 7. next-step reset: the seeds form and the bank form ----------------------------------------------------------------------
@pytest.mark.parametrize("form", ["seeds", "bank"])
def test_next_step_levels_vs_oracle(form):
    import torch
    B, T, L = 131, 60, 5
    base = 4200 + np.arange(B)
    env = product_envs.build(BENCH, batch_size=B, seeds=base, place_obs=False, auto_reset="next_step", episode_info=True, max_steps=9)
    ref = level_ref.LevelOracle(_spec(9), base, render="image")
    dev = env.device
    first = 100 + np.arange(B)
    first[::7] = -1
    pick = Relevel(B, first)
    if form == "seeds":
        env.set_levels(seeds=torch.from_numpy(first).to(dev))
        ref.set_levels(first)
    else:
        bank_seeds = np.array([11, 12, 13, 2 ** 63 - 1, 15], np.int64)
        bank = env.level_bank(torch.from_numpy(bank_seeds).to(dev))
        assert len(bank) == L and bank.seeds.tolist() == bank_seeds.tolist()
        ids = np.where(first < 0, -1, np.arange(B) % L)
        env.set_levels(bank, torch.from_numpy(ids).to(dev))
        resolve = lambda: np.where(ids >= 0, bank_seeds[np.maximum(ids, 0)], -1)
        ref.set_levels(resolve())
    _same_obs(env.reset(), ref.reset(), "reset")
    assert np.array_equal(_np(env.episode_level), ref.episode_level)
    for t in range(T):
        a = rng_actions(t, B)
        out = env.step(torch.from_numpy(a))
        what = "%s form, step %d" % (form, t)
        _check_step(out, ref.step(a), what)
        assert np.array_equal(_np(env.episode_level), ref.episode_level), what
        done_t = out[2]
        d = _np(done_t)
        if d.any() and form == "seeds":
            nxt = pick.seeds(d)
            env.set_levels(seeds=torch.from_numpy(nxt).to(dev), env_mask=done_t)
            ref.set_levels(nxt, d)
        elif d.any():
            new = pick.slots(d, L)
            ids = np.where(d, new, ids)
            env.set_levels(bank, torch.from_numpy(new).to(dev), env_mask=done_t)
            ref.set_levels(resolve())
        if form == "bank" and t == 25:      # new levels in two slots: whoever points there plays them from its next reset on
            bank.assign(torch.tensor([2, 0], device=dev), torch.tensor([777, 2 ** 40 + 1], device=dev))
            bank_seeds[[2, 0]] = [777, 2 ** 40 + 1]
            ref.set_levels(resolve())
    _same_rng(env, ref, form)
    env.check_errors()
    assert ref.levelled.min() >= 5, ref.levelled
    if form == "bank":
        assert bank.seeds.tolist() == bank_seeds.tolist()
        assert max(np.bincount(ids[ids >= 0])) >= 10          # many envs share a level


def rng_actions(t, B, n=3):
    return np.random.RandomState(1000 + t).choice(7, size=(B, n), p=P_ACT)


# ---- 8. replay -----------------------------------------------------------------------------------------------------------------
def test_a_level_replays_in_another_row_and_two_rows_share_one():
    """B = 130, max_steps = 9: every env runs into the time limit at steps 9, 19, 29, 39 and resets at steps 10, 20, 30, 40.  Row 0
    plays level S from the reset on; row 129 is pointed at S before step 30 and given row 0's action rows 30 steps late.  Rows 5
    and 70 point at one bank slot all along and get the same actions."""
    import torch
    B, S = 130, 424242
    env = product_envs.build(BENCH, batch_size=B, seeds=4200 + np.arange(B), place_obs=False, auto_reset="next_step", episode_info=True,
                             max_steps=9)
    bank = env.level_bank([S, 99])
    ids = np.full(B, -1)
    ids[[0, 5, 70]] = [0, 1, 1]
    env.set_levels(bank, ids)
    obs = [env.reset().cpu().numpy()]
    rew, acts, lvl = [None], [None], [None]
    for t in range(1, 41):
        a = rng_actions(t, B)
        a[70] = a[5]
        if t > 30:
            a[129] = acts[t - 30][0]
        if t == 25:
            env.set_levels(bank, 0, env_ids=[129])
        o, r, d, info = env.step(torch.from_numpy(a))
        assert bool(d.all()) == (t % 10 == 9) and bool(d.any()) == (t % 10 == 9)
        obs.append(o.cpu().numpy()), rew.append(r.cpu().numpy()), acts.append(a), lvl.append(info["level"].cpu().numpy())
    assert (obs[0][0] != obs[0][129]).any() and (obs[10][129] != obs[10][0]).any()
    for t in range(0, 11):
        assert np.array_equal(obs[30 + t][129], obs[t][0]), t         # t = 0: the reset's observation; t = 10: the level again
        if t:
            assert np.array_equal(rew[30 + t][129], rew[t][0]), t
            assert lvl[30 + t][129] == S == lvl[t][0] and lvl[t][129] == -1
    assert np.array_equal(obs[10][0], obs[0][0]) and any((obs[t][0] != obs[0][0]).any() for t in range(1, 10))
    for t in range(41):
        assert np.array_equal(obs[t][5], obs[t][70]), t
        if t:
            assert np.array_equal(rew[t][5], rew[t][70]) and lvl[t][5] == lvl[t][70] == 99
    assert any((obs[t][5] != obs[t - 1][5]).any() for t in range(1, 10))
    env.check_errors()


# ---- 9. every step path --------------------------------------------------------------------------------------------------------
class _Shards(object):
    """a ShardPipeline / DeviceShards behind the surface the runner below uses"""

    def __init__(self, sh):
        self.sh = sh
        self.device = sh.envs[0].device

    def set_levels(self, **kw):
        self.sh.set_levels(**kw)

    def reset(self):
        out = self.sh.reset()
        self.sh.synchronize()       # (what a shard returns is ordered on its own stream)
        return out

    def step(self, a):
        out = self.sh.step(a.to(self.device))
        self.sh.synchronize()
        info = {k: [o[3][k] for o in out] for k in out[0][3]}
        return [o[0] for o in out], [o[1] for o in out], [o[2] for o in out], info

    @property
    def episode_level(self):
        return self.sh.episode_level

    def numpy_rng_state(self, g):
        for (lo, hi), e in zip(self.sh.ranges, self.sh.envs):
            if lo <= g < hi:
                return e.numpy_rng_state(g - lo)

    def check_errors(self):
        self.sh.check_errors()

    @property
    def launches(self):
        return [e._level_launches for e in self.sh.envs]


def _run_path(env, ref, B, T, bank=None, L=4):
    import torch
    first = 100 + np.arange(B)
    first[::7] = -1
    pick = Relevel(B, first, seed=8)
    dev = env.device
    if bank is None:
        env.set_levels(seeds=torch.from_numpy(first).to(dev))
        ref.set_levels(first)
    else:
        bank_seeds = bank.seeds.cpu().numpy().copy()
        ids = np.where(first < 0, -1, np.arange(B) % L)
        env.set_levels(bank=bank, ids=torch.from_numpy(ids).to(dev))
        resolve = lambda: np.where(ids >= 0, bank_seeds[np.maximum(ids, 0)], -1)
        ref.set_levels(resolve())
    _same_obs(env.reset(), ref.reset(), "reset")
    for t in range(T):
        a = rng_actions(t, B)
        out = env.step(torch.from_numpy(a))
        what = "step %d" % t
        _check_step(out, ref.step(a), what)
        assert np.array_equal(_np(env.episode_level), ref.episode_level), what
        d = _np(out[2])
        done_t = torch.from_numpy(d).to(dev)
        if d.any() and bank is None:
            nxt = pick.seeds(d)
            env.set_levels(seeds=torch.from_numpy(nxt).to(dev), env_mask=done_t)
            ref.set_levels(nxt, d)
        elif d.any():
            new = pick.slots(d, L)
            ids = np.where(d, new, ids)
            env.set_levels(bank=bank, ids=torch.from_numpy(new).to(dev), env_mask=done_t)
            if t < 10:       # ... and a new level in a slot, on every replica
                bank.assign(torch.tensor([1], device=bank.device), torch.tensor([31337], device=bank.device))
                bank_seeds[1] = 31337
            ref.set_levels(resolve())
    for b in (0, 1, B // 2 - 1, B // 2, B - 1):
        assert seeding_same(env.numpy_rng_state(b), ref.envs[b].mt_state()), "RNG of env %d" % b
    env.check_errors()
    assert ref.levelled.min() >= 3, ref.levelled


PATHS = ["fused", "unfused", "encoded", "delta_ex", "specialize", "pipeline", "devices"]


@pytest.mark.parametrize("path", PATHS)
def test_every_step_path_vs_oracle(path, tmp_path):
    import torch
    from marlgrid_amd import envs as E
    B, T, M = 70, 25, 7
    base = 4200 + np.arange(B)
    kw = dict(batch_size=B, place_obs=False, auto_reset="next_step", episode_info=True, max_steps=M)
    spec, fmt, bank = _spec(M), "image", None
    if path == "fused":
        env = product_envs.build(BENCH, seeds=base, **kw)
    elif path == "unfused":
        env = product_envs.build(BENCH, seeds=base, fused_step=False, **kw)
    elif path == "encoded":
        env, fmt = product_envs.build(BENCH, seeds=base, obs_format="encoded", **kw), "encoded"
    elif path == "delta_ex":
        env = product_envs.build(BENCH, seeds=base, obs_delta=True, **kw)
    elif path == "specialize":
        # (an off-table shape, as tests/test_hip_specialize.py builds it: view 10 at 6-pixel tiles)
        from marlgrid_amd.agents import GridAgentInterface
        team = [GridAgentInterface(color=c, view_size=10, view_tile_size=6) for c in scenarios.REG_COLORS[:3]]
        env = E.ClutteredMultiGrid(agents=team, grid_size=15, n_clutter=12, seeds=base, specialize="auto", specialize_cache=str(tmp_path), **kw)
        assert env.kernel_name.startswith("mg::render_kernel<10, 6, ")
        spec = scenarios.cluttered_spec(3, 15, 10, n_clutter=12, tile_size=6, max_steps=M)
    elif path == "pipeline":
        env = _Shards(E.make(BENCH, pipeline=2, seed=4200, **kw))
    else:
        sh = E.make(BENCH, devices=["cuda:0", "cuda:0"], seed=4200, **kw)
        env = _Shards(sh)
        bank = sh.envs[0].level_bank([21, 22, 23, 2 ** 62])
    ref = level_ref.LevelOracle(spec, base, render=fmt)
    _run_path(env, ref, B, T, bank=bank)
    if path == "delta_ex":
        assert env._delta_launches == T
    if path == "devices":
        assert list(bank._replicas) == [torch.device("cuda", 0)]          # one replica per distinct device
        rep = bank._replicas[torch.device("cuda", 0)]
        assert rep.seeds.tolist() == bank.seeds.tolist() == [21, 31337, 23, 2 ** 62]
        assert all(e._level_bank is rep for e in sh.envs)
    launches = env.launches if isinstance(env, _Shards) else [env._level_launches]
    assert all(n == T + 1 for n in launches), launches       # one small launch per reset() and per step()


# ---- 11. nothing new without levels ----------------------------------------------------------------------------------------------
def test_an_env_without_levels_launches_nothing_new():
    import torch
    B = 67
    env = product_envs.build(BENCH, batch_size=B, seeds=4200 + np.arange(B), place_obs=False, auto_reset="next_step", episode_info=True,
                             max_steps=9)
    env.reset()
    for t in range(20):
        _, _, _, info = env.step(torch.from_numpy(rng_actions(t, B)))
        assert "level" not in info
    assert env._level_launches == 0 and not env._levels_on and env._level_bank is None and env._own_bank is None
    assert (env.episode_level == -1).all()
    assert "episode_level_t" not in env.state_dict() and "level_next_t" not in env.state_dict()
    with pytest.raises(ValueError, match="next_step"):
        product_envs.build(BENCH, batch_size=4, place_obs=False, auto_reset=True).set_levels(seeds=1)


# ---- 12. checkpoints ---------------------------------------------------------------------------------------------------------------
def test_state_dict_carries_running_and_pending_levels():
    import torch
    from marlgrid_amd import envs as E
    B, M = 70, 7
    base = 4200 + np.arange(B)
    kw = dict(batch_size=B, place_obs=False, auto_reset="next_step", episode_info=True, max_steps=M)
    env = product_envs.build(BENCH, seeds=base, **kw)
    bank = env.level_bank([61, 62, 63])
    env.set_levels(bank, np.arange(B) % 4 - 1)
    env.reset()
    for t in range(10):                  # (mid-episode: three steps into the second one)
        env.step(torch.from_numpy(rng_actions(t, B)))
    pend = np.where(np.arange(B) % 3 == 0, -1, 900 + np.arange(B) % 5)
    env.set_levels(bank, 2, env_ids=[1, 2])                  # pending assignments: through the bank, and then ...
    sd = env.state_dict()
    assert sd["episode_level_t"].tolist() == [[-1, 61, 62, 63][b % 4] for b in range(B)]
    want_next = [[-1, 61, 62, 63][b % 4] if b not in (1, 2) else 63 for b in range(B)]
    assert sd["level_next_t"].tolist() == want_next
    env.set_levels(seeds=pend)                               # ... every env in the seeds form
    sd = env.state_dict()
    assert sd["level_next_t"].tolist() == pend.tolist()
    fresh = product_envs.build(BENCH, seeds=base + 500, **kw)
    pipe = E.make(BENCH, pipeline=2, seed=77, **kw)
    fresh.load_state_dict(sd)
    pipe.load_state_dict({k: v.cpu() for k, v in sd.items()})
    for t in range(10, 30):
        a = torch.from_numpy(rng_actions(t, B))
        o, r, d, info = env.step(a)
        o2, r2, d2, info2 = fresh.step(a)
        out = pipe.step(a.to(env.device))
        pipe.synchronize()              # (what a part returns is ordered on its own stream)
        what = "step %d" % t
        for x, y, k in ((o, o2, 0), (r, r2, 1), (d, d2, 2)):
            assert torch.equal(x, y), what
            assert torch.equal(x, torch.cat([p[k] for p in out])), what
        for key in INFO_KEYS:
            assert torch.equal(info[key], info2[key]), (what, key)
            assert torch.equal(info[key], torch.cat([p[3][key] for p in out])), (what, key)
        assert torch.equal(env.episode_level, fresh.episode_level) and torch.equal(env.episode_level, torch.cat(pipe.episode_level))
    assert set(env.episode_level.tolist()) == set(pend.tolist())         # every env has reset onto its pending level by now
    pipe.synchronize()
    merged = pipe.state_dict()
    sd_end = env.state_dict()
    assert set(merged) == set(sd_end)
    for key in ("episode_level_t", "level_next_t", "mt_state", "agent_state"):
        assert torch.equal(merged[key], sd_end[key].cpu()), key
    # a checkpoint without the keys loads as before
    plain = product_envs.build(BENCH, seeds=base, **kw)
    fresh.load_state_dict(plain.state_dict())
