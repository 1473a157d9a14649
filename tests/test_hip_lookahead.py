"""GPU (-m gpu): `env.lookahead` / `env.lookahead_errors` / `env.fork` — mg_fork_rows and mg_rollout — on the cases of
tests/lookahead_cases.py (the host twin runs the same bodies in tests/test_lookahead_host.py).  Per case:
  (a) the env is untouched: state_dict(), error_t, the host flag and the last observation tensor are byte-identical before and
      after, also when a plan holds an action outside 0..6 — whose MG_ERR_VALUE shows in lookahead_errors and nowhere else;
  (b) a second env loaded from that state_dict(), auto_reset=False, stepped T times per plan: rewards BIT-identical, done
      identical, both with the freeze mask applied;
  (c) the oracle, as in the host test: done, rewards within 1e-6, the state every shadow row was left in, its generator;
  (d) the first row of a one-plan lookahead equals the rewards of the real step issued afterwards."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "native"))

import lookahead_cases as LC  # noqa: E402
from marlgrid_amd import _native as N  # noqa: E402

pytestmark = pytest.mark.gpu


def _build(cs, seeds=None, **kw):
    import product_envs
    seeds = cs.seeds if seeds is None else seeds
    args = dict(batch_size=len(seeds), seeds=[int(s) for s in seeds], place_obs=False, auto_reset=False)
    return product_envs.build(cs.name, **dict(args, **dict(cs.kw, **kw)))


def _after_prefix(cs, **kw):
    import torch
    env = _build(cs, **kw)
    for a in cs.prefix(env.num_agents):
        env.step(torch.from_numpy(a))
    return env


def _snapshot(env):
    sd = env.state_dict()
    return dict(sd=sd, error=env.error_t.clone(), flag=bool(env._flag.raised()), obs=env.obs.clone(), rewards=env.rewards.clone())


def _untouched(env, snap):
    import torch
    sd = env.state_dict()
    assert sd.keys() == snap["sd"].keys()
    for k, v in sd.items():
        assert torch.equal(v, snap["sd"][k]), "state_dict()[%r] changed" % k
    assert torch.equal(env.error_t, snap["error"]) and bool(env._flag.raised()) == snap["flag"]
    assert torch.equal(env.obs, snap["obs"]) and torch.equal(env.rewards, snap["rewards"])


def _ended(env, sd):
    rec = sd["agent_state"].cpu().numpy().astype(np.uint64)
    all_done = (((rec >> np.uint64(8 * N.AG_FLAGS)) & np.uint64(N.AF_DONE)) != 0).all(axis=1)
    return (sd["step_count_t"].cpu().numpy() >= env.max_steps) | all_done


def _by_stepping(cs, sd, plans, ids, **kw):
    """(b): what T step() calls of an auto_reset=False env in the state `sd` return per plan, the freeze mask applied"""
    import torch
    env2 = _build(cs, **kw)
    K, T, m, n = plans.shape
    rew, done = np.zeros((K, T, m, n), np.float32), np.zeros((K, T, m), bool)
    full = np.full((env2.batch_size, n), 6, np.int64)
    for p in range(K):
        env2.load_state_dict(sd)
        frozen = _ended(env2, sd)[ids]
        for t in range(T):
            full[ids] = plans[p, t]
            _, r, d, _ = env2.step(torch.from_numpy(full))
            rew[p, t] = np.where(frozen[:, None], np.float32(0), r.cpu().numpy()[ids])
            done[p, t] = frozen | d.cpu().numpy()[ids]
            frozen = done[p, t].copy()
    return rew, done


def _shadow_state(env, R):
    sh, W, H = env._look.shadow, env.width, env.height
    return dict(grid=sh.grid_state[:R].cpu().numpy()[:, :W * H].reshape(R, W, H), rec=sh.agent_state[:R].cpu().numpy(),
                step_count=sh.step_count_t[:R].cpu().numpy(), mt=sh.mt_state[:R].cpu().numpy().view(np.uint32),
                mt_pos=sh.mt_pos[:R].cpu().numpy(), mt_head=sh.mt_head[:R].cpu().numpy().view(np.uint32))


@pytest.mark.parametrize("key", LC.ORACLE_CASES)
def test_plans_match_step_and_the_oracle(key):
    import torch
    cs = LC.case(key)
    env = _after_prefix(cs)
    assert env.strict and env._look.shadow is None and env._look.launches == 0 and env.lookahead_errors is None
    B, n, K, T = cs.B, env.num_agents, cs.K, cs.T
    plans = cs.plans(n)
    snap = _snapshot(env)
    # (a) with a plan that holds an unknown action: recorded in its row, the env as it was, nothing raised
    bad = plans.copy()
    bad[K - 1, 1, B // 2, n - 1] = 9
    env.lookahead(torch.from_numpy(bad).to(env.device))
    errs = env.lookahead_errors.cpu().numpy()
    want_err = np.zeros((K, B), np.int32)
    want_err[K - 1, B // 2] = N.ERR_VALUE
    assert env._look.launches == 2 and np.array_equal(errs, want_err)
    _untouched(env, snap)
    env.check_errors()
    # the plans themselves, as int32 this time
    out = env.lookahead(torch.from_numpy(plans.astype(np.int32)).to(env.device))
    rew_t, done_t = out
    assert env._look.launches == 4 and rew_t.dtype == torch.float32 and done_t.dtype == torch.bool
    assert tuple(rew_t.shape) == (K, T, B, n) and tuple(done_t.shape) == (K, T, B)
    assert env._look.shadow.rows == K * B and env._look.grid_state.shape == (K * B, env.cells_stride)
    assert (env._look.prestige_t is None) == (env.prestige_t is None)
    rew, done = rew_t.cpu().numpy(), done_t.cpu().numpy()
    assert not env.lookahead_errors.any()
    _untouched(env, snap)
    # (b)
    rew2, done2 = _by_stepping(cs, snap["sd"], plans, np.arange(B))
    assert np.array_equal(done, done2)
    assert np.array_equal(rew.view(np.uint32), rew2.view(np.uint32))
    # (c)
    want = LC.Want(cs)
    want.coverage(cs)
    LC.compare(want, rew, done, _shadow_state(env, K * B), env.scenario_spec(), key)
    if key == "doorkey":        # pickup and toggle wrote the SHADOW grid: some shadow row differs from its env's
        assert bool((env._look.grid_state.view(K, B, -1) != env.grid_state.unsqueeze(0)).any())
    # (d) one plan in the (T, m, n) form: the same numbers (results do not depend on K), and the real step's rewards
    one = torch.from_numpy(plans[0]).to(env.device)
    r1, d1 = env.lookahead(one)
    assert tuple(r1.shape) == (1, T, B, n) and torch.equal(r1[0], rew_t[0]) and torch.equal(d1[0], done_t[0])
    first = r1[0, 0].clone()
    _, r, d, _ = env.step(one[0])
    assert torch.equal(r, first) and torch.equal(d, d1[0, 0])
    env.check_errors()


def test_the_256_lane_rollout_at_its_smallest_batch():
    """K * m = 131 073 rows, the first count step_lanes answers with 256 lanes: against step() alone"""
    import torch
    cs = LC.case("wide_k3")
    B, T = 256 * 8 * 64 + 1, 2
    env = _build(cs, seeds=4242 + np.arange(B))
    n = env.num_agents
    gen = torch.Generator(env.device).manual_seed(11)
    for _ in range(3):
        env.step(torch.randint(0, 7, (B, n), device=env.device, generator=gen))
    plan = torch.randint(0, 7, (T, B, n), device=env.device, generator=gen)
    sd = {k: v.clone() for k, v in env.state_dict().items()}
    rew, done = env.lookahead(plan)
    for k, v in env.state_dict().items():
        assert torch.equal(v, sd[k]), k
    frozen = torch.zeros(B, dtype=torch.bool, device=env.device)
    for t in range(T):
        _, r, d, _ = env.step(plan[t])
        assert torch.equal(rew[0, t], torch.where(frozen[:, None], torch.zeros_like(r), r)), t
        assert torch.equal(done[0, t], frozen | d), t
        frozen = frozen | d
    env.check_errors()


def test_env_ids_on_the_host_and_on_the_device():
    import torch
    cs = LC.case("wide_k3")
    env = _after_prefix(cs)
    n, K, B = env.num_agents, cs.K, cs.B
    plans = torch.from_numpy(cs.plans(n)).to(env.device)
    rew_all, done_all = (v.clone() for v in env.lookahead(plans))
    snap = _snapshot(env)
    host = [66, 3, 17, 3, 0]
    rew, done = env.lookahead(plans[:, :, host], env_ids=host)
    assert tuple(rew.shape) == (K, cs.T, 5, n) and torch.equal(rew, rew_all[:, :, host]) and torch.equal(done, done_all[:, :, host])
    ids = torch.tensor([66, 3, 200, 3, -1, 0], device=env.device)
    ok = ((ids >= 0) & (ids < B)).cpu()
    src = torch.where(ok.to(env.device), ids, torch.zeros_like(ids))
    rew, done = env.lookahead(plans[:, :, src], env_ids=ids)
    assert torch.equal(rew[:, :, ok], rew_all[:, :, ids[ok]]) and torch.equal(done[:, :, ok], done_all[:, :, ids[ok]])
    assert bool(done[:, :, ~ok].all()) and not bool(rew[:, :, ~ok].any()) and not bool(env.lookahead_errors.any())
    every_other = torch.arange(B, device=env.device)[::2]           # a strided view of ids
    rew, done = env.lookahead(plans[:, :, ::2], env_ids=every_other)
    assert not every_other.is_contiguous() and torch.equal(rew, rew_all[:, :, ::2]) and torch.equal(done, done_all[:, :, ::2])
    _untouched(env, snap)
    assert len(env._look.out) == 1                  # the outputs of the last shape only
    for wrong in ([0, B], [-1]):
        with pytest.raises(ValueError):
            env.lookahead(plans[:, :, :len(wrong)], env_ids=wrong)
    with pytest.raises(ValueError):
        env.lookahead(plans[:, :, :4])
    env.check_errors()


def test_an_ended_episode_under_next_step_reset_is_frozen_from_the_first_row():
    import torch
    cs = LC.case("truncated")
    env = _build(cs, auto_reset="next_step")
    n = env.num_agents
    plans = torch.from_numpy(cs.plans(n)).to(env.device)
    for t in range(5):
        env.step(plans[1, t])
    rew, done = env.lookahead(plans)
    assert not bool(done[:, 0].any()) and bool(done[:, 1:].all())        # two steps are left: the second is the time limit
    env.step(plans[1, 5])
    _, _, d, _ = env.step(plans[1, 6])
    assert bool(d.all())                            # the terminal states: the env's next call is its reset
    snap = _snapshot(env)
    rew, done = env.lookahead(plans)
    assert bool(done.all()) and not bool(rew.any()) and not bool(env.lookahead_errors.any())
    _untouched(env, snap)
    _, r, d, _ = env.step(plans[0, 0])              # ... and it still is
    assert not bool(d.any()) and not bool(r.any()) and bool((env.step_count_t == 0).all())


# ---- fork --------------------------------------------------------------------------------------------------------------------
def _rows_equal(a, b, rows_a, rows_b):
    import torch
    for k in a:
        if k != "version":
            assert torch.equal(a[k][rows_a], b[k][rows_b]), k


@pytest.mark.parametrize("kw", [dict(obs_delta=True), dict(episode_info=True, auto_reset="next_step"), dict()],
                         ids=["obs_delta", "episode_info_levels", "plain"])
def test_fork_copies_rows_and_the_copies_stay_identical(kw):
    import torch
    cs = LC.case("wide_k3")
    B = 12
    env = _build(cs, seeds=cs.seeds[:B], **kw)
    n = env.num_agents
    levels = "episode_info" in kw
    if levels:
        env.set_levels(seeds=torch.arange(B, device=env.device) + 900)
        env.reset()
    gen = torch.Generator(env.device).manual_seed(3)
    for _ in range(6):
        env.step(torch.randint(0, 7, (B, n), device=env.device, generator=gen))
    before = {k: v.clone() for k, v in env.state_dict().items()}
    assert not levels or {"ep_return_t", "episode_level_t", "level_next_t"} <= set(before)
    env.fork([0, 1], [5, 0])                        # row 0 is a source and a destination
    after = env.state_dict()
    _rows_equal(after, before, [5, 0], [0, 1])
    rest = [b for b in range(B) if b not in (5, 0)]
    _rows_equal(after, before, rest, rest)
    assert env._look.launches == 2 and env._look.shadow is None
    # equal actions in a pair: the pair stays byte-identical for ever, observations included (row 0 is now old row 1's twin;
    # then a second pair made from device ids)
    # device ids are not read back: a pair with an id outside the batch copies nothing (and nothing faults); the ids a strided view
    mid = {k: v.clone() for k, v in env.state_dict().items()}
    src = torch.tensor([3, 0, 1, 0, 500, 0, 2, 0], device=env.device)[::2]
    dst = torch.tensor([4, 0, -1, 0, 6, 0, 99, 0], device=env.device)[::2]
    env.fork(src, dst)
    assert env._look.launches == 4
    after = env.state_dict()
    _rows_equal(after, mid, [4], [3])
    rest = [b for b in range(B) if b != 4]
    _rows_equal(after, mid, rest, rest)
    env.check_errors()
    for _ in range(10):
        a = torch.randint(0, 7, (B, n), device=env.device, generator=gen)
        a[0], a[4] = a[1], a[3]
        obs, r, d, info = env.step(a)
        sd = env.state_dict()
        for x, y in ((0, 1), (4, 3)):
            assert torch.equal(obs[x], obs[y]) and torch.equal(r[x], r[y]) and torch.equal(d[x], d[y])
            _rows_equal(sd, sd, [x], [y])
            for k, v in info.items():
                assert torch.equal(v[x], v[y]), k
    with pytest.raises(ValueError):
        env.fork([1, 2], [7, 7])
    with pytest.raises(ValueError):
        env.fork([1, 2], [7])
    env.check_errors()


def test_a_forked_env_in_the_seeds_form_is_reseeded_by_its_own_id():
    """`set_levels(seeds=)`: row b of the env's own bank is env b's.  fork copies the bank ROW, so the copy plays its source's
    level next, can be given another level by its own id, and does not follow its source when that one is re-seeded"""
    import torch
    cs = LC.case("wide_k3")
    B = 12
    env = _build(cs, seeds=cs.seeds[:B])
    n, dev = env.num_agents, env.device
    seeds = 900 + torch.arange(B, device=dev)
    seeds[6], seeds[7] = seeds[3], seeds[1]         # twins of the sources, to compare resets with
    env.set_levels(seeds=seeds)
    env.reset()
    gen = torch.Generator(dev).manual_seed(3)
    for _ in range(4):
        env.step(torch.randint(0, 7, (B, n), device=dev, generator=gen))
    env.fork([3, 1], [4, 2])
    assert torch.equal(env._levels.level_of_env, torch.arange(B, device=dev))
    nxt = env.state_dict()["level_next_t"].cpu().tolist()
    assert (nxt[4], nxt[2], nxt[3], nxt[1]) == (903, 901, 903, 901)
    env.set_levels(seeds=torch.tensor([777, 777], device=dev), env_ids=[4, 8])      # the copy, by its own id (8: its twin)
    env.set_levels(seeds=555, env_ids=[1])                                          # a source: its copy (2) stays on 901
    nxt = env.state_dict()["level_next_t"].cpu().tolist()
    assert (nxt[4], nxt[8], nxt[3], nxt[1], nxt[2]) == (777, 777, 903, 555, 901)
    env.reset()
    lv = env.episode_level.cpu().tolist()
    assert (lv[4], lv[8], lv[3], lv[6], lv[1], lv[2], lv[7]) == (777, 777, 903, 903, 555, 901, 901)
    for a, b in ((4, 8), (3, 6), (2, 7)):
        for k in ("grid_state", "agent_state", "mt_state", "mt_pos", "mt_head"):
            assert torch.equal(getattr(env, k)[a], getattr(env, k)[b]), (a, b, k)
    assert not torch.equal(env.grid_state[4], env.grid_state[3]) and not torch.equal(env.grid_state[1], env.grid_state[2])
    env.check_errors()


def test_shards_lookahead_as_the_one_env_and_fork_within_a_shard():
    import torch
    from marlgrid_amd import envs as E
    cs = LC.case("wide_k3")
    B, K, T = 16, 2, 6
    one = E.make(cs.name, batch_size=B, seed=700, place_obs=False)
    sh = E.make(cs.name, batch_size=B, seed=700, place_obs=False, devices=[0, 0])
    n = one.num_agents
    r = np.random.RandomState(4)
    for _ in range(4):
        a = torch.from_numpy(r.randint(0, 7, (B, n)))
        one.step(a)
        sh.step(a)
    plans = torch.from_numpy(r.randint(0, 7, (K, T, B, n)))
    rew, done = one.lookahead(plans)
    parts = sh.lookahead(plans)
    sh.synchronize()
    assert torch.equal(torch.cat([p[0] for p in parts], dim=2).cpu(), rew.cpu())
    assert torch.equal(torch.cat([p[1] for p in parts], dim=2).cpu(), done.cpu())
    ids = [9, 2, 15]
    parts = sh.lookahead(plans[:, :, ids], env_ids=ids)
    sh.synchronize()
    assert torch.equal(parts[0][0].cpu(), rew[:, :, [2]].cpu()) and torch.equal(parts[1][0].cpu(), rew[:, :, [9, 15]].cpu())
    ids = [2, 3]                                    # none of them on shard 1: it launches nothing and returns empty tensors
    before = [env._look.launches for env in sh.envs]
    parts = sh.lookahead(plans[:, :, ids], env_ids=ids)
    sh.synchronize()
    assert torch.equal(parts[0][0].cpu(), rew[:, :, ids].cpu()) and torch.equal(parts[0][1].cpu(), done[:, :, ids].cpu())
    assert tuple(parts[1][0].shape) == (K, T, 0, n) and tuple(parts[1][1].shape) == (K, T, 0)
    assert [env._look.launches for env in sh.envs] == [before[0] + 2, before[1]]
    with pytest.raises(NotImplementedError):
        sh.fork([1, 9], [2, 3])                     # env 9 lives on shard 1, env 3 on shard 0
    sh.fork([1, 9], [2, 15])
    one.fork([1, 9], [2, 15])
    sh.synchronize()
    a, b = one.state_dict(), sh.state_dict()
    for k in a:
        assert torch.equal(a[k].cpu(), b[k].cpu()), k
