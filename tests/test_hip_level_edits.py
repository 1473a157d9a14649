"""GPU (-m gpu): per-env cell edits — `MultiGridEnv(level_edits=K)`, an EDITS op at the end of the reset program that applies
the env's own list from the table behind the template and the parameter table — replayed by `reset_env` inside every kernel
that resets: mg_reset, the step kernel, the encoded-views kernel, the fused render kernels and a delta instantiation.  The
yardstick is the constant TWIN (tests/edit_envs.py): the same scenario with the list's cells written by put_obj / grid.set at the
end of `_gen_grid`, and the same seeds; tests/test_gen_edits_diff_host.py closes twin == oracle on the CPU.

The constructor's reset of an edits env runs with empty lists and draws other RNG words than a twin's: both sides are seeded
again (`env.seed()`) once the lists are set, then reset."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "native"))

import edit_envs as EE  # noqa: E402

pytestmark = pytest.mark.gpu
REW_TOL = 1e-6
K, T, MAX_STEPS = 4, 40, 10

# every kernel that resets: (constructor kwargs, batch sizes).  B = 67: 4-wave workgroups with a ragged last wave; B = 4 099:
# 16-wave workgroups at their register limit
CASES = {
    "mg_reset": (dict(auto_reset=False), (67,)),
    "step_kernel": (dict(auto_reset=True, fused_step=False), (67,)),
    "pixels": (dict(auto_reset=True), (67, 4099)),
    "encoded": (dict(auto_reset=True, obs_format="encoded"), (67,)),
    "delta_next_step": (dict(auto_reset="next_step", obs_delta=True, episode_info=True), (67, 4099)),
}
E1 = [(name, B) for name, (_, sizes) in CASES.items() for B in sizes]


def _started(env, tab=None):
    """lists set, seeded as the constructor seeded it, reset"""
    if tab is not None:
        env.set_edits(tab)
    env.seed()
    return env.reset()


def _same_info(i1, i2, rows, what):
    import torch
    assert sorted(i1) == sorted(i2), what
    for k in i1:
        assert torch.equal(i1[k][rows], i2[k][rows]), (what, k)


@pytest.mark.parametrize("case,B", E1, ids=["%s-%d" % c for c in E1])
def test_mixed_batch_equals_the_twins(case, B):
    import torch
    kw = dict(batch_size=B, seeds=8100 + np.arange(B), place_obs=False, max_steps=MAX_STEPS, strict=False, **CASES[case][0])
    tab, which = EE.table(K, B)
    env = EE.build(K=K, **kw)
    rows = {i: torch.from_numpy(np.nonzero(which == i)[0]).to(env.device) for i in range(4)}
    obs = _started(env, tab)
    assert torch.equal(env.edits_t.cpu(), torch.from_numpy(tab))
    twins = {i: EE.build(i, K, **kw) for i in range(4)}
    for i, t in twins.items():
        assert torch.equal(_started(t)[rows[i]], obs[rows[i]]), (i, "reset")
    if case == "delta_next_step":
        assert env.kernel_name.startswith("mg::render_kernel<7, 8, ")
    # the lists did what they say (against the twins alone this would hold if neither side applied anything)
    g = env.grid_state[:, :EE.W * EE.H].reshape(B, EE.W, EE.H)
    assert bool((g[rows[1], 7, 7] == EE.WALL).all()) and bool((g[rows[2], 3, 3] == EE.GOAL).all())
    assert bool((g[rows[2], 13, 13] == 0).all()) and bool((g[rows[0], 13, 13] == EE.GOAL).all())
    rng = np.random.RandomState(17)
    ends = torch.zeros(B, dtype=torch.int64, device=env.device)
    for step in range(T):
        a = torch.from_numpy(rng.randint(0, 7, size=(B, EE.N_AGENTS))).to(env.device)
        obs, r, d, info = env.step(a)
        ends += d
        out = [t.step(a) for t in twins.values()]
        for (i, t), (o2, r2, d2, info2) in zip(twins.items(), out):
            m = rows[i]
            assert torch.equal(obs[m], o2[m]) and torch.equal(d[m], d2[m]), (i, step)
            assert float((r[m] - r2[m]).abs().max()) <= REW_TOL, (i, step)
            _same_info(info, info2, m, (i, step))
        if case == "mg_reset" and bool(d.any()):
            mask = d.clone()
            obs = env.reset(env_mask=mask)
            for i, t in twins.items():
                assert torch.equal(t.reset(env_mask=mask)[rows[i]], obs[rows[i]]), (i, step, "reset(env_mask=)")
    assert int(ends.min()) >= T // MAX_STEPS - 1                          # the time limit ends every episode
    if case == "delta_next_step":                                         # every step was the delta launch, in all five envs
        assert env._delta_launches == T and all(t._delta_launches == T for t in twins.values())
    for i, t in twins.items():
        for k in env._STATE_KEYS:                                         # canonical state and the RNG, byte for byte
            assert torch.equal(getattr(env, k)[rows[i]], getattr(t, k)[rows[i]]), (i, k)
    assert not env.grid_state[:, EE.W * EE.H:].any()
    assert not env.error_t.any()


def test_the_device_guards_a_tensor_of_out_of_range_entries():
    """what tests/test_gen_edits_diff_host.py::test_a_garbage_table_changes_nothing pins on the CPU, from a device tensor: an
    entry outside the grid or of a kind without a descriptor is ignored, whatever slot it sits in"""
    import torch
    B = 67
    kw = dict(batch_size=B, seeds=8300 + np.arange(B), place_obs=False, max_steps=MAX_STEPS, auto_reset=True)
    env = EE.build(K=K, **kw)
    twin = EE.build(0, K, **kw)
    n_obj = len(env.obj_reg.objs)
    assert n_obj == 3
    bad = torch.tensor([(EE.W, 5, EE.WALL, 1), (5, EE.H, EE.WALL, 1), (5, 5, n_obj, 1), (255, 255, 255, 255)], device=env.device)
    tab = bad[torch.arange(B * K, device=env.device).reshape(B, K) % 4]     # every entry in every slot position
    assert torch.equal(_started(env, tab), _started(twin))
    assert torch.equal(env.edits_t[:, :, :3], tab[:, :, :3].to(torch.uint8))   # (written as given: nothing was checked on the host)
    rng = np.random.RandomState(19)
    ends = 0
    for step in range(25):
        a = torch.from_numpy(rng.randint(0, 7, size=(B, EE.N_AGENTS)))
        o, r, d, _ = env.step(a)
        o2, r2, d2, _ = twin.step(a)
        assert torch.equal(o, o2) and torch.equal(d, d2) and float((r - r2).abs().max()) <= REW_TOL, step
        ends += int(d.sum())
    assert ends >= 2 * B
    for k in env._STATE_KEYS:
        assert torch.equal(getattr(env, k), getattr(twin, k)), k
    assert not env.grid_state[:, EE.W * EE.H:].any()
    env.check_errors()


def test_a_new_list_waits_for_the_reset_and_a_new_kind_is_known_by_then():
    import torch
    from marlgrid_amd.objects import Goal
    B = 64
    env = EE.build(K=K, batch_size=B, seeds=8500 + np.arange(B), place_obs=False, max_steps=MAX_STEPS, auto_reset=True)
    _started(env)
    # a kind the env has not seen, registered now: valid in the launch that next resets.  (A goal: nobody picks it up or moves
    # it, and the scenario's own is green and sits in the corner)
    key = env.edit_key(Goal(color="blue", reward=1))
    assert key == 3

    def key_at_77():
        return env.grid_state[:, 7 * EE.H + 7] == key
    rng = np.random.RandomState(23)
    current = torch.zeros(B, dtype=torch.bool, device=env.device)
    for step in range(30):
        if step == 4:
            before = env.grid_state.clone()
            env.set_edits(torch.tensor([(7, 7, key, 1)], device=env.device))
            assert torch.equal(env.grid_state, before)
        if step == 15:
            env.set_edits([], env_ids=np.arange(0, B, 2))
        _, _, d, _ = env.step(torch.from_numpy(rng.randint(0, 7, size=(B, EE.N_AGENTS))))
        current = torch.where(d, env.edits_t[:, 0, 3] != 0, current)
        assert torch.equal(key_at_77(), current), step
    assert bool(current[1::2].all()) and not bool(current[0::2].any())
    env.check_errors()


def test_shards_pipeline_and_checkpoint_equal_the_one_env():
    import torch
    B = 24
    kw = dict(batch_size=B, seed=8800, place_obs=False, auto_reset=True, max_steps=MAX_STEPS)
    one = EE.build(K=K, **kw)
    ds = EE.build(K=K, devices=[0, 0], **kw)
    pipe = EE.build(K=K, pipeline=2, **kw)
    tab, which = EE.table(K, B)                                           # global env order
    for e in (one, ds, pipe):
        e.set_edits(tab)
    one.seed(8800)
    ds._each(lambda k, env: env.seed())
    pipe._each(lambda k, env: env.seed())
    o = one.reset()
    assert torch.equal(ds.gather(ds.reset()), o)
    po = pipe.reset()
    pipe.synchronize()
    assert torch.equal(torch.cat(po), o)
    assert torch.equal(torch.cat(ds.edits_t).cpu(), one.edits_t.cpu()) and torch.equal(torch.cat(pipe.edits_t).cpu(), one.edits_t.cpu())
    rng = np.random.RandomState(41)
    resumed = None
    for t in range(30):
        if t == 7:                                          # a change in global order, mid-episode, by id, one list per id
            ids = np.array([23, 0, 11, 12, 5])
            new = np.zeros((5, 2, 4), np.int64)
            new[:, 0] = [(2 + j, 3, EE.WALL, 1) for j in range(5)]
            new[:, 1] = (EE.W - 2, EE.H - 2, 0, 1)
            for e in (one, ds, pipe):
                e.set_edits(new, env_ids=ids)
        if t == 21:                                         # ... and by mask, from a device tensor
            mask = torch.from_numpy(np.arange(B) % 3 == 0).to(one.device)
            lst = torch.tensor([(6, 6, EE.GOAL, 1)], device=one.device)
            for e in (one, ds, pipe, resumed):
                e.set_edits(lst, env_mask=mask)
        a = rng.randint(0, 7, size=(B, EE.N_AGENTS))
        at = torch.from_numpy(a)
        o, r, d, _ = one.step(at)
        o2, r2, d2, _ = ds.gather(ds.step(a))
        assert torch.equal(o, o2) and torch.equal(r, r2) and torch.equal(d, d2), t
        for k in range(2):
            with pipe.on(k):
                part = slice(k * B // 2, (k + 1) * B // 2)
                o3, r3, d3, _ = pipe.step_part(k, at[part].to(one.device))
                torch.cuda.current_stream().synchronize()
                assert torch.equal(o3, o[part]) and torch.equal(r3, r[part]) and torch.equal(d3, d[part]), (t, k)
        if resumed is not None:
            o4, r4, d4, _ = resumed.step(at)
            assert torch.equal(o4, o) and torch.equal(r4, r) and torch.equal(d4, d), t
        if t == 14:                     # mid-episode: the pipeline's checkpoint into a fresh one env, the one env's into the shards
            sd = one.state_dict()
            assert "edits_t" in sd and torch.equal(sd["edits_t"], one.edits_t)
            whole = pipe.state_dict()
            assert sorted(whole) == sorted(sd) and all(torch.equal(whole[k], sd[k].cpu()) for k in sd)
            resumed = EE.build(K=K, **dict(kw, seed=1))
            resumed.reset()
            resumed.load_state_dict({k: v.to(resumed.device) for k, v in whole.items()})
            assert torch.equal(resumed.edits_t, one.edits_t)
            ds.load_state_dict(sd)
    for k in one._STATE_KEYS + ("edits_t",):
        assert torch.equal(getattr(one, k), getattr(resumed, k)), k
    one.check_errors(), resumed.check_errors(), pipe.check_errors()
    for e in ds.envs:
        e.check_errors()


# ---- levels that carry their parameters and edits: a full LevelBank ------------------------------------------------------------
CURRICULUM = "MarlGrid-3AgentClutteredCurriculum15x15-v0"
L = 5
LEVEL_SEEDS = [901, 2 ** 32 + 7, 903, 904, 905]
LEVEL_CLUTTER = [0, 10, 25, 40, 50]
LEVEL_EDITS = [[], [(7, 7, EE.WALL, 1)], EE.lists(K)[2], EE.lists(K)[3], [(5, 5, EE.GOAL, 1), (6, 6, EE.WALL, 0)]]


def _edit_rows(lists_):
    t = np.zeros((len(lists_), K, 4), np.uint8)
    for i, lst in enumerate(lists_):
        if lst:
            t[i, :len(lst)] = np.asarray(lst, np.uint8)
    return t


def _slot_plan(B, T, seed=3):
    """(T + 1, B) slots: what every env is pointed at before the reset (row 0) and before step t (row t + 1); env 7 runs free"""
    ids = np.random.RandomState(seed).randint(0, L, size=(T + 1, B)).astype(np.int64)
    ids[:, 7] = -1
    ids[0, :L] = np.arange(L)                                             # every slot is played from the start
    ids[:, 9] = 2                                                         # ... and env 9 plays slot 2 throughout
    return ids


def _fill(bank):
    bank.assign(None, LEVEL_SEEDS, params=dict(n_clutter=LEVEL_CLUTTER), edits=_edit_rows(LEVEL_EDITS))


def test_full_bank_levels_are_seed_parameters_and_edits():
    import torch
    from marlgrid_amd import envs as E
    B, T2 = 12, 36
    kw = dict(place_obs=False, max_steps=MAX_STEPS, level_edits=K, episode_info=True)
    env = E.make(CURRICULUM, batch_size=B, seed=9100, auto_reset="next_step", **kw)
    dev = env.device
    bank = env.level_bank(L, full=True)
    assert torch.equal(bank.params[:, 0].cpu(), torch.full((L,), 25, dtype=torch.uint8)) and not bank.edits.any()
    _fill(bank)
    plan = _slot_plan(B, T2)
    plan_dev = torch.from_numpy(plan).to(dev)
    acts = torch.from_numpy(np.random.RandomState(29).randint(0, 7, size=(T2, B, EE.N_AGENTS))).to(dev)
    new_seed, new_edits, t_assign = 777, [(9, 9, EE.GOAL, 1), (13, 13, 0, 1)], 17
    new_dev = (torch.tensor([2], device=dev), torch.tensor([new_seed], device=dev), torch.tensor(_edit_rows([new_edits])[0], device=dev))
    free_rows = (env.params_t[7].clone(), env.edits_t[7].clone())
    env.set_levels(bank, plan_dev[0])
    torch.cuda.synchronize()
    launches0 = (env._level_launches, bank.launches)
    # ---- the loop: device tensors only, nothing is read back (what is checked is cloned on the device and looked at afterwards)
    log = [dict(obs=env.reset().clone(), par=env.params_t.clone(), ed=env.edits_t.clone())]
    done = torch.zeros(B, dtype=torch.bool, device=dev)
    for t in range(T2):
        if t == t_assign:                                                 # a slot's level replaced mid-run
            bank.assign(new_dev[0], new_dev[1], edits=new_dev[2])
        env.set_levels(bank, plan_dev[t + 1], env_mask=done)
        obs, r, done, info = env.step(acts[t])
        log.append(dict(obs=obs.clone(), r=r.clone(), d=done.clone(), reset=info["reset"].clone(), level=info["level"].clone(),
                        par=env.params_t.clone(), ed=env.edits_t.clone()))
    assert (env._level_launches - launches0[0], bank.launches - launches0[1]) == (T2 + 1, 1)    # one small launch per call
    # ---- afterwards: every episode of every env, from its first observation on, against a fresh env made for its triple
    torch.cuda.synchronize()
    resets = np.stack([e["reset"].cpu().numpy() for e in log[1:]])        # (T2, B)
    levels = {False: (LEVEL_SEEDS, _edit_rows(LEVEL_EDITS)),              # the bank before and after the assign
              True: (LEVEL_SEEDS[:2] + [new_seed] + LEVEL_SEEDS[3:], _edit_rows(LEVEL_EDITS[:2] + [new_edits] + LEVEL_EDITS[3:]))}
    episodes = []                                                         # (env, log index of its first observation, slot, after)
    for b in range(B):
        episodes.append((b, 0, int(plan[0, b]), False))
        episodes += [(b, t + 1, int(plan[t + 1, b]), t >= t_assign) for t in range(T2) if resets[t, b]]
    assert min(sum(1 for e in episodes if e[0] == b) for b in range(B)) >= 3
    played = [e for e in episodes if e[2] >= 0]
    assert {e[0] for e in episodes if e[2] < 0} == {7} and any(e[2] == 2 and e[3] for e in played)
    starts9 = [e[1] for e in played if e[0] == 9]                         # an episode of slot 2 was running over the assign
    assert any(t0 <= t_assign and not any(t0 < u <= t_assign + 1 for u in starts9) for t0 in starts9)
    for b, t0, slot, after in episodes:                                   # after the reset the env's rows are the slot's
        if slot >= 0:
            assert int(log[t0]["par"][b, 0]) == LEVEL_CLUTTER[slot], (b, t0)
            assert np.array_equal(log[t0]["ed"][b].cpu().numpy(), levels[after][1][slot]), (b, t0)
            if t0:
                assert int(log[t0]["level"][b]) == levels[after][0][slot], (b, t0)
    for e in log:                                                         # ... and the free-running env keeps its own
        assert torch.equal(e["par"][7], free_rows[0]) and torch.equal(e["ed"][7], free_rows[1])
    R = len(played)
    ref = E.make(CURRICULUM, batch_size=R, seeds=[levels[a][0][s] for _, _, s, a in played], auto_reset=False, **kw)
    ref.set_params(n_clutter=np.array([LEVEL_CLUTTER[s] for _, _, s, _ in played]))
    ref.set_edits(np.stack([levels[a][1][s] for _, _, s, a in played]))
    ref.seed()
    o = ref.reset()
    alive = np.ones(R, bool)
    for j, (b, t0, _, _) in enumerate(played):
        assert torch.equal(o[j], log[t0]["obs"][b]), ("first observation", b, t0)
    for k in range(1, MAX_STEPS + 1):
        a = torch.zeros((R, EE.N_AGENTS), dtype=torch.int64, device=dev)
        for j, (b, t0, _, _) in enumerate(played):
            if alive[j] and t0 + k <= T2:
                a[j] = acts[t0 + k - 1, b]
        o, r, d, _ = ref.step(a)
        d = d.cpu().numpy()
        for j, (b, t0, _, _) in enumerate(played):
            if not alive[j] or t0 + k > T2:
                continue
            e = log[t0 + k]
            assert torch.equal(o[j], e["obs"][b]) and bool(e["d"][b]) == bool(d[j]), (b, t0, k)
            assert abs(float(r[j].sum() - e["r"][b].sum())) <= REW_TOL * EE.N_AGENTS and float((r[j] - e["r"][b]).abs().max()) <= REW_TOL
            alive[j] = not d[j]
    assert not alive[[t0 + MAX_STEPS <= T2 for _, t0, _, _ in played]].any()       # every episode that had the time ended
    env.check_errors()


def test_full_bank_through_pipeline_and_device_shards():
    import torch
    from marlgrid_amd import envs as E
    B, T2 = 12, 30
    kw = dict(batch_size=B, seed=9300, place_obs=False, max_steps=MAX_STEPS, level_edits=K, auto_reset="next_step")
    one = E.make(CURRICULUM, **kw)
    ds = E.make(CURRICULUM, devices=[0, 0], **kw)
    pipe = E.make(CURRICULUM, pipeline=2, **kw)
    dev = one.device
    banks = [e.level_bank(L, full=True) for e in (one, ds, pipe)]
    for bank in banks:
        _fill(bank)
    plan = torch.from_numpy(_slot_plan(B, T2)).to(dev)
    for e, bank in zip((one, ds, pipe), banks):
        e.set_levels(bank, plan[0])
    o = one.reset()
    assert torch.equal(ds.gather(ds.reset()), o)
    po = pipe.reset()
    pipe.synchronize()
    assert torch.equal(torch.cat(po), o)
    rng = np.random.RandomState(47)
    done = torch.zeros(B, dtype=torch.bool, device=dev)
    for t in range(T2):
        if t == 11:
            for bank in banks:
                bank.assign([4, 0], [31, 32], params=dict(n_clutter=[3, 44]), edits=[(2, 2, EE.GOAL, 1)])
        for e, bank in zip((one, ds, pipe), banks):
            e.set_levels(bank, plan[t + 1], env_mask=done)
        a = rng.randint(0, 7, size=(B, EE.N_AGENTS))
        at = torch.from_numpy(a)
        o, r, d, _ = one.step(at)
        o2, r2, d2, _ = ds.gather(ds.step(a))
        assert torch.equal(o, o2) and torch.equal(r, r2) and torch.equal(d, d2), t
        for k in range(2):
            with pipe.on(k):
                part = slice(k * B // 2, (k + 1) * B // 2)
                o3, r3, d3, _ = pipe.step_part(k, at[part].to(dev))
                torch.cuda.current_stream().synchronize()
                assert torch.equal(o3, o[part]) and torch.equal(r3, r[part]) and torch.equal(d3, d[part]), (t, k)
        done = d
    for e in (ds, pipe):
        assert torch.equal(torch.cat(e.edits_t).cpu(), one.edits_t.cpu())
        assert torch.equal(torch.cat([p["n_clutter"] for p in e.params]).cpu(), one.params["n_clutter"].cpu())
    one.check_errors(), pipe.check_errors()
    for e in ds.envs:
        e.check_errors()
