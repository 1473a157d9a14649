"""GPU (-m gpu): mg_solve_distance — `env.solve_distance()` / `env.solve_exact` — against tests/solve_ref.py on the state read
back from the env: distance, first action and `exact` on the DoorKey batches right after reset and after 30 random steps, the
grids made by hand and the edge shapes through the bare C ABI (tests/solve_cases.py; the host twin runs the same in
tests/test_solve_distance_host.py), env selection, the refusal of caps that do not fit, pipelines and device shards, and an
end-to-end run in which an agent that follows the policy arrives at exactly the step the distance names with exactly the return
`optimal_return` names."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "native"))

import solve_cases as SC  # noqa: E402
import solve_ref as S  # noqa: E402
from marlgrid_amd import _native as N  # noqa: E402

pytestmark = pytest.mark.gpu


def _reference(env, caps=(2, 2)):
    """solve_ref.layered for the env's state as it is on the device now"""
    flags = env.agent_flags.cpu().numpy()
    pos = env.agent_pos.cpu().numpy()
    in_cell = ((flags & N.AF_ACTIVE) != 0) & ((flags & N.AF_EVICTED) == 0)
    return S.layered(env.grid.grid.cpu().numpy(), S.Kinds.of_env(env), pos[..., 0], pos[..., 1], env.agent_dir.cpu().numpy() & 3,
                     in_cell, env.agent_carrying.cpu().numpy(), *caps)


def _build(name, B, **kw):
    import product_envs
    return product_envs.build(name, batch_size=B, seeds=[1337 + b for b in range(B)], place_obs=False, auto_reset=False, strict=False,
                              **kw)


@pytest.mark.parametrize("name,B,steps", SC.SCENARIOS)
def test_scenarios_match_the_reference(name, B, steps):
    import torch
    env = _build(name, B)
    assert env._goal.solve_dist is None and env.solve_exact is None and env._goal.launches == 0     # nothing until it is asked for
    env.reset()
    gen = torch.Generator(env.device).manual_seed(5)
    for _ in range(steps):
        env.step(torch.randint(0, 7, (B, env.num_agents), device=env.device, generator=gen))
    assert env._goal.solve_dist is None and env._goal.launches == 0
    want = _reference(env)
    dist, act = env.solve_distance(policy=True)
    assert env._goal.launches == 1 and dist.dtype == torch.int32 and act.dtype == torch.int64
    assert dist.shape == act.shape == (B, env.num_agents) and env.solve_exact.shape == (B,) and env.solve_exact.dtype == torch.bool
    assert np.array_equal(dist.cpu().numpy(), want[0])
    assert np.array_equal(act.cpu().numpy(), want[1])
    assert np.array_equal(env.solve_exact.cpu().numpy(), want[2]) and want[2].all()
    assert env.solve_distance() is dist         # the env-owned tensor
    if name == SC.S15:      # no door, no item: goal_distance's numbers
        static = env.goal_distance()
        assert torch.equal(static, dist) and bool((static < 0).any()) and bool((static > 0).any())
    elif steps == 0:
        static = env.goal_distance().cpu().numpy()
        assert (want[0] > 0).all() and (static < 0).sum() > 400
        assert np.array_equal(want[0][static >= 0], static[static >= 0])
    else:
        kinds = S.Kinds.of_env(env)
        carried = np.array([kinds.key_colour(int(c)) >= 0 for c in env.agent_carrying.cpu().numpy().ravel()])
        assert carried.sum() >= 10 and (want[0] < 0).any() and (want[0] > 0).any()
    assert "solve" not in " ".join(env.state_dict().keys())


def test_selection_leaves_other_rows_alone():
    import torch
    B = 67
    env = _build(SC.DK8, B)
    env.reset()
    want = _reference(env)
    sel = np.arange(B) % 3 == 1

    def fresh():
        env.solve_distance(policy=True)
        env._goal.solve_dist.fill_(-7)
        env._goal.solve_act8.fill_(-7)
        env._goal.exact_u8.fill_(7)

    for how in ("mask", "ids", "device_ids"):
        fresh()
        if how == "mask":
            d, a = env.solve_distance(env_mask=torch.from_numpy(sel).to(env.device), policy=True)
        elif how == "ids":
            d, a = env.solve_distance(env_ids=np.nonzero(sel)[0], policy=True)
        else:
            d, a = env.solve_distance(env_ids=torch.from_numpy(np.nonzero(sel)[0]).to(env.device), policy=True)
        d, a, e = d.cpu().numpy(), env._goal.solve_act8.cpu().numpy(), env._goal.exact_u8.cpu().numpy()
        assert np.array_equal(d[sel], want[0][sel]) and np.array_equal(a[sel], want[1][sel]) and (e[sel] == 1).all(), how
        assert (d[~sel] == -7).all() and (a[~sel] == -7).all() and (e[~sel] == 7).all(), how
    # ids outside the batch: refused on the host, ignored from a device tensor (nothing is read back to check them)
    fresh()
    d = env.solve_distance(env_ids=torch.tensor([1, B + 3, -2], device=env.device)).cpu().numpy()
    assert np.array_equal(d[1], want[0][1]) and (np.delete(d, 1, axis=0) == -7).all()
    with pytest.raises(ValueError):
        env.solve_distance(env_ids=[1, B + 3])
    with pytest.raises(ValueError):
        env.solve_distance(env_mask=np.ones(B, bool), env_ids=[0])
    with pytest.raises(ValueError):
        env.solve_distance(max_doors=5)
    with pytest.raises(ValueError):
        env.solve_distance(max_items=-1)


def test_caps_change_what_is_tracked():
    """the same batch with caps (0, 0) is the static analysis; with (4, 3), the largest, it is the default's answer"""
    import torch
    env = _build(SC.DK8, 64)
    env.reset()
    want = _reference(env)
    static = env.goal_distance().clone()
    d00 = env.solve_distance(max_doors=0, max_items=0).clone()
    assert torch.equal(d00, static) and not bool(env.solve_exact.any())
    d43 = env.solve_distance(max_doors=4, max_items=3).clone()
    assert np.array_equal(d43.cpu().numpy(), want[0]) and bool(env.solve_exact.all())


def test_caps_that_do_not_fit_are_refused_before_any_launch():
    from marlgrid_amd.agents import GridAgentInterface
    from marlgrid_amd.envs import EmptyMultiGrid
    env = EmptyMultiGrid(agents=[GridAgentInterface(view_tile_size=8)], grid_size=200, batch_size=2, place_obs=False, auto_reset=False)
    env.reset()
    need = 8 * 200 * 4 * (2 + 12 * 12) + 1024
    with pytest.raises(NotImplementedError, match=r"need %d bytes.*caps that fit: \(0, 0\)$" % need):
        env.solve_distance()
    assert env._goal.launches == 0 and env._goal.solve_dist is None
    assert N.lib().mg_solve_distance_lds_bytes(200, 200, 2, 2) == need > 160 * 1024
    d = env.solve_distance(max_doors=0, max_items=0)
    assert env._goal.launches == 1 and bool((d > 0).all()) and bool(env.solve_exact.all())
    # the bare call answers the same by arithmetic and writes nothing
    d.fill_(-7)
    rc = N.lib().mg_solve_distance(C.byref(env._cfg), C.byref(env._state), None, 1, 0, d.data_ptr(), None, None, None)
    assert rc == N.E_UNSUPPORTED
    for bad in ((5, 0), (0, 4), (-1, 0)):
        assert N.lib().mg_solve_distance(C.byref(env._cfg), C.byref(env._state), None, bad[0], bad[1], d.data_ptr(), None, None,
                                         None) == N.E_ARG
    assert N.lib().mg_solve_distance(C.byref(env._cfg), C.byref(env._state), None, 0, 0, None, None, None, None) == N.E_ARG
    import torch
    torch.cuda.synchronize()
    assert bool((d == -7).all())


def test_pipeline_and_device_shards_equal_the_one_env():
    import torch
    from marlgrid_amd.envs import make
    B = 24
    kw = dict(batch_size=B, seed=4400, place_obs=False, auto_reset=False)
    one = make(SC.DK8, **kw)
    pipe = make(SC.DK8, pipeline=2, **kw)
    ds = make(SC.DK8, devices=["cuda:0", "cuda:0"], **kw)
    one.reset()
    pipe.reset()
    ds.reset()
    d, a = one.solve_distance(policy=True)
    assert bool((d > 0).all())
    for shards in (pipe, ds):
        parts = shards.solve_distance(policy=True)
        shards.synchronize()
        assert torch.equal(torch.cat([p[0] for p in parts]), d) and torch.equal(torch.cat([p[1] for p in parts]), a)
        assert torch.equal(torch.cat(shards.solve_exact), one.solve_exact)
        # selectors are in global env order: envs 3 and 20 live in different shards
        shards._each(lambda k, env: env._goal.solve_dist.fill_(-7))
        parts = shards.solve_distance(env_ids=[3, 20])
        shards.synchronize()
        got = torch.cat(parts)
        keep = torch.ones(B, dtype=torch.bool)
        keep[[3, 20]] = False
        assert torch.equal(got[[3, 20]], d[[3, 20]]) and bool((got[keep.to(got.device)] == -7).all())
        mask = torch.zeros(B, dtype=torch.bool, device=d.device)
        mask[5] = mask[13] = True
        parts = shards.solve_distance(env_mask=mask)
        shards.synchronize()            # (every shard launched on its own stream: joined before anything reads)
        got = torch.cat(parts)
        assert torch.equal(got[mask], d[mask]) and bool((got[~mask & keep.to(got.device)] == -7).all())


# ---- grids made by hand, through the bare C ABI ---------------------------------------------------------------------------------
def _run_case(case, caps):
    """a hostemu_solve.SolveCase uploaded — the config and state mg_solve_distance reads, nothing else filled in — and solved"""
    import torch
    dev = torch.device("cuda:0")
    grid = torch.from_numpy(case.grid).to(dev)
    rec = torch.from_numpy(case.rec.view(np.int64)).to(dev)
    obj = torch.from_numpy(np.frombuffer(bytes(case.obj), np.uint8).copy()).to(dev)
    cfg = N.Config()
    C.memmove(C.addressof(cfg), C.addressof(case.cfg), C.sizeof(N.Config))
    cfg.obj = obj.data_ptr()
    state = N.State()
    state.grid, state.agents = grid.data_ptr(), rec.data_ptr()
    B, n = case.cfg.B, case.cfg.n_agents
    dist = torch.full((B, n), -7, dtype=torch.int32, device=dev)
    act = torch.full((B, n), -7, dtype=torch.int8, device=dev)
    exact = torch.full((B,), 7, dtype=torch.uint8, device=dev)
    rc = N.lib().mg_solve_distance(C.byref(cfg), C.byref(state), None, caps[0], caps[1], dist.data_ptr(), act.data_ptr(),
                                   exact.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, rc
    torch.cuda.synchronize()
    return dist.cpu().numpy(), act.cpu().numpy(), exact.cpu().numpy()


def test_hand_cases_match_the_reference():
    for name, (case, caps, want) in SC.hand_cases().items():
        dist, act, exact = _run_case(case, caps)
        assert np.array_equal(dist, want[0]), (name, dist, want[0])
        assert np.array_equal(act, want[1]), (name, act, want[1])
        assert np.array_equal(exact, want[2].astype(np.uint8)), name


@pytest.mark.parametrize("name", SC.EDGE_SHAPES)
def test_edge_shapes(name):
    case, caps, want = SC.edge(name)
    dist, act, exact = _run_case(case, caps)
    assert np.array_equal(dist, want[0]) and np.array_equal(act, want[1]) and np.array_equal(exact, want[2].astype(np.uint8))


# ---- following the policy ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", SC.FOLLOW)
def test_following_the_policy_pays_what_optimal_return_says(M):
    """MarlGrid-1AgentDoorKey8x8-v0, 512 envs: every step `solve_distance(policy=True)` and its action into `env.step`.  While
    an env runs its distance is the previous one minus 1; the agent is done at exactly step d with the return
    `optimal_return(dist=d0)` names, within the project's 1e-6; where step_count + d > max_steps nothing is earned."""
    import torch
    from marlgrid_amd.envs import make
    B = 512
    env = make(SC.SOLO8, batch_size=B, seeds=1337 + np.arange(B), max_steps=M, auto_reset=False, place_obs=False)
    env.reset()
    dev = env.device
    dist, act = env.solve_distance(policy=True)
    d0 = dist[:, 0].clone().long()
    want = env.optimal_return(dist=dist)[:, 0].clone()
    assert env.max_steps == M and env.reward_decay and bool((d0 > 0).all()) and bool(env.solve_exact.all())
    pays = d0 <= M
    assert torch.equal(want == 0, ~pays) and bool((want[pays] > 0).all()) and bool(pays.any())
    ref_pays, ref_want = SC.follow_expectation(d0.cpu().numpy(), np.zeros(B, np.int64), M)
    assert np.array_equal(ref_pays, pays.cpu().numpy()) and np.abs(ref_want - want.cpu().numpy()).max() <= SC.REW_TOL
    if M < 40:      # the truncation rule is met on both sides
        assert bool((d0 == M).any()) and bool((d0 == M + 1).any())
    done_at = torch.full((B,), -1, dtype=torch.long, device=dev)
    got = torch.zeros(B, dtype=torch.float64, device=dev)
    over = torch.zeros(B, dtype=torch.bool, device=dev)
    used = torch.zeros(7, dtype=torch.bool, device=dev)
    for t in range(1, M + 1):
        dist, act = env.solve_distance(policy=True)
        run = ~over
        assert torch.equal(dist[run, 0].long(), d0[run] - (t - 1)), t
        used[act[run, 0]] = True
        _, rew, done, _ = env.step(act)
        got += torch.where(over, torch.zeros_like(got), rew[:, 0].double())      # an env that is done pays nothing that counts
        newly = env.agent_done[:, 0] & (done_at < 0) & ~over
        done_at = torch.where(newly, torch.full_like(done_at, t), done_at)
        over = over | done
    env.check_errors()
    assert bool(over.all())
    assert torch.equal(done_at[pays], d0[pays])
    assert float((got[pays] - want[pays]).abs().max()) <= SC.REW_TOL
    assert bool((done_at[~pays] < 0).all()) and bool((got[~pays] == 0).all())
    if M >= 40:
        assert used.cpu().tolist() == [True, True, True, True, False, True, False]
