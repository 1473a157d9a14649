"""GPU (-m gpu): mg_goal_distance — `env.goal_distance()` / `optimal_return()` — against tests/goal_ref.py on the state read
back from the env, the register-resident kernel and the LDS kernel forced in turn and held to each other, env selection,
pipelines and device shards, the mazes and the hand-made grids through the bare C ABI, and an end-to-end run in which an agent
that follows the field arrives at exactly the step the field names with exactly the return `optimal_return` names.

Further down: the edge shapes of both kernels (tests/goal_cases.py); what a cell is, read from what one `forward` of the step
launch does (tests/goal_probe.py), held to the flag rule and to the field; the field followed from the middle of an episode and
across truncation; and the running use — `goal_distance(env_mask=info["reset"])` every step under auto-reset — against a host
mirror, with the bound that no episode returns more than `optimal_return` said at its start."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "native"))

import goal_ref as G  # noqa: E402
from marlgrid_amd import _native as N  # noqa: E402

pytestmark = pytest.mark.gpu
REW_TOL = 1e-6          # the project's reward tolerance
IN_CELL = N.AF_ACTIVE | N.AF_PLACED
S15, S11 = "MarlGrid-3AgentCluttered15x15-v0", "MarlGrid-3AgentCluttered11x11-v0"


def _reference(env):
    """(dist, field) of goal_ref for the env's state as it is on the device now"""
    free, goal = G.classify(env.grid.grid.cpu().numpy(), *G.kinds_of(env))
    field = G.field_levels(free, goal)
    dist = G.agents_from_field(field, env.agent_pos.cpu().numpy(), env.agent_dir.cpu().numpy(), env.agent_flags.cpu().numpy())
    return dist, field


def _both_paths(env, want_dist, want_field):
    """the two kernels in turn, each with and without the field, into sentinel-filled tensors"""
    import torch
    out = {}
    for path in ("reg", "lds"):
        env.goal_distance()                 # (makes the tensors)
        env._goal.dist.fill_(-7)
        d = env.goal_distance(_path=path).clone()
        env._goal.dist.fill_(-7)
        d2, f = env.goal_distance(field=True, _path=path)
        assert torch.equal(d, d2), path
        assert np.array_equal(d.cpu().numpy(), want_dist), path
        assert np.array_equal(f.cpu().numpy(), want_field), path
        out[path] = (d2.clone(), f.clone())
    assert torch.equal(out["reg"][0], out["lds"][0]) and torch.equal(out["reg"][1], out["lds"][1])
    env._goal.dist.fill_(-7)
    assert np.array_equal(env.goal_distance().cpu().numpy(), want_dist)        # the path the launcher picks itself


@pytest.mark.parametrize("name,B,steps", [(S15, 1, 0), (S15, 7, 30), (S15, 4099, 0), (S15, 4099, 30), (S11, 512, 0),
                                          (S11, 512, 30), ("Test-4AgentEmpty5x5-crowded", 64, 0),
                                          ("Test-4AgentEmpty5x5-crowded", 64, 30)])
def test_scenarios_match_the_reference(name, B, steps):
    import product_envs
    import torch
    env = product_envs.build(name, batch_size=B, seeds=[1337 + b for b in range(B)], place_obs=False, auto_reset=False, strict=False)
    assert env._goal.dist is None and env._goal.launches == 0      # nothing until it is asked for
    env.reset()
    gen = torch.Generator(env.device).manual_seed(5)
    for _ in range(steps):
        env.step(torch.randint(0, 7, (B, env.num_agents), device=env.device, generator=gen))
    dist, field = _reference(env)
    if B >= 512 and name == S15 and steps == 0:
        assert (dist < 0).any() and (dist > 0).any()
    if steps and B >= 512 and "Cluttered" in name:
        assert (env.agent_flags.cpu().numpy() & N.AF_ACTIVE == 0).any()        # done agents give -1
    _both_paths(env, dist, field)


def test_wide_grid_takes_the_lds_kernel():
    """30 x 30 does not fit a wave's registers: the launcher's own pick is the LDS kernel, and forcing the other is refused"""
    import product_envs
    B = 64
    env = product_envs.build("Custom-8AgentCluttered30x30", batch_size=B, seeds=[1337 + b for b in range(B)], place_obs=False,
                             auto_reset=False, strict=False)
    env.reset()
    dist, field = _reference(env)
    d, f = env.goal_distance(field=True)
    assert np.array_equal(d.cpu().numpy(), dist) and np.array_equal(f.cpu().numpy(), field)
    with pytest.raises(RuntimeError, match="unsupported"):
        env.goal_distance(_path="reg")


def test_selection_leaves_other_rows_alone():
    import torch
    from marlgrid_amd.envs import make
    B = 67
    env = make(S15, batch_size=B, seed=1337, place_obs=False, auto_reset=False)
    env.reset()
    dist, field = _reference(env)
    for path in ("reg", "lds"):
        for how in ("mask", "ids", "device_ids"):
            env.goal_distance(field=True)
            env._goal.dist.fill_(-7)
            env._goal.field.fill_(-7)
            sel = np.arange(B) % 3 == 1
            if how == "mask":
                d, f = env.goal_distance(env_mask=torch.from_numpy(sel).to(env.device), field=True, _path=path)
            elif how == "ids":
                d, f = env.goal_distance(env_ids=np.nonzero(sel)[0], field=True, _path=path)
            else:
                d, f = env.goal_distance(env_ids=torch.from_numpy(np.nonzero(sel)[0]).to(env.device), field=True, _path=path)
            d, f = d.cpu().numpy(), f.cpu().numpy()
            assert np.array_equal(d[sel], dist[sel]) and np.array_equal(f[sel], field[sel]), (path, how)
            assert (d[~sel] == -7).all() and (f[~sel] == -7).all(), (path, how)
    # ids outside the batch: refused on the host, ignored from a device tensor (nothing is read back to check them)
    env._goal.dist.fill_(-7)
    d = env.goal_distance(env_ids=torch.tensor([1, B + 3, -2], device=env.device)).cpu().numpy()
    assert np.array_equal(d[1], dist[1]) and (np.delete(d, 1, axis=0) == -7).all()
    with pytest.raises(ValueError):
        env.goal_distance(env_ids=[1, B + 3])
    with pytest.raises(ValueError):
        env.goal_distance(env_mask=np.ones(B, bool), env_ids=[0])
    assert "goal" not in " ".join(env.state_dict().keys())


def test_pipeline_and_device_shards_equal_the_one_env():
    import torch
    from marlgrid_amd.envs import make
    B = 24
    kw = dict(batch_size=B, seed=4400, place_obs=False, auto_reset=False)
    one = make(S15, **kw)
    pipe = make(S15, pipeline=2, **kw)
    ds = make(S15, devices=["cuda:0", "cuda:0"], **kw)
    one.reset()
    pipe.reset()
    ds.reset()
    d, f = one.goal_distance(field=True)
    for shards in (pipe, ds):
        parts = shards.goal_distance(field=True)
        shards.synchronize()
        assert torch.equal(torch.cat([p[0] for p in parts]), d) and torch.equal(torch.cat([p[1] for p in parts]), f)
        # selectors are in global env order: envs 3 and 20 live in different shards
        shards._each(lambda k, env: (env._goal.dist.fill_(-7), env._goal.field.fill_(-7)))
        parts = shards.goal_distance(env_ids=[3, 20])
        shards.synchronize()
        got = torch.cat(parts)
        keep = torch.ones(B, dtype=torch.bool)
        keep[[3, 20]] = False
        assert torch.equal(got[[3, 20]], d[[3, 20]]) and (got[keep.to(got.device)] == -7).all()
        mask = torch.zeros(B, dtype=torch.bool, device=d.device)
        mask[5] = mask[13] = True
        parts = shards.goal_distance(env_mask=mask)
        shards.synchronize()            # (every shard launched on its own stream: joined before anything reads)
        got = torch.cat(parts)
        assert torch.equal(got[mask], d[mask])


# ---- grids made by hand, through the bare C ABI ---------------------------------------------------------------------------
class _Device(object):
    """a hostemu_goal.RawCase uploaded: the config and state mg_goal_distance reads, nothing else filled in"""

    def __init__(self, case):
        import torch
        self.case = case
        dev = torch.device("cuda:0")
        self.grid = torch.from_numpy(case.grid).to(dev)
        self.rec = torch.from_numpy(case.rec.view(np.int64)).to(dev)
        self.obj = torch.from_numpy(np.frombuffer(bytes(case.obj), np.uint8).copy()).to(dev)
        self.cfg = N.Config()
        C.memmove(C.addressof(self.cfg), C.addressof(case.cfg), C.sizeof(N.Config))
        self.cfg.obj = self.obj.data_ptr()
        self.state = N.State()
        self.state.grid, self.state.agents = self.grid.data_ptr(), self.rec.data_ptr()
        B, W, H, n = case.cfg.B, case.cfg.W, case.cfg.H, case.cfg.n_agents
        self.dist = torch.full((B, n), -7, dtype=torch.int32, device=dev)
        self.field = torch.full((B, W, H, 4), -7, dtype=torch.int32, device=dev)

    def run(self, path, field=True):
        import torch
        self.dist.fill_(-7)
        self.field.fill_(-7)
        rc = N.lib().mg_goal_distance_path(C.byref(self.cfg), C.byref(self.state), None, self.dist.data_ptr(),
                                           self.field.data_ptr() if field else None, path,
                                           C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, rc
        torch.cuda.synchronize()
        return self.dist.cpu().numpy(), self.field.cpu().numpy()


def _check_raw(grid, agents):
    import hostemu_goal as HG
    case = HG.RawCase(grid, agents)
    free, goal = G.classify(np.asarray(grid), *case.kinds())
    field = np.stack([G.field_queue(free[b], goal[b]) for b in range(free.shape[0])])
    dist = G.agents_from_field(field, *G.unpack_records(case.rec))
    return _check_case(case, dist, field)


def _check_case(case, dist, field, without_field=None):
    """without_field: also run without the field (the sentinel rows untouched); by default where W * H <= 10 000"""
    dev = _Device(case)
    W, H = case.cfg.W, case.cfg.H
    fits = 4 * W <= 64 and H <= 64
    # (a grid that does not fit a wave's registers: the launcher's own pick IS the LDS kernel — test_wide_grid_takes_the_lds_kernel)
    for path in ([N.GOAL_PATH_REG, N.GOAL_PATH_AUTO] if fits else []) + [N.GOAL_PATH_LDS]:
        d, f = dev.run(path)
        assert np.array_equal(d, dist) and np.array_equal(f, field), path
        if (W * H <= 10000) if without_field is None else without_field:      # (the largest maze is 32 509 levels a run: once)
            d, f = dev.run(path, field=False)
            assert np.array_equal(d, dist) and (f == -7).all(), path
    return dist, field


def _walled(W, H, B):
    import hostemu_goal as HG
    g = np.zeros((B, W, H), np.uint8)
    g[:, 0, :] = g[:, -1, :] = g[:, :, 0] = g[:, :, -1] = HG.RawCase.WALL
    return g


@pytest.mark.parametrize("W,H", sorted(G.MAZES))
def test_mazes(W, H):
    import hostemu_goal as HG
    wall, goal = G.serpentine(W, H)
    g = np.zeros((2, W, H), np.uint8)
    g[:, wall] = HG.RawCase.WALL
    g[:, goal[0], goal[1]] = HG.RawCase.GOAL
    if H > 5:
        g[1, 1, H - 2] = HG.RawCase.WALL      # env 1: the first corridor sealed
    dist, _ = _check_raw(g, [[(1, 1, 0, IN_CELL)], [(1, 1, 0, IN_CELL)]])
    assert dist[0, 0] == G.MAZES[(W, H)] and dist[1, 0] == (-1 if H > 5 else G.MAZES[(W, H)])


def test_hand_cases():
    import hostemu_goal as HG
    R = HG.RawCase
    g = _walled(5, 5, 2)
    g[:, 3, 2] = R.GOAL
    g[1, 2, 2] = g[1, 3, 1] = g[1, 3, 3] = R.WALL
    agents = [[(2, 2, 0, IN_CELL), (2, 2, 1, IN_CELL), (2, 2, 2, IN_CELL), (3, 2, 0, IN_CELL), (1, 1, 0, 0),
               (1, 1, 0, IN_CELL | N.AF_EVICTED)],
              [(3, 2, 0, IN_CELL), (3, 2, 3, IN_CELL), (1, 1, 0, IN_CELL), (1, 1, 0, N.AF_DONE), (1, 3, 2, IN_CELL),
               (1, 2, 1, IN_CELL)]]
    dist, _ = _check_raw(g, agents)
    assert dist[0].tolist() == [1, 2, 3, 5, -1, -1] and dist[1].tolist() == [-1] * 6


def test_other_grids():
    import hostemu_goal as HG
    R = HG.RawCase
    g = _walled(7, 7, 5)
    a = [[(1, 1, 0, IN_CELL), (5, 3, 2, IN_CELL)] for _ in range(5)]
    g[0, 5, 5] = g[0, 1, 5] = R.GOAL                               # two goals; env 1: none
    g[2, 5, 5] = R.GOAL                                            # a goal behind lava
    g[2, 4, 1:6] = R.LAVA
    g[3, 5, 5] = R.GOAL                                            # ... behind a closed door
    g[3, 4, 1:6] = R.WALL
    g[3, 4, 3] = R.DOOR_CLOSED
    g[4] = g[3]                                                    # ... and behind an open one
    g[4, 4, 3] = R.DOOR_OPEN
    a[3][1] = a[4][1] = (3, 3, 0, IN_CELL)
    dist, field = _check_raw(g, a)
    assert (dist[0] > 0).all() and (dist[1] == -1).all() and (field[1] == -1).all()
    assert dist[2].tolist() == [-1, 3] and dist[3].tolist() == [-1, -1] and (dist[4] > 0).all()


def test_border_cell_emptied_by_set_edits():
    """a 7 x 7 room whose border cell (6, 3) an edit empties, an agent facing out through it: nothing wraps, nothing is read
    outside the grid, and the emptied cell is a cell like any other"""
    import torch
    from marlgrid_amd.agents import GridAgentInterface
    from marlgrid_amd.envs import EmptyMultiGrid
    env = EmptyMultiGrid(agents=[GridAgentInterface(color="red", view_size=7, view_tile_size=8) for _ in range(2)], grid_size=7,
                         batch_size=2, seed=3, level_edits=2, auto_reset=False, place_obs=False)
    env.set_edits(np.array([[6, 3, 0, 1]], np.uint8), env_ids=[1])
    env.reset()
    assert env.grid.grid[1, 6, 3].item() == 0 and env.grid.grid[0, 6, 3].item() != 0
    env.set_agent(0, x=5, y=3, dir=0)
    env.set_agent(1, x=5, y=5, dir=3, env_mask=torch.tensor([True, False]))
    env.set_agent(1, x=6, y=3, dir=0, env_mask=torch.tensor([False, True]))
    dist, field = _reference(env)
    for b in range(2):
        free, goal = G.classify(env.grid.grid[b].cpu().numpy(), *G.kinds_of(env))
        for k in range(2):
            x, y = env.agent_pos[b, k].tolist()
            assert dist[b, k] == G.agent_bfs(free, goal, x, y, int(env.agent_dir[b, k]))
    assert dist[1, 1] > 0 and (field[1, 6, 3] > 0).all() and (field[0, 6, 3] == -1).all()
    _both_paths(env, dist, field)


def test_following_the_field_arrives_when_it_says():
    """MarlGrid-1AgentCluttered15x15-v0, 512 envs: every step the agent takes the action whose successor state has the smaller
    field value.  Every env with d >= 0 sees its agent done at exactly step d, with the reward optimal_return names; no env
    with d = -1 finishes before max_steps."""
    import torch
    from marlgrid_amd.envs import make
    B = 512
    env = make("MarlGrid-1AgentCluttered15x15-v0", batch_size=B, seeds=1337 + np.arange(B), place_obs=False, auto_reset=False,
               strict=False)
    env.reset()
    dev, W, H = env.device, env.width, env.height
    dist, field = env.goal_distance(field=True)
    d0 = dist[:, 0].clone().long()
    want = env.optimal_return(dist)[:, 0].clone()
    assert (d0 >= 0).any() and (d0 < 0).any() and int(d0.max()) < env.max_steps
    assert torch.equal(want == 0, d0 < 0)
    big = torch.iinfo(torch.int32).max
    f = torch.where(field < 0, torch.full_like(field, big), field).long()
    dx = torch.tensor([1, 0, -1, 0], device=dev)
    dy = torch.tensor([0, 1, 0, -1], device=dev)
    b = torch.arange(B, device=dev)
    done_at = torch.full((B,), -1, dtype=torch.long, device=dev)
    gen = torch.Generator(dev).manual_seed(11)
    got = torch.zeros(B, dtype=torch.float64, device=dev)
    goal_id = [i for i, o in enumerate(env.obj_reg.objs) if type(o).__name__ == "Goal"]
    for t in range(1, env.max_steps + 1):
        pos, d = env.agent_pos[:, 0], env.agent_dir[:, 0]
        x, y = pos[:, 0], pos[:, 1]
        fx, fy = (x + dx[d]).clamp(0, W - 1), (y + dy[d]).clamp(0, H - 1)
        ahead = env.grid.grid[b, fx, fy].long()
        enters = torch.zeros(B, dtype=torch.bool, device=dev)
        for gid in goal_id:
            enters |= ahead == gid
        here = f[b, x, y, d]
        v_left, v_right, v_fwd = f[b, x, y, (d + 3) & 3], f[b, x, y, (d + 1) & 3], f[b, fx, fy, d]
        v_fwd = torch.where(enters, torch.zeros_like(v_fwd), v_fwd)      # entering the goal: nothing left to do
        vals = torch.stack([v_left, v_right, v_fwd], 1)                   # action ids 0, 1, 2
        act = vals.argmin(1)
        # an agent without a path has nothing to follow (three equal values: it would turn left for ever): it acts at random
        # — left / right / forward —, so that a goal it CAN reach after all is reached and the last assertion fails
        act = torch.where(here >= big, torch.randint(0, 3, (B,), device=dev, generator=gen), act)
        ok = (here >= big) | (vals.min(1).values == here - 1)             # the field is consistent: one action, one less
        active = env.agent_active[:, 0]
        assert bool(ok[active].all())
        _, rew, done, _ = env.step(act.unsqueeze(1))
        newly = env.agent_done[:, 0] & (done_at < 0)
        done_at = torch.where(newly, torch.full_like(done_at, t), done_at)
        got += rew[:, 0].double()
    reach = d0 >= 0
    assert torch.equal(done_at[reach], d0[reach])
    assert float((got[reach] - want[reach]).abs().max()) <= REW_TOL
    assert bool((done_at[~reach] < 0).all()) and float(got[~reach].abs().max() if (~reach).any() else 0.0) == 0.0


def test_optimal_return_rules():
    import torch
    from marlgrid_amd.envs import make
    from marlgrid_amd.objects import Goal
    env = make(S11, batch_size=4, seed=1, place_obs=False, auto_reset=False)
    env.reset()
    d = torch.tensor([[0, 1, -1], [10, env.max_steps, env.max_steps + 1]] * 2, dtype=torch.int32, device=env.device)
    v = env.optimal_return(d).cpu().numpy()
    R, M = 1.0, float(env.max_steps)
    assert v.dtype == np.float64 and v.shape == (4, 3)
    assert np.allclose(v[0], [R, R * (1 - 0.9 / M), 0.0], atol=1e-15) and np.allclose(v[1], [R * (1 - 9.0 / M), R * 0.1, 0.0], atol=1e-15)
    env.reward_decay = False
    assert np.array_equal(env.optimal_return(d).cpu().numpy()[1], [R, R, 0.0])
    env.obj_reg.get_key(Goal(color="green", reward=2))
    with pytest.raises(ValueError):
        env.optimal_return(d)


def test_contract_error_codes():
    """bare ctypes: MG_E_ARG for null pointers and sizes outside the bounds, MG_E_UNSUPPORTED for a kernel forced on a shape
    it does not take; nothing is launched"""
    import hostemu_goal as HG
    L = N.lib()
    dev = _Device(HG.RawCase(_walled(5, 5, 1), [[(1, 1, 0, IN_CELL)]]))
    cfg, st, dist = C.byref(dev.cfg), C.byref(dev.state), dev.dist.data_ptr()
    assert L.mg_goal_distance(None, st, None, dist, None, None) == N.E_ARG
    assert L.mg_goal_distance(cfg, None, None, dist, None, None) == N.E_ARG
    assert L.mg_goal_distance(cfg, st, None, None, None, None) == N.E_ARG
    for field, bad in (("W", 0), ("W", 256), ("H", 256), ("n_agents", 0), ("n_agents", 33), ("cells_stride", 24), ("n_obj", 0)):
        c2 = N.Config()
        C.memmove(C.addressof(c2), C.addressof(dev.cfg), C.sizeof(N.Config))
        setattr(c2, field, bad)
        assert L.mg_goal_distance(C.byref(c2), st, None, dist, None, None) == N.E_ARG, field
    s2 = N.State()
    s2.agents = dev.state.agents
    assert L.mg_goal_distance(cfg, C.byref(s2), None, dist, None, None) == N.E_ARG
    assert L.mg_goal_distance_path(cfg, st, None, dist, None, 3, None) == N.E_ARG
    wide = _Device(HG.RawCase(_walled(17, 5, 1), [[(1, 1, 0, IN_CELL)]]))
    assert L.mg_goal_distance_path(C.byref(wide.cfg), C.byref(wide.state), None, wide.dist.data_ptr(), None, N.GOAL_PATH_REG, None) \
        == N.E_UNSUPPORTED
    assert L.mg_goal_distance(cfg, st, None, dist, None, None) == 0


# ---- the edge shapes of both kernels (tests/goal_cases.py; tests/test_goal_distance_host.py runs the same on the host builds) ----
def _edge_shapes():
    import goal_cases
    return goal_cases.REG_SHAPES + goal_cases.LDS_SHAPES


@pytest.mark.parametrize("W,H", _edge_shapes())
def test_edge_shapes(W, H):
    """goal_reg_kernel with lane 63 owning a plane (W = 16), bit 63 (H = 64), W != H, one column, one row and 32 agents on at
    most 12 plane lanes; goal_lds_kernel one past each of the other's limits, with H on both sides of every word boundary, and
    around 64 KiB of dynamic LDS: 146 x 193 asks for exactly 65 536 bytes without the attribute, 147 x 193 for 65 984 with it
    (what a process accepts there BEFORE any larger grid raised the kernel's limit: test_first_lds_launch_of_a_process_at_64_kib).
    Each path the shape admits, with the field and without (the sentinel rows untouched) at every shape; the coverage conditions
    are asserted on the reference's field in goal_cases.edge."""
    import goal_cases
    case, dist, field = goal_cases.edge(W, H)
    fits = goal_cases.reg_fits(W, H)
    assert fits == ((W, H) in goal_cases.REG_SHAPES)
    _check_case(case, dist, field, without_field=True)     # (at most 377 levels a run, at 146 x 193)
    if not fits:
        import torch
        dev = _Device(case)
        rc = N.lib().mg_goal_distance_path(C.byref(dev.cfg), C.byref(dev.state), None, dev.dist.data_ptr(), dev.field.data_ptr(),
                                           N.GOAL_PATH_REG, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert rc == N.E_UNSUPPORTED and bool((dev.dist == -7).all()) and bool((dev.field == -7).all())


@pytest.mark.parametrize("W,H,attribute", [(146, 193, False), (147, 193, True)])
def test_first_lds_launch_of_a_process_at_64_kib(W, H, attribute):
    """hipFuncSetAttribute acts on the function for the rest of the process, and the mazes raise goal_lds_kernel's limit before
    test_edge_shapes runs: what THIS process accepts at 65 536 bytes says nothing.  A fresh child process (tests/goal_first_launch.py)
    whose first goal_lds_kernel launch is 146 x 193 — exactly 64 KiB of dynamic LDS, `lds > 64 * 1024` false, no attribute set —
    must get return code 0 and the reference's numbers; and one whose first is 147 x 193, 65 984 bytes with the attribute."""
    import subprocess
    import goal_cases
    assert (goal_cases.scratch_bytes(W, H) > 64 * 1024) == attribute
    here = os.path.dirname(os.path.abspath(__file__))
    out = subprocess.run([sys.executable, os.path.join(here, "goal_first_launch.py"), str(W), str(H)], stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, universal_newlines=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:]
    assert "FIRST_LDS_LAUNCH_OK %d %d %d" % (W, H, goal_cases.scratch_bytes(W, H)) in out.stdout, out.stdout[-2000:]


# ---- what a cell is, read from what `forward` does (tests/goal_probe.py; the oracle's verdicts: tests/test_oracle_goal_kinds.py) ----
def _probe(name, prepare=None):
    """-> (env, env 0's pre-step grid, the agents' cells after reset, verdict map, counts, env 0's field per path)"""
    import goal_probe as P
    import product_envs
    import scenarios
    import torch
    spec = scenarios.registered(name)
    plan = P.Plan(spec["W"], spec["H"])
    B = plan.B
    env = product_envs.build(name, batch_size=B, seeds=[P.SEED] * B, place_obs=False, auto_reset=False, strict=False)
    env.reset()
    if prepare is not None:
        prepare(env)
    grid = env.grid.grid.cpu().numpy()
    rec = env.agent_state.cpu().numpy()
    pos0, _, flags = G.unpack_records(rec)
    P.assert_probe_ready(grid, flags)
    fields = {}
    for path in (["reg"] if 4 * plan.W <= 64 and plan.H <= 64 else []) + ["lds", None]:
        env.goal_distance(field=True)
        env._goal.field.fill_(-7)
        fields[path] = env.goal_distance(env_ids=[0], field=True, _path=path)[1].cpu().numpy()
        assert (fields[path][1:] == -7).all()
        fields[path] = fields[path][0]
    env.agent_state[:, 0] = torch.from_numpy(plan.records(rec[:, 0]).view(np.int64)).to(env.device)
    _, rew, _, _ = env.step(torch.from_numpy(plan.actions(env.num_agents)).to(env.device))
    pos, _, fl = G.unpack_records(env.agent_state.cpu().numpy())
    want_err = plan.errors(grid[0], env, pos[:, 0])     # (strict=False: the probes that leave a wall record what upstream raises)
    assert np.array_equal(env.error_t.cpu().numpy(), want_err) and (want_err != 0).any() and (want_err == 0).any()
    with pytest.raises(AssertionError):
        env.check_errors()
    assert np.array_equal(pos[~plan.probed, 0], pos0[~plan.probed, 0])
    verdict, counts = plan.verdicts(pos[:, 0], (fl[:, 0] & N.AF_DONE) != 0, rew[:, 0].cpu().numpy())
    return env, grid[0], pos0[0], verdict, counts, fields


def _hold_probe(env, grid, verdict, fields, leave_out=()):
    import goal_probe as P
    return P.hold(*G.classify(grid, *G.kinds_of(env)), verdict, fields, leave_out)


def _probe_scenes():
    import goal_probe as P
    return P.SCENES


@pytest.mark.parametrize("name", _probe_scenes())
def test_probed_cells_are_the_rule_and_give_the_field(name):
    """every state of one grid probed with one `forward` of the step launch, in 4 W H envs: the verdicts equal the flag rule cell
    for cell, and the reverse queue search over the PROBED maps equals the field of both kernels for that grid"""
    import goal_probe as P
    env, grid, pos0, verdict, counts, fields = _probe(name)
    if name == "Limit-3Agent100Kinds24x24":
        assert len(np.unique(grid)) == 102 and sorted(fields, key=str) == [None, "lds"]
        assert counts == (1800, 64, 232), counts        # (what the host build of the step bodies gives)
    if name == P.NOGHOST:       # other agents block: exactly the two cells under agents 1 and 2 read differently
        others = [(int(x), int(y)) for x, y in pos0[1:]]
        assert len(set(others)) == 2 and not env.ghost_mode
        want = _hold_probe(env, grid, verdict, fields, leave_out=others)
    else:
        assert env.ghost_mode
        want = _hold_probe(env, grid, verdict, fields)
    if name == "Edge-HumanPlayerConfig":        # bonus tiles, no goal
        assert (verdict != P.GOAL).all() and (want == -1).all()
    else:
        assert (want > 0).any() and (want == -1).any()


def test_zoo_of_kinds():
    """a 9 x 7 room, one object of every kind put after the constructor — goal_distance right after the registry and the object
    table grew —: the step's verdict per kind is the table of MultiGridEnv.goal_distance's docstring — free: open Door, Floor,
    BonusTile; goal: Goal; everything else blocks"""
    import goal_probe as P
    from marlgrid_amd import objects as PO
    zoo = P.zoo_objects(PO)
    placed = {}

    def prepare(env):
        pos = env.agent_pos.cpu().numpy()
        assert (pos == pos[0]).all()
        n_before = len(env.obj_reg.objs)
        for (kind, obj), (x, y) in zip(zoo, P.zoo_cells(env.width, env.height, pos[0])):
            env.put_obj(obj, x, y)
            placed[kind] = (x, y)
        assert len(env.obj_reg.objs) > n_before

    env, grid, _, verdict, _, fields = _probe(P.ZOO, prepare)
    assert sorted(fields, key=str) == [None, "lds", "reg"] and env.batch_size == 252
    assert len({int(grid[c]) for c in placed.values()}) == len(zoo)
    assert [verdict[placed[kind]] for kind, _ in zoo] == P.ZOO_VERDICTS
    want = _hold_probe(env, grid, verdict, fields)
    assert (want > 0).any()


# ---- following the field from the middle of an episode and across truncation ---------------------------------------------------
@pytest.mark.parametrize("M,warm", [(14, 0), (20, 6), (100, 30)])
def test_following_the_field_pays_what_optimal_return_says(M, warm):
    """MarlGrid-1AgentCluttered15x15-v0, 512 envs, `warm` steps of left / right / forward (numpy's RandomState(9), as
    tests/test_goal_distance_host.py draws them), then the field is followed.  Where d >= 0 and step_count + d <= max_steps the
    agent is done at exactly step d and its return is optimal_return's within REW_TOL; everywhere else optimal_return is 0 and
    nothing is earned — at step_count + d == max_steps + 1 the episode is truncated one step before the goal.  Rewards count
    until the env is done."""
    import torch
    from marlgrid_amd.envs import make
    B = 512
    env = make("MarlGrid-1AgentCluttered15x15-v0", batch_size=B, seeds=1337 + np.arange(B), max_steps=M, auto_reset=False,
               place_obs=False)
    env.reset()
    dev, W, H = env.device, env.width, env.height
    rng = np.random.RandomState(9)
    over = torch.zeros(B, dtype=torch.bool, device=dev)
    for _ in range(warm):
        over = env.step(torch.from_numpy(rng.randint(0, 3, size=(B, 1))).to(dev))[2].clone()
    dist, field = env.goal_distance(field=True)
    d0 = dist[:, 0].clone().long()
    want = env.optimal_return(dist)[:, 0].clone()
    sc = env.step_count.clone().long()
    assert env.max_steps == M and env.reward_decay and bool((sc[~over] == warm).all()) and bool((d0[over] < 0).all())
    t_goal = sc + d0
    pays = (d0 >= 0) & (t_goal <= M)
    assert bool(pays.any()) and bool((d0 < 0).any())
    if M < 100:     # the truncation rule is met on both sides
        assert bool(((d0 >= 0) & (t_goal == M)).any()) and bool(((d0 >= 0) & (t_goal == M + 1)).any())
    else:
        assert warm == 30 and bool((sc[~over] == 30).all())
    assert torch.equal(want == 0, ~pays) and bool((want[pays] > 0).all())
    big = torch.iinfo(torch.int32).max
    f = torch.where(field < 0, torch.full_like(field, big), field).long()
    dx = torch.tensor([1, 0, -1, 0], device=dev)
    dy = torch.tensor([0, 1, 0, -1], device=dev)
    b = torch.arange(B, device=dev)
    goal = torch.from_numpy(G.classify(env.grid.grid.cpu().numpy(), *G.kinds_of(env))[1]).to(dev)
    done_at = torch.full((B,), -1, dtype=torch.long, device=dev)
    got = torch.zeros(B, dtype=torch.float64, device=dev)
    gen = torch.Generator(dev).manual_seed(11)
    for t in range(1, M - warm + 1):
        pos, d = env.agent_pos[:, 0], env.agent_dir[:, 0]
        x, y = pos[:, 0], pos[:, 1]
        fx, fy = (x + dx[d]).clamp(0, W - 1), (y + dy[d]).clamp(0, H - 1)
        v_fwd = torch.where(goal[b, fx, fy], torch.zeros_like(x), f[b, fx, fy, d])
        vals = torch.stack([f[b, x, y, (d + 3) & 3], f[b, x, y, (d + 1) & 3], v_fwd], 1)
        here = f[b, x, y, d]
        act = torch.where(here >= big, torch.randint(0, 3, (B,), device=dev, generator=gen), vals.argmin(1))
        _, rew, done, _ = env.step(act.unsqueeze(1))
        got += torch.where(over, torch.zeros_like(got), rew[:, 0].double())      # an env that is done pays nothing that counts
        newly = env.agent_done[:, 0] & (done_at < 0) & ~over
        done_at = torch.where(newly, torch.full_like(done_at, t), done_at)
        over = over | done
    env.check_errors()
    assert bool(over.all())
    assert torch.equal(done_at[pays], d0[pays])
    assert float((got[pays] - want[pays]).abs().max()) <= REW_TOL
    assert bool((done_at[~pays] < 0).all()) and bool((got[~pays] == 0).all())


# ---- the running use: goal_distance(env_mask=info["reset"]) under auto-reset (examples/level_regret.py) ------------------------
def _reference_rows(env, m):
    """(dist, field) of goal_ref for the envs of the bool array `m`, from the state as it is on the device now"""
    free, goal = G.classify(env.grid.grid.cpu().numpy()[m], *G.kinds_of(env))
    field = G.field_levels(free, goal)
    dist = G.agents_from_field(field, env.agent_pos.cpu().numpy()[m], env.agent_dir.cpu().numpy()[m], env.agent_flags.cpu().numpy()[m])
    return dist, field


@pytest.mark.parametrize("auto_reset,episode_info", [(True, False), ("next_step", True)])
def test_masked_by_the_steps_own_reset_mask_under_auto_reset(auto_reset, episode_info):
    """MarlGrid-3AgentCluttered15x15-v0, 259 envs (a 4-wave workgroup of the register kernel and a ragged tail), max_steps=25, 150
    steps of left / right / forward (nothing is toggled: an episode's grid is static).  Every step
    `goal_distance(env_mask=..., field=True)` with the mask exactly as step() returned it — info["reset"] where there is episode
    info, `done` under same-step reset, where the step that ends an episode is the one that resets it — against a host mirror:
    the reset envs hold the reference of their new grid, every other env still holds its episode's first analysis.  And a
    theorem, not a measurement: in ghost mode on a static grid no policy beats a shortest path, so every completed episode's
    return per agent is at most optimal_return taken at that episode's start (+ REW_TOL), and 0 where the start distance was
    -1 — which a distance that is too LARGE fails.  Required of the run: steps that select no env, steps that select one, a
    step that selects more than a workgroup's four, and at least 5 episodes started in every env."""
    import torch
    from marlgrid_amd.envs import make
    B, M, steps = 259, 25, 150
    env = make(S15, batch_size=B, seeds=1337 + np.arange(B), max_steps=M, auto_reset=auto_reset, episode_info=episode_info,
               place_obs=False)
    assert env.ghost_mode
    env.reset()
    n, dev = env.num_agents, env.device
    # Three random walkers do not all reach the goal within 25 steps: left alone, every env is truncated at the same step and
    # every mask is all or nothing.  Envs 1 .. 11 therefore begin their first episode at step_count 2, 4, .. 22 — they are
    # truncated alone, 25 (26) steps apart from then on; optimal_return reads step_count itself, so the bound stands.
    env.step_count[:12] = torch.arange(0, 24, 2, dtype=env.step_count.dtype, device=dev)
    dist, field = env.goal_distance(field=True)
    every = np.ones(B, bool)
    m_dist, m_field = _reference_rows(env, every)
    assert np.array_equal(dist.cpu().numpy(), m_dist) and np.array_equal(field.cpu().numpy(), m_field)
    best = env.optimal_return(dist).cpu().numpy().copy()
    start_d = m_dist.copy()
    sc = env.step_count.cpu().numpy().astype(np.int64)[:, None]      # the staggered envs' bound: optimal_return reads step_count
    assert sc[:12, 0].tolist() == list(range(0, 24, 2)) and (sc[12:] == 0).all()
    formula = np.where((m_dist < 0) | (sc + m_dist > M), 0.0, 1.0 - 0.9 * (sc + m_dist) / float(M))
    fresh = np.where(m_dist < 0, 0.0, 1.0 - 0.9 * m_dist / float(M))        # ... what the same distance is worth from step 0
    late = np.zeros((B, n), bool)
    late[1:12] = m_dist[1:12] > 0
    assert np.abs(best - formula).max() <= 1e-12 and late.any() and (best[late] < fresh[late]).all()
    ret = np.zeros((B, n))
    starts = np.ones(B, np.int64)
    selected, episodes, paid = [], 0, 0
    rng = np.random.RandomState(3)
    for t in range(steps):
        _, rew, done, info = env.step(torch.from_numpy(rng.randint(0, 3, size=(B, n))).to(dev))
        mask = info["reset"] if episode_info else done
        dist, field = env.goal_distance(env_mask=mask, field=True)
        opt = env.optimal_return(dist).cpu().numpy()
        m, fin = mask.cpu().numpy().astype(bool), done.cpu().numpy().astype(bool)
        ret += rew.cpu().numpy().astype(np.float64)
        returns = info["episode_return"].cpu().numpy() if episode_info else ret
        if episode_info:
            assert np.abs(returns[fin] - ret[fin]).max(initial=0.0) <= REW_TOL      # (the two ways of summing agree)
        assert (returns[fin] <= best[fin] + REW_TOL).all(), t
        assert (returns[fin][start_d[fin] < 0] == 0).all(), t
        episodes += int(fin.sum())
        paid += int((returns[fin] > 0).sum())
        ret[fin] = 0
        if m.any():
            m_dist[m], m_field[m] = _reference_rows(env, m)
            best[m], start_d[m] = opt[m], m_dist[m]
            assert (env.step_count.cpu().numpy()[m] == 0).all()
        assert np.array_equal(dist.cpu().numpy(), m_dist) and np.array_equal(field.cpu().numpy(), m_field), t
        selected.append(int(m.sum()))
        starts += m
    env.check_errors()
    assert 0 in selected and 1 in selected and max(selected) > 4 and starts.min() >= 5
    assert episodes >= 5 * B and paid > 0       # (some agents did reach a goal: the bound was not held by zeros alone)
