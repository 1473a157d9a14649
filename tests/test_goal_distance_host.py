"""goal_distance without a GPU: the bodies of mg_goal_distance (marlgrid_amd/csrc/mg_goal_core.h, the text the two kernels of
mg_goal_dist.hip run) built with g++ (tests/native/mg_goal_dist.cpp) — the general path with 64 lanes and with 1, the
register-resident path where the grid fits a wave — against tests/goal_ref.py: agent_dist and the WHOLE field, on the host
emulation's own state arrays, on grids made by hand and on the serpentine mazes."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
NATIVE = os.path.join(HERE, "native")
if NATIVE not in sys.path:
    sys.path.insert(0, NATIVE)

import goal_ref as G  # noqa: E402
from marlgrid_amd import _native as N  # noqa: E402

IN_CELL = N.AF_ACTIVE | N.AF_PLACED
SCENARIOS = [("MarlGrid-3AgentCluttered15x15-v0", 512, 0), ("MarlGrid-3AgentCluttered15x15-v0", 512, 30),
             ("MarlGrid-3AgentCluttered11x11-v0", 512, 0), ("MarlGrid-3AgentCluttered11x11-v0", 512, 30),
             ("Custom-8AgentCluttered30x30", 64, 0), ("Test-4AgentEmpty5x5-crowded", 64, 0), ("Test-4AgentEmpty5x5-crowded", 64, 30)]


def _paths(cfg):
    out = [("general", 64), ("general", 1)]
    if 4 * cfg.W <= 64 and cfg.H <= 64:
        out.append(("reg", 64))
    return out


def _check_all(cfg, state, want_dist, want_field, mask=None, light=False):
    import hostemu_goal as HG
    if light:       # (the largest maze: 32 509 levels of 4 080 words a run — labels and the whole field, once at 64 lanes and once at
        for lanes in (64, 1):       # 1; the run without a field, and the sealed corridor, are the smaller mazes': 67 x 131 crosses words too)
            dist, fld = HG.run(cfg, state, "general", lanes)
            assert np.array_equal(dist, want_dist) and np.array_equal(fld, want_field), lanes
        return
    for path, lanes in _paths(cfg):
        dist, fld = HG.run(cfg, state, path, lanes, mask=mask)
        sel = slice(None) if mask is None else np.asarray(mask, bool)
        assert np.array_equal(dist[sel], want_dist[sel]), (path, lanes)
        assert np.array_equal(fld[sel], want_field[sel]), (path, lanes, np.argwhere(fld[sel] != want_field[sel])[:5])
        if mask is not None:
            assert (dist[~sel] == -7).all() and (fld[~sel] == -7).all(), (path, lanes)
        # without a field an env stops as soon as its agents are labelled: the same labels
        dist2, _ = HG.run(cfg, state, path, lanes, mask=mask, field=False)
        assert np.array_equal(dist2, dist), (path, lanes)


@pytest.fixture(scope="module")
def emus():
    """one emulated batch per (name, B, steps), stepped once: (emu, reference dist, reference field, on-goal count)"""
    import hostemu
    cache = {}

    def get(name, B, steps):
        key = (name, B, steps)
        if key not in cache:
            emu = hostemu.HostEmu(name, B, 1337 + np.arange(B))
            emu.reset()
            rng = np.random.RandomState(5)
            for _ in range(steps):
                emu.step(rng.randint(0, 7, size=(B, emu.n)))
            W, H = emu.env.width, emu.env.height
            grid = emu.grid[:, :W * H].reshape(B, W, H)
            free, goal = G.classify(grid, *G.kinds_of(emu.env))
            field = G.field_levels(free, goal)
            pos, dirs, flags = G.unpack_records(emu.rec)
            dist = G.agents_from_field(field, pos, dirs, flags)
            b = np.arange(B)[:, None]
            in_cell = ((flags & N.AF_ACTIVE) != 0) & ((flags & N.AF_EVICTED) == 0)
            on_goal = in_cell & goal[b, pos[..., 0], pos[..., 1]]
            cache[key] = (emu, dist, field, in_cell, on_goal)
        return cache[key]
    return get


@pytest.mark.parametrize("name,B,steps", SCENARIOS)
def test_scenarios_match_the_reference(emus, name, B, steps):
    emu, dist, field, in_cell, on_goal = emus(name, B, steps)
    if steps:
        assert (~in_cell).any() or "Empty" in name       # (done agents give -1)
        assert (dist[~in_cell] == -1).all()
    _check_all(emu._cfg(), emu.state, dist, field)


def test_the_15x15_input_holds_every_kind_of_pair(emus):
    """seeds 1337 + b, after the reset: pairs with no path, agents standing on a goal, and reachable ones"""
    _, dist, _, in_cell, on_goal = emus("MarlGrid-3AgentCluttered15x15-v0", 512, 0)
    assert in_cell.all()
    assert (dist < 0).sum() >= 1 and on_goal.sum() >= 1 and (dist > 0).sum() >= 1
    assert ((dist < 0).sum(), on_goal.sum()) == (32, 13)


def test_env_mask_leaves_unselected_rows_alone(emus):
    emu, dist, field, _, _ = emus("MarlGrid-3AgentCluttered11x11-v0", 512, 0)
    mask = (np.arange(512) % 3 == 1)
    _check_all(emu._cfg(), emu.state, dist, field, mask=mask)


def _walled(W, H, B=1):
    import hostemu_goal as HG
    g = np.zeros((B, W, H), np.uint8)
    g[:, 0, :] = g[:, -1, :] = g[:, :, 0] = g[:, :, -1] = HG.RawCase.WALL
    return g


def _raw(grid, agents):
    """-> (case, reference dist, reference field) with every env's field by the reverse queue search and every agent by the
    forward search of the definition"""
    import hostemu_goal as HG
    case = HG.RawCase(grid, agents)
    free, goal = G.classify(np.asarray(grid), *case.kinds())
    field = np.stack([G.field_queue(free[b], goal[b]) for b in range(free.shape[0])])
    pos, dirs, flags = G.unpack_records(case.rec)
    dist = G.agents_from_field(field, pos, dirs, flags)
    for b in range(dist.shape[0]):
        for k in range(dist.shape[1]):
            if flags[b, k] & N.AF_ACTIVE and not flags[b, k] & N.AF_EVICTED:
                assert dist[b, k] == G.agent_bfs(free[b], goal[b], int(pos[b, k, 0]), int(pos[b, k, 1]), int(dirs[b, k]))
    return case, dist, field


def test_hand_cases():
    """a walled 5 x 5 grid with the goal at (3, 2)"""
    import hostemu_goal as HG
    R = HG.RawCase
    g = _walled(5, 5, 2)
    g[:, 3, 2] = R.GOAL
    g[1, 2, 2] = g[1, 3, 1] = g[1, 3, 3] = R.WALL        # env 1: the goal's three other neighbours walled
    agents = [[(2, 2, 0, IN_CELL), (2, 2, 1, IN_CELL), (2, 2, 2, IN_CELL), (3, 2, 0, IN_CELL), (1, 1, 0, 0),
               (1, 1, 0, IN_CELL | N.AF_EVICTED)],
              [(3, 2, 0, IN_CELL), (3, 2, 3, IN_CELL), (1, 1, 0, IN_CELL), (1, 1, 0, N.AF_DONE), (1, 3, 2, IN_CELL),
               (1, 2, 1, IN_CELL)]]
    case, dist, field = _raw(g, agents)
    assert dist[0].tolist() == [1, 2, 3, 5, -1, -1]
    assert dist[1].tolist() == [-1, -1, -1, -1, -1, -1]
    _check_all(case.cfg, case.state, dist, field)


@pytest.mark.parametrize("W,H", sorted(G.MAZES))
def test_mazes(W, H):
    import hostemu_goal as HG
    wall, goal = G.serpentine(W, H)
    g = np.zeros((2, W, H), np.uint8)
    g[:, wall] = HG.RawCase.WALL
    g[:, goal[0], goal[1]] = HG.RawCase.GOAL
    big = W * H > 10000
    if big:
        g[1, goal[0], goal[1]] = 0                        # env 1 of the largest maze: no goal, nothing to search
    elif H > 5:
        g[1, 1, H - 2] = HG.RawCase.WALL                  # env 1: the first corridor sealed, nothing reachable from the start
    case, dist, field = _raw(g, [[(1, 1, 0, IN_CELL)], [(1, 1, 0, IN_CELL)]])
    assert dist[0, 0] == G.MAZES[(W, H)]
    assert dist[1, 0] == (-1 if big or H > 5 else G.MAZES[(W, H)])
    _check_all(case.cfg, case.state, dist, field, light=big)


def test_other_grids():
    import hostemu_goal as HG
    R = HG.RawCase
    g = _walled(7, 7, 6)
    a = [[(1, 1, 0, IN_CELL), (5, 3, 2, IN_CELL)] for _ in range(6)]
    g[0, 5, 5] = g[0, 1, 5] = R.GOAL                               # two goals
    # env 1: no goal at all
    g[2, 5, 5] = R.GOAL                                            # a goal behind lava
    g[2, 4, 1:6] = R.LAVA
    g[3, 5, 5] = R.GOAL                                            # ... behind a closed door
    g[3, 4, 1:6] = R.WALL
    g[3, 4, 3] = R.DOOR_CLOSED
    g[4] = g[3]                                                    # ... and behind an open one
    g[4, 4, 3] = R.DOOR_OPEN
    g[5, 3, 3] = R.GOAL                                            # a border cell emptied, an agent facing out through it
    g[5, 6, 3] = 0
    a[5] = [(5, 3, 0, IN_CELL), (6, 3, 0, IN_CELL)]
    a[3][1] = a[4][1] = (3, 3, 0, IN_CELL)
    case, dist, field = _raw(g, a)
    assert (dist[0] > 0).all() and (dist[1] == -1).all() and (field[1] == -1).all()
    assert dist[2].tolist() == [-1, 3] and dist[3].tolist() == [-1, -1]
    assert (dist[4] > 0).all()
    assert dist[5].tolist() == [4, 5]       # turn, turn, forward, forward; from the border cell one forward more
    _check_all(case.cfg, case.state, dist, field)


def test_scratch_fits_lds_at_the_largest_grid():
    import hostemu_goal as HG
    assert HG.lib().gd_scratch_bytes(255, 255) == 14 * 8 * 255 * 4 + 128 <= 160 * 1024


# ---- the edge shapes of both kernels (tests/goal_cases.py; the device runs the same in tests/test_hip_goal_distance.py) ------
def _edge_shapes():
    import goal_cases
    return goal_cases.REG_SHAPES + goal_cases.LDS_SHAPES


@pytest.mark.parametrize("W,H", _edge_shapes())
def test_edge_shapes(W, H):
    """lane 63 owning a plane, bit 63, W != H, one column, one row, more agents than plane lanes; H on both sides of every
    word boundary; the two shapes around 64 KiB of scratch.  The coverage conditions are asserted on the reference's field
    (goal_cases.edge): states with a distance in the first and last row and column and in every row beside a word boundary."""
    import ctypes as C
    import goal_cases
    import hostemu_goal as HG
    case, dist, field = goal_cases.edge(W, H)
    fits = goal_cases.reg_fits(W, H)
    assert fits == ((W, H) in goal_cases.REG_SHAPES)
    assert HG.lib().gd_scratch_bytes(W, H) == goal_cases.scratch_bytes(W, H)
    assert [p for p, _ in _paths(case.cfg)] == ["general", "general"] + ["reg"] * fits
    _check_all(case.cfg, case.state, dist, field)
    if not fits:        # the register kernel is not launched for the shape
        d = np.full(dist.shape, -7, np.int32)
        assert HG.lib().gd_reg(C.byref(case.cfg), C.byref(case.state), None, d.ctypes.data, None) == -1 and (d == -7).all()


def test_edge_shapes_sit_where_they_are_meant_to():
    import goal_cases
    assert goal_cases.scratch_bytes(146, 193) == 64 * 1024 and goal_cases.scratch_bytes(147, 193) == 65984
    assert len(_edge_shapes()) == 22 and len(set(_edge_shapes())) == 22
    for W, H in goal_cases.REG_SHAPES:
        n = goal_cases.edge(W, H)[0].cfg.n_agents
        assert n == (32 if W <= 3 else 6) and (n > 4 * W) == (W <= 3)


# ---- following the field from the middle of an episode and across truncation ---------------------------------------------------
FOLLOW = [(14, 0), (20, 6), (100, 30)]          # (max_steps, warm-up steps); the device runs the same cases
REW_TOL = 1e-6


@pytest.mark.parametrize("M,warm", FOLLOW)
def test_following_the_field_pays_what_optimal_return_says(M, warm):
    """MarlGrid-1AgentCluttered15x15-v0, 512 envs, `warm` steps of left / right / forward, then every step the action whose
    successor has the smaller field value.  optimal_return's formula, restated here, is held to the rewards the step body
    pays: where d >= 0 and step_count + d <= max_steps the agent is done at exactly step d with exactly that return; everywhere
    else the formula says 0 and nothing is earned — at step_count + d == max_steps + 1 the episode is truncated one step
    before the goal."""
    import hostemu
    import hostemu_goal as HG
    B = 512
    emu = hostemu.HostEmu("MarlGrid-1AgentCluttered15x15-v0", B, 1337 + np.arange(B), max_steps=M)
    emu.reset()
    rng = np.random.RandomState(9)
    for _ in range(warm):
        emu.step(rng.randint(0, 3, size=(B, 1)))
    W, H = emu.env.width, emu.env.height
    grid = emu.grid[:, :W * H].reshape(B, W, H).copy()
    dist, field = HG.run(emu._cfg(), emu.state, "reg")
    goal = G.classify(grid, *G.kinds_of(emu.env))[1]
    sc = emu.step_count.astype(np.int64).copy()
    d0 = dist[:, 0].astype(np.int64)
    running = ~emu.done.astype(bool)
    assert (sc[running] == warm).all() and running.any()
    assert (dist[~running, 0] == -1).all()      # (an env that ended in the warm-up: its agent is done, in no cell)
    t_goal = sc + d0
    pays = (d0 >= 0) & (t_goal <= M)
    want = np.where(pays, 1.0 * (1.0 - 0.9 * (t_goal / float(M))), 0.0)
    assert emu.env.reward_decay and emu.env.max_steps == M
    if M < 100:     # the truncation rule is met on both sides
        assert (running & (d0 >= 0) & (t_goal == M)).any() and (running & (d0 >= 0) & (t_goal == M + 1)).any()
    assert pays.any() and (d0 < 0).any()
    big = np.iinfo(np.int32).max
    f = np.where(field < 0, big, field).astype(np.int64)
    b = np.arange(B)
    dx, dy = np.array([1, 0, -1, 0]), np.array([0, 1, 0, -1])
    done_at = np.full(B, -1, np.int64)
    got = np.zeros(B)
    over = ~running
    for t in range(1, M - warm + 1):
        pos, d, _ = G.unpack_records(emu.rec)
        x, y, d = pos[:, 0, 0], pos[:, 0, 1], d[:, 0]
        fx, fy = np.clip(x + dx[d], 0, W - 1), np.clip(y + dy[d], 0, H - 1)
        v_fwd = np.where(goal[b, fx, fy], 0, f[b, fx, fy, d])
        vals = np.stack([f[b, x, y, (d + 3) & 3], f[b, x, y, (d + 1) & 3], v_fwd], 1)
        here = f[b, x, y, d]
        act = np.where(here >= big, rng.randint(0, 3, size=B), vals.argmin(1))
        rew, done = emu.step(act[:, None])
        got += np.where(over, 0.0, rew[:, 0].astype(np.float64))       # an env that is done pays nothing that counts
        _, _, fl = G.unpack_records(emu.rec)
        newly = ((fl[:, 0] & N.AF_DONE) != 0) & (done_at < 0) & ~over
        done_at = np.where(newly, t, done_at)
        over |= done
    assert over.all()
    assert np.array_equal(done_at[pays], d0[pays])
    assert np.abs(got[pays] - want[pays]).max() <= REW_TOL
    assert (done_at[~pays] < 0).all() and (got[~pays] == 0).all() and (want[~pays] == 0).all()
