"""TEST INFRASTRUCTURE — the inputs tests/test_solve_distance_host.py (the host twin) and tests/test_hip_solve_distance.py (the
device) share: the scenario batches, the grids made by hand and the edge shapes, each with what tests/solve_ref.py says about it.
A hand case is (SolveCase, (max_doors, max_items), reference (dist, action, exact)); where the reference calls the case exact,
every agent's number is also held to the definition (`full_bfs`) here, once."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "native"))

import solve_ref as S  # noqa: E402
from marlgrid_amd import _native as N  # noqa: E402

IN_CELL = N.AF_ACTIVE | N.AF_PLACED
DK8, DK6, CDK8 = "MarlGrid-2AgentDoorKey8x8-v0", "MarlGrid-2AgentDoorKey6x6-v0", "MarlGrid-2AgentColoredDoorKey8x8-v0"
S15 = "MarlGrid-3AgentCluttered15x15-v0"
SOLO8 = "MarlGrid-1AgentDoorKey8x8-v0"
SCENARIOS = [(name, 512, steps) for name in (DK8, DK6, CDK8) for steps in (0, 30)] + [(S15, 512, 0)]
FOLLOW = [14, 40, 100]      # max_steps of the follow-the-policy runs
REW_TOL = 1e-6              # the project's reward tolerance


def reference(grid, kinds, rec, caps=(2, 2)):
    x, y, d, in_cell, carry = S.unpack(rec)
    return S.layered(grid, kinds, x, y, d, in_cell, carry, *caps)


def _case(grid, agents, caps=(2, 2), check_definition=True):
    import hostemu_solve as HS
    case = HS.SolveCase(np.asarray(grid, np.uint8)[None], [agents])
    kinds = HS.SolveCase.kinds()
    want = reference(case.grid3, kinds, case.rec, caps)
    if check_definition and want[2].all():
        x, y, d, in_cell, carry = S.unpack(case.rec)
        for k in range(x.shape[1]):
            if in_cell[0, k]:
                full = S.full_bfs(case.grid3[0], kinds, int(x[0, k]), int(y[0, k]), int(d[0, k]), int(carry[0, k]))
                assert full == want[0][0, k], (k, full, want[0][0, k])
    return case, caps, want


def walled(W, H):
    g = np.zeros((W, H), np.uint8)
    g[0, :] = g[-1, :] = g[:, 0] = g[:, -1] = 1
    return g


def _a(x, y, d, carry=0, flags=IN_CELL):
    return (x, y, d, flags, carry)


def hand_cases():
    """name -> (case, caps, reference)"""
    import hostemu_solve as HS
    K = HS.SolveCase
    out = {}
    # the key lies behind the closed door A, the locked door is in the start room: A is passed twice and paid once
    g = walled(7, 7)
    g[3, 1:6] = K.WALL
    g[3, 1] = K.SHUT_A
    g[5, 5] = K.KEY_B
    g[1:3, 4] = K.WALL
    g[1, 4] = K.LOCKED_B
    g[1, 5] = K.GOAL
    out["door_passed_twice"] = _case(g, [_a(2, 2, 0), _a(1, 1, 3), _a(4, 4, 2)])
    # two locked doors of two colours in series: one object at most is ever picked up
    g = walled(9, 5)
    g[4, 1:4] = g[6, 1:4] = K.WALL
    g[4, 2], g[6, 2], g[7, 2] = K.LOCKED_A, K.LOCKED_B, K.GOAL
    g[1, 1], g[1, 3] = K.KEY_A, K.KEY_B
    out["two_locked_in_series"] = _case(g, [_a(2, 2, 0), _a(5, 2, 0), _a(5, 2, 0, K.KEY_B)])
    # a ball plugs a one-cell corridor
    g = walled(7, 5)
    g[3, 1:4] = K.WALL
    g[3, 2], g[5, 2] = K.BALL, K.GOAL
    out["ball_plugs_corridor"] = _case(g, [_a(1, 2, 0), _a(2, 2, 0, K.KEY_A)])
    # the right key in hand, the wrong key, a ball (none of the two can pick the key up), empty hands; a box on the floor
    g = walled(7, 7)
    g[3, 1:6] = K.WALL
    g[3, 3], g[5, 3], g[1, 5], g[2, 5] = K.LOCKED_A, K.GOAL, K.KEY_A, K.BOX
    out["carries"] = _case(g, [_a(2, 3, 0, K.KEY_A), _a(2, 3, 0, K.KEY_B), _a(2, 3, 0, K.BALL), _a(2, 3, 0), _a(1, 1, 1, K.BOX)])
    # doors whose opened id is not a free cell
    g = walled(7, 7)
    g[3, 1:6] = K.WALL
    g[3, 2], g[3, 4], g[5, 3] = K.STUCK, K.SHUT_TO_LAVA, K.GOAL
    out["doors_that_do_not_open"] = _case(g, [_a(2, 2, 0), _a(2, 4, 0)])
    # an open door is a plain free cell; an agent in a shut door's cell; done, evicted and unspawned agents
    g = walled(7, 7)
    g[3, 1:6] = K.WALL
    g[3, 3], g[3, 1], g[5, 3] = K.OPEN_A, K.SHUT_A, K.GOAL
    out["open_door_and_agents_in_no_cell"] = _case(g, [_a(2, 3, 0), _a(3, 1, 0), _a(1, 1, 0, flags=0), _a(1, 1, 0, flags=N.AF_DONE),
                                                       _a(1, 1, 0, flags=IN_CELL | N.AF_EVICTED), _a(3, 3, 2)])
    # the goal is reachable without the door, and sooner through it
    g = walled(7, 7)
    g[3, 1:5] = K.WALL
    g[3, 1], g[4, 1] = K.SHUT_A, K.GOAL
    out["door_is_a_shortcut"] = _case(g, [_a(2, 1, 0), _a(1, 5, 3)])
    # more doors than the cap: the first in grid order is tracked, the near one blocks
    g = walled(7, 7)
    g[3, 1:6] = K.WALL
    g[3, 1], g[3, 5], g[4, 5] = K.SHUT_A, K.SHUT_A, K.GOAL
    out["caps_exceeded"] = _case(g, [_a(2, 5, 0), _a(2, 1, 0)], caps=(1, 1))
    out["caps_exceeded_uncapped"] = _case(g, [_a(2, 5, 0), _a(2, 1, 0)])
    # more items than the cap: the key that matters is the third item
    g = walled(7, 7)
    g[3, 1:6] = K.WALL
    g[3, 3], g[5, 3], g[1, 1], g[1, 2], g[2, 5] = K.LOCKED_B, K.GOAL, K.BALL, K.KEY_A, K.KEY_B
    out["items_beyond_the_cap"] = _case(g, [_a(2, 3, 0)])
    out["items_within_the_cap"] = _case(g, [_a(2, 3, 0)], caps=(2, 3))
    return out


def _boundary(H, W=5):
    """the last rows of a H-row grid without a border: a ball, two doors and a key around row H - 1 — at H = 65 on both sides
    of the word boundary"""
    import hostemu_solve as HS
    K = HS.SolveCase
    yb = H - 1
    g = np.full((W, H), K.WALL, np.uint8)
    g[1, max(0, yb - 8):] = 0
    g[1, yb - 1] = K.BALL
    g[2, yb], g[3, yb], g[3, yb - 1], g[3, yb - 2], g[4, yb] = K.SHUT_A, 0, K.SHUT_B, K.GOAL, K.KEY_A
    return _case(g, [_a(1, yb - 4, 1), _a(3, yb, 0), _a(1, yb, 0, K.KEY_B)], check_definition=H <= 70)


def _corridor(W, H, n=3):
    """a walled W x H room cut by a wall with a closed door in it, the goal in the far corner; n agents on the near side"""
    import hostemu_solve as HS
    K = HS.SolveCase
    g = walled(W, H)
    if W >= H:
        cut = W // 2
        g[cut, 1:H - 1] = K.WALL
        g[cut, 1 + (H - 2) // 2] = K.SHUT_A
        cells = [(x, y) for x in range(1, cut) for y in range(1, H - 1)]
    else:
        cut = H // 2
        g[1:W - 1, cut] = K.WALL
        g[1 + (W - 2) // 2, cut] = K.SHUT_A
        cells = [(x, y) for y in range(1, cut) for x in range(1, W - 1)]
    g[W - 2, H - 2] = K.GOAL
    agents = [_a(*cells[(5 * k) % len(cells)], k % 4) for k in range(n)]
    return _case(g, agents, check_definition=n <= 6)


EDGE_SHAPES = ["one_column", "one_row", "lanes_64", "H64", "H65", "H129", "more_agents_than_planes"]


def edge(name):
    if name == "one_column":
        return _corridor(3, 9)
    if name == "one_row":
        return _corridor(9, 3)
    if name == "lanes_64":
        return _corridor(16, 7)             # 4 W = 64
    if name == "more_agents_than_planes":
        return _corridor(3, 11, n=32)       # 32 agents, 12 planes
    return _boundary(int(name[1:]))


# ---- the scenario batches -----------------------------------------------------------------------------------------------------
_emus = {}


def emu_batch(name, B, steps):
    """the host emulation of `name` with seeds 1337 + b, reset and stepped `steps` times at random: (emu, grid (B, W, H), kinds,
    reference (dist, action, exact)), made once"""
    key = (name, B, steps)
    if key not in _emus:
        import hostemu
        emu = hostemu.HostEmu(name, B, 1337 + np.arange(B))
        emu.reset()
        rng = np.random.RandomState(5)
        for _ in range(steps):
            emu.step(rng.randint(0, 7, size=(B, emu.n)))
        W, H = emu.env.width, emu.env.height
        grid = emu.grid[:, :W * H].reshape(B, W, H).copy()
        kinds = S.Kinds.of_env(emu.env)
        _emus[key] = (emu, grid, kinds, reference(grid, kinds, emu.rec))
    return _emus[key]


def half_open_and_carried(grid, kinds, rec):
    """(envs with an unlocked but shut door, agents carrying a key)"""
    shut = np.array([kinds.is_shut_door(i) and not kinds.flags[i] & N.OF_DOOR_LOCKED for i in range(kinds.n)])
    carry = S.unpack(rec)[4]
    keys = np.array([kinds.key_colour(i) >= 0 for i in range(kinds.n)])
    return int(shut[grid].any(axis=(1, 2)).sum()), int(keys[carry].sum())


def follow_expectation(d0, step_count, M):
    """optimal_return's formula, restated: (pays, the return) for distances d0 at step_count under max_steps M, R = 1 with decay"""
    t = step_count.astype(np.int64) + d0.astype(np.int64)
    pays = (d0 >= 0) & (t <= M)
    return pays, np.where(pays, 1.0 - 0.9 * (t / float(M)), 0.0)
