"""tests/goal_ref.py against itself: the forward queue search per agent (the definition), the reverse queue search and the
batched level-by-level numpy field give the same numbers on the inputs the goal-distance tests use."""
import numpy as np
import pytest

import goal_ref as G
from marlgrid_amd import _native as N


def _random_batch(B, W, H, seed):
    rng = np.random.RandomState(seed)
    r = rng.randint(0, 20, size=(B, W, H))
    free = r >= 5
    goal = np.zeros_like(free)
    for b in range(B):
        for _ in range(rng.randint(0, 3)):
            x, y = rng.randint(W), rng.randint(H)
            goal[b, x, y], free[b, x, y] = True, False
    return free, goal


@pytest.mark.parametrize("W,H", [(1, 1), (3, 9), (9, 3), (15, 15), (11, 11), (7, 70)])
def test_three_forms_agree_on_random_grids(W, H):
    free, goal = _random_batch(24, W, H, W * 100 + H)
    levels = G.field_levels(free, goal)
    rng = np.random.RandomState(1)
    for b in range(free.shape[0]):
        assert np.array_equal(G.field_queue(free[b], goal[b]), levels[b])
        for _ in range(12):
            x, y, d = rng.randint(W), rng.randint(H), rng.randint(4)
            assert G.agent_bfs(free[b], goal[b], x, y, d) == levels[b, x, y, d]


@pytest.mark.parametrize("name,B", [("MarlGrid-3AgentCluttered15x15-v0", 512), ("MarlGrid-3AgentCluttered11x11-v0", 512)])
def test_forms_agree_on_the_oracle_envs(name, B):
    """every agent of the first 512 envs (seeds 1337 + b, after the user reset()) on the host emulation's grids — bit-exact
    with the oracle's (tests/test_core_hostemu.py) —, the agents standing on a goal included"""
    import os
    import sys
    native = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")
    if native not in sys.path:
        sys.path.insert(0, native)
    import hostemu
    emu = hostemu.HostEmu(name, B, 1337 + np.arange(B))
    emu.reset()
    W, H = emu.env.width, emu.env.height
    free, goal = G.classify(emu.grid[:, :W * H].reshape(B, W, H), *G.kinds_of(emu.env))
    pos, dirs, flags = G.unpack_records(emu.rec)
    assert ((flags & N.AF_ACTIVE) != 0).all()
    levels = G.field_levels(free, goal)
    n_unreach = n_on_goal = 0
    for b in range(B):
        for k in range(emu.n):
            x, y, d = int(pos[b, k, 0]), int(pos[b, k, 1]), int(dirs[b, k])
            v = G.agent_bfs(free[b], goal[b], x, y, d)
            assert v == levels[b, x, y, d]
            n_unreach += v < 0
            n_on_goal += bool(goal[b, x, y])
    assert n_unreach == (32 if "15x15" in name else 64)
    assert n_on_goal >= 1


def test_maze_table():
    for (W, H), want in G.MAZES.items():
        wall, g = G.serpentine(W, H)
        goal = np.zeros_like(wall)
        goal[g] = True
        assert G.agent_bfs(~wall & ~goal, goal, 1, 1, 0) == want
    wall, g = G.serpentine(67, 131)
    goal = np.zeros_like(wall)
    goal[g] = True
    f = G.field_queue(~wall & ~goal, goal)
    assert f[1, 1, 0] == 4353 and f.max() == 4354     # (the start facing -y: two turns instead of one before the first corridor)
    assert np.array_equal(f, G.field_levels((~wall & ~goal)[None], goal[None])[0])
