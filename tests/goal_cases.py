"""TEST INFRASTRUCTURE — the edge shapes of goal_distance's two kernels, shared by the host test (tests/test_goal_distance_host.py)
and the device test (tests/test_hip_goal_distance.py): the shapes, the generator of their batches, the reference and the
coverage the reference's own field has to show, so that a green run cannot mean "nothing was reachable".

  REG_SHAPES   fit a wave's registers (4 W <= 64, H <= 64): lane 63 owning a plane (W = 16), bit 63 (H = 64), W != H, one
               column, one row, and W <= 3 with 32 agents — more agents than lanes that own a plane
  LDS_SHAPES   do not: one past each limit of the register kernel, H on both sides of every word boundary (64 / 65, 128 / 129,
               192 / 193), one column and one row of 255, and the two shapes around 64 KiB of scratch: 146 x 193 takes exactly
               65 536 bytes, 147 x 193 takes 65 984
"""
import numpy as np

import goal_ref as G
import hostemu_goal
from marlgrid_amd import _native as N

IN_CELL = N.AF_ACTIVE | N.AF_PLACED
REG_SHAPES = [(16, 64), (16, 63), (15, 64), (16, 5), (3, 64), (2, 64), (2, 2), (1, 7), (7, 1), (9, 12), (13, 6)]
LDS_SHAPES = [(17, 5), (17, 64), (5, 65), (4, 128), (3, 129), (2, 192), (2, 193), (1, 255), (255, 1), (146, 193), (147, 193)]
WORD_ROWS = (63, 64, 127, 128, 191, 192)


def reg_fits(W, H):
    return 4 * W <= 64 and H <= 64


def scratch_bytes(W, H):
    """what DESIGN.md §3.3c says the LDS kernel takes"""
    return 14 * 8 * W * ((H + 63) // 64) + 128


def edge_case(W, H, B=6):
    """-> (grid (B, W, H) of RawCase ids, agents (B, n, 4) as (x, y, dir, flags)): mostly empty cells, some walls, lava, floor
    and doors; envs 0 .. 3 with the goal in one corner each, the others with three goals anywhere; agent 0 in the last column
    and row facing out of the grid, agent 1 in the first facing out, agent 2 not active, agent 3 evicted"""
    R = hostemu_goal.RawCase
    rng = np.random.RandomState(1000 * W + H)
    pal = ([0] * 15 + [R.WALL] * 2 + [R.LAVA, R.FLOOR, R.DOOR_OPEN, R.DOOR_CLOSED] if min(W, H) > 4
           else [0] * 60 + [R.WALL, R.LAVA, R.FLOOR, R.DOOR_OPEN])
    g = rng.choice(np.array(pal, np.uint8), size=(B, W, H))
    corners = [(W - 1, H - 1), (0, 0), (W - 1, 0), (0, H - 1)]
    for b in range(B):
        if b < 4:
            g[b][corners[b]] = R.GOAL
        else:
            for _ in range(3):
                g[b, rng.randint(W), rng.randint(H)] = R.GOAL
    n = 32 if W <= 3 else 6          # W <= 3: more agents than lanes that own a plane
    ag = np.stack([rng.randint(W, size=(B, n)), rng.randint(H, size=(B, n)), rng.randint(4, size=(B, n)),
                   np.full((B, n), IN_CELL)], -1)
    ag[:, 0, :3] = [W - 1, H - 1, 1]     # in the last column and row, facing out of the grid
    ag[:, 1, :3] = [0, 0, 3]
    ag[:, 2, 3] = 0                      # not active
    ag[:, 3, 3] = IN_CELL | N.AF_EVICTED
    return g, ag


def reference(case, grid):
    """-> (dist (B, n), field (B, W, H, 4)) by the reverse queue search per env and the field at each agent's state"""
    free, goal = G.classify(np.asarray(grid), *case.kinds())
    field = np.stack([G.field_queue(free[b], goal[b]) for b in range(free.shape[0])])
    return G.agents_from_field(field, *G.unpack_records(case.rec)), field


def assert_coverage(dist, field):
    """on the REFERENCE's numbers: a state with a distance in the first and last row and column and in every row beside a word
    boundary that the shape has, an agent with a distance and one without"""
    B, W, H, _ = field.shape
    for name, part in (("row 0", field[:, :, 0]), ("row H - 1", field[:, :, H - 1]), ("column 0", field[:, 0]),
                       ("column W - 1", field[:, W - 1])):
        assert (part > 0).any(), (W, H, name)
    for y in WORD_ROWS:
        if y < H:
            assert (field[:, :, y] > 0).any(), (W, H, y)
    assert (dist > 0).any() and (dist == -1).any(), (W, H)


_cache = {}


def edge(W, H):
    """(RawCase, reference dist, reference field) of a shape, made once and left alone"""
    if (W, H) not in _cache:
        g, ag = edge_case(W, H)
        case = hostemu_goal.RawCase(g, ag)
        dist, field = reference(case, g)
        assert_coverage(dist, field)
        dist.setflags(write=False)
        field.setflags(write=False)
        _cache[(W, H)] = (case, dist, field)
    return _cache[(W, H)]
