"""goal_distance's notion of a cell against the ORACLE (CPU): the verdicts of tests/goal_probe.py — blocked / free / goal, read
from what one `forward` does — taken from the oracle, which is the pin to the reference, and held to the product's flag rule
(tests/goal_ref.py:kinds_of, the text of mg_goal_core.h:goal_cell_kind) on the same scenes and the same seed.

Every probe is the FIRST step of a freshly reset oracle env: agent 0 is put on an in-grid neighbour of the cell, turned to face
it, and steps `forward` while the others act `done`.  (A reused env's step_count runs past max_steps and a goal's decayed
reward goes negative.)  `place_agent_at` refuses neighbours the agent cannot stand on, so a cell without a standable in-grid
neighbour is left out — border walls; the test requires that every object id of the grid is probed in some cell."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(HERE, "native")):
    if p not in sys.path:
        sys.path.insert(0, p)

import goal_probe as P  # noqa: E402
import goal_ref as G  # noqa: E402
from oracle import oracle as O  # noqa: E402
import scenarios  # noqa: E402

REFUSED = "oracle rc=-1"            # OracleEnv.place_agent_at where the agent cannot stand (MGO_ERR_VALUE)
# probes made per scene: the (cell, standable in-grid neighbour) pairs of the grid of seed 1337
PROBES = {"Limit-3Agent100Kinds24x24": 1800, "MarlGrid-3AgentCluttered11x11-v0": 276, "Edge-HumanPlayerConfig": 412,
          "Test-3AgentCluttered12x6-nonsquare": 132, P.NOGHOST: 268}


def _fresh(spec, like, prepare):
    e = O.OracleEnv(spec, P.SEED, _like=like)
    e.reset(observe=False)
    if prepare is not None:
        prepare(e)
    return e


def _oracle_verdicts(spec, prepare=None):
    """-> (base grid (W, H) of object ids, verdict (W, H) with -1 where the cell was left out, other agents' cells, probes)"""
    first = _fresh(spec, None, prepare)
    st0 = first.state()
    W, H, n = first.W, first.H, first.n
    assert st0["step_count"] == 0 and st0["active"][0]
    lo, hi = np.full((W, H), 9), np.full((W, H), -1)
    probes = 0
    for x in range(W):
        for y in range(H):
            for d in range(4):
                nx, ny = x - P.DX[d], y - P.DY[d]
                if not (0 <= nx < W and 0 <= ny < H):
                    continue
                e = _fresh(spec, first, prepare)
                try:
                    e.place_agent_at(0, int(nx), int(ny))
                except ValueError as err:   # not a cell an agent can stand on: try_place's refusal, and nothing else
                    assert str(err) == REFUSED, err
                    continue
                e.set_dir(0, d)
                _, rew, _, _ = e.step([P.FORWARD] + [P.DONE] * (n - 1))
                st = e.state()
                px, py = st["pos"][0]
                moved = (px, py) == (x, y)
                assert moved or (px, py) == (nx, ny)
                v = P.BLOCKED if not moved else (P.FREE if not st["done"][0] else (P.GOAL if rew[0] > 0 else P.BLOCKED))
                lo[x, y], hi[x, y] = min(lo[x, y], v), max(hi[x, y], v)
                probes += 1
    assert np.array_equal(lo[hi >= 0], hi[hi >= 0]), "probes that enter one cell disagree"
    return st0["base"], hi, [tuple(int(v) for v in p) for p in st0["pos"][1:]], probes


def _assert_every_kind_probed(base, verdict):
    probed = verdict >= 0
    ids = set(np.unique(base).tolist())
    assert ids == set(np.unique(base[probed]).tolist())              # every object id of the grid is probed in some cell
    assert set(np.unique(base[~probed]).tolist()) <= set(np.unique(base[probed]).tolist())       # ... the left-out ones too
    return ids


@pytest.mark.parametrize("name", P.SCENES)
def test_oracle_verdicts_are_the_products_rule(name):
    import hostemu
    spec = scenarios.registered(name)
    base, verdict, others, probes = _oracle_verdicts(spec)
    ids = _assert_every_kind_probed(base, verdict)
    probed = verdict >= 0
    # left out (18 of 576 cells of Kinds, 4 of 121 of Cluttered 11 x 11, 10 of 169 of Edge-HumanPlayerConfig): border walls all
    border = np.ones(base.shape, bool)
    border[1:-1, 1:-1] = False
    assert (base[~probed] == spec["wall_obj"]).all() and border[~probed].all()
    assert probes == PROBES[name], probes
    if name == "Limit-3Agent100Kinds24x24":
        assert len(ids) == 102
    # the product's rule on the product's grid of the same seed
    emu = hostemu.HostEmu(name, 1, [P.SEED])
    emu.reset()
    W, H = spec["W"], spec["H"]
    grid = emu.grid[0, :W * H].reshape(W, H)
    free, goal = G.classify(grid, *G.kinds_of(emu.env))
    rule = np.where(goal, P.GOAL, np.where(free, P.FREE, P.BLOCKED))
    assert np.array_equal(grid != 0, base != 0)
    leave = np.zeros((W, H), bool)
    if name == P.NOGHOST:       # other agents block there: those two cells are not compared, every other one is
        assert len(set(others)) == 2
        for x, y in others:
            leave[x, y] = True
        assert all(verdict[x, y] == P.BLOCKED and rule[x, y] == P.FREE for x, y in others)
    sel = probed & ~leave
    assert np.array_equal(verdict[sel], rule[sel]), np.argwhere((verdict != rule) & sel)
    if name == "Edge-HumanPlayerConfig":
        assert (verdict != P.GOAL).all() and (verdict == P.FREE).any()
    else:
        assert (verdict == P.GOAL).any() and (verdict == P.FREE).any() and (verdict == P.BLOCKED).any()


def test_oracle_zoo_of_kinds():
    """tests/scenarios.py:objects_zoo_spec with one object of each id 1 .. 11 put on the board: the oracle's verdict per kind is
    the table the product's docstring states (goal_probe.ZOO_VERDICTS), which tests/test_goal_probe_host.py and the device test
    hold the product's step to"""
    spec = scenarios.objects_zoo_spec()
    e0 = O.OracleEnv(spec, P.SEED)
    e0.reset(observe=False)
    cells = P.zoo_cells(spec["W"], spec["H"], e0.state()["pos"])
    assert [o["type"] for o in spec["objects"][1:]] == ["Wall", "Goal", "Door", "Door", "Door", "Key", "Ball", "Lava", "Floor",
                                                        "BonusTile", "Box"]
    assert [o["state"] for o in spec["objects"][3:6]] == [O.DOOR_OPEN, O.DOOR_CLOSED, O.DOOR_LOCKED]

    def prepare(e):
        for i, (x, y) in enumerate(cells):
            e.put_obj(i + 1, x, y)

    base, verdict, _, _ = _oracle_verdicts(spec, prepare)
    _assert_every_kind_probed(base, verdict)
    assert [int(base[c]) for c in cells] == list(range(1, 12))
    assert [int(verdict[c]) for c in cells] == P.ZOO_VERDICTS
