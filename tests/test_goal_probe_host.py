"""goal_distance's notion of a cell against what the step bodies DO, without a GPU (tests/goal_probe.py): every state of one grid
probed with one `forward` through the host build of mg_core.h's step — the serial body and the lane-parallel one of the fused
step —, the verdicts held to the flag rule of tests/goal_ref.py:kinds_of cell for cell, and the reverse queue search over the
PROBED maps held to the field the host builds of both kernels return for that grid."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
NATIVE = os.path.join(HERE, "native")
if NATIVE not in sys.path:
    sys.path.insert(0, NATIVE)

import goal_probe as P  # noqa: E402
import goal_ref as G  # noqa: E402
from marlgrid_amd import _native as N  # noqa: E402


def _fields(emu):
    """the field of env 0 on every host path the shape admits: general with 64 lanes and with 1, reg where it fits"""
    import hostemu_goal as HG
    cfg = emu._cfg()
    mask = np.zeros(emu.B, np.uint8)
    mask[0] = 1
    paths = [("general", 64), ("general", 1)] + ([("reg", 64)] if 4 * cfg.W <= 64 and cfg.H <= 64 else [])
    return {p: HG.run(cfg, emu.state, p[0], p[1], mask=mask)[1][0].copy() for p in paths}


def _probe(name, par, prepare=None):
    """-> (emu before-step facts, verdict map, counts, fields of the pre-step grid)"""
    import hostemu
    import scenarios
    spec = scenarios.registered(name)
    plan = P.Plan(spec["W"], spec["H"])
    W, H, B = plan.W, plan.H, plan.B
    emu = hostemu.HostEmu(name, B, [P.SEED] * B, par=par)
    emu.reset()
    if prepare is not None:
        prepare(emu)
    grid = emu.grid[:, :W * H].reshape(B, W, H).copy()
    pos0, _, flags = G.unpack_records(emu.rec)
    P.assert_probe_ready(grid, flags)
    fields = _fields(emu)
    emu.rec[:, 0] = plan.records(emu.rec[:, 0])
    rew, _ = emu.step(plan.actions(emu.n))
    pos, _, fl = G.unpack_records(emu.rec)
    want_err = plan.errors(grid[0], emu.env, pos[:, 0])
    assert np.array_equal(emu.error, want_err) and (want_err != 0).any() and (want_err == 0).any()
    assert np.array_equal(pos[~plan.probed, 0], pos0[~plan.probed, 0])
    verdict, counts = plan.verdicts(pos[:, 0], (fl[:, 0] & N.AF_DONE) != 0, rew[:, 0])
    return emu, grid[0], pos0[0], verdict, counts, fields


def _hold(emu, grid, verdict, fields, leave_out=()):
    return P.hold(*G.classify(grid, *G.kinds_of(emu.env)), verdict, fields, leave_out)


@pytest.mark.parametrize("par", [False, True])
@pytest.mark.parametrize("name", P.SCENES)
def test_probed_cells_are_the_rule_and_give_the_field(name, par):
    emu, grid, pos0, verdict, counts, fields = _probe(name, par)
    ids = set(np.unique(grid).tolist())
    if name == "Limit-3Agent100Kinds24x24":
        assert len(ids) == 102 and sorted(fields) == [("general", 1), ("general", 64)]
        assert counts == (1800, 64, 232), counts
        assert (verdict == P.GOAL).sum() == 15 + 1 and (verdict == P.FREE).sum() > 39
    if name == P.NOGHOST:       # other agents block: exactly the two cells under agents 1 and 2 read differently
        others = [(int(x), int(y)) for x, y in pos0[1:]]
        assert len(set(others)) == 2 and not emu.env.ghost_mode
        want = _hold(emu, grid, verdict, fields, leave_out=others)
    else:
        assert emu.env.ghost_mode
        want = _hold(emu, grid, verdict, fields)
    if name == "Edge-HumanPlayerConfig":        # bonus tiles, no goal
        assert (verdict != P.GOAL).all() and (want == -1).all()
    else:
        assert (want > 0).any() and (want == -1).any()


@pytest.mark.parametrize("par", [False, True])
def test_zoo_of_kinds(par):
    """a 9 x 7 room with one object of every kind written into the grid after the kinds were registered: the step's verdict per
    kind is the table of MultiGridEnv.goal_distance's docstring — free: open Door, Floor, BonusTile; goal: Goal; everything
    else blocks"""
    from marlgrid_amd import objects as PO
    zoo = P.zoo_objects(PO)
    placed = {}

    def prepare(emu):
        W, H = emu.env.width, emu.env.height
        pos, _, _ = G.unpack_records(emu.rec)
        assert (pos == pos[0]).all()
        n_before = len(emu.env.obj_reg.objs)
        for (kind, obj), (x, y) in zip(zoo, P.zoo_cells(W, H, pos[0])):
            key = emu.env.obj_reg.get_key(obj)
            emu.grid[:, x * H + y] = key
            placed[kind] = (x, y, key)
        assert len(emu.env.obj_reg.objs) > n_before         # the registry and the object table grew after the reset

    emu, grid, _, verdict, _, fields = _probe(P.ZOO, par, prepare)
    assert sorted(fields) == [("general", 1), ("general", 64), ("reg", 64)]
    assert [verdict[placed[kind][:2]] for kind, _ in zoo] == P.ZOO_VERDICTS
    assert len({key for _, _, key in placed.values()}) == len(zoo) and all(grid[x, y] == key for x, y, key in placed.values())
    want = _hold(emu, grid, verdict, fields)
    assert (want > 0).any()
