"""The step bodies against the oracle on the action table, without a GPU: every case of tests/act_table.py through the host
build of mg_core.h's step — the sequential loop (`par=False`) and the lane-per-agent resolve / commit of the fused step with
its fall-back to the loop (`par=True`) —, one env per case, and after every step of the scripts: canonical state of every env,
stack order included; rewards to REW_TOL; `done`; the error word, mapped to the reference's exception class, at the step the
oracle raises and not before.  An env that raised is not compared afterwards.  tests/test_oracle_act_table.py pins the oracle
of these very cases to the reference."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE, os.path.join(HERE, "native")):
    if p not in sys.path:
        sys.path.insert(0, p)

import act_table as A  # noqa: E402
import canon  # noqa: E402
from marlgrid_amd import _native as N  # noqa: E402

REW_TOL = 1e-6      # per step: tests/test_core_hostemu.py


@pytest.fixture(scope="module")
def table():
    return A.cases()


@pytest.fixture(scope="module")
def traces(table):
    return {v: A.oracle_trace(batch) for v, batch in table.items()}


def _emu(batch, par):
    import hostemu
    from marlgrid_amd import objects as PO
    v = batch[0].variant
    emu = hostemu.HostEmu(A.NAME, len(batch), [c.seed for c in batch], par=par, **A.VARIANTS[v])
    emu.reset()
    A.register(emu.env, PO)
    emu.grid[:], emu.rec[:] = A.product_state(batch, emu.grid, emu.rec, N)
    return emu


@pytest.mark.parametrize("par", [False, True])
@pytest.mark.parametrize("variant", sorted(A.VARIANTS))
def test_host_step_against_the_oracle(table, traces, variant, par):
    batch, trace = table[variant], traces[variant]
    emu = _emu(batch, par)
    assert emu.env.ghost_mode == (variant != "noghost") and bool(emu.env.respawn) == (variant == "respawn")
    names = np.array([c.name for c in batch])
    before = np.ones(len(batch), bool)
    for t, want in enumerate(trace):
        rew, done = emu.step(A.actions(batch, t))
        err = A.error_names(emu.error, N)
        bad = before & (err != want["err"])
        assert not bad.any(), ("step %d: error words" % t, list(zip(names[bad], err[bad], want["err"][bad]))[:12], int(bad.sum()))
        live = want["live"]
        st = emu.canonical()
        for b in np.flatnonzero(live):
            canon.assert_same(st[b], want["canon"][b], "%s step %d" % (batch[b].name, t))
        assert np.abs(rew.astype(np.float64) - want["rewards"])[live].max() <= REW_TOL, t
        assert np.array_equal(done[live], want["done"][live]), t
        before = live
    raised = {c.name for c, ok in zip(batch, before) if not ok}
    assert raised == {n for n in A.expected_errors() if n in set(names)}
    if par:         # (sanity only: some env-steps took the sequential loop and some did not; WHAT the resolve must hand to
        # the loop is held by the parity asserts above — DESIGN.md 4.1's fault-injection record —, not by this count)
        assert emu.n_serial.value < len(batch) * A.STEPS
        assert (emu.n_serial.value > 0) == (variant != "respawn")        # (P: moves onto Lava and Goal, nothing for the loop)
