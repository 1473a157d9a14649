"""CPU: `reset_env` with an EDITS op (marlgrid_amd/csrc/mg_core.h, built for the host) — a batch whose envs hold different edit
lists against the constant TWINS of tests/edit_envs.py, env by env, and the twins against the CPU oracle through a hand-written
spec, so that `edits env == twin == oracle == reference` closes.  The edit table lies behind the template and the parameter
table as on the device, with a guard band behind it (tests/native/hostemu_edits.py).

The constructor's reset of an edits env runs with empty lists and draws other RNG words than a twin's: both sides are seeded
again (`MultiGridEnv.seed()`'s seeds) after the lists are set, then reset."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "native"))

import edit_envs as EE  # noqa: E402

B, T, MAX_STEPS = 256, 40, 10
SEED0 = 717100
REW_TOL = 1e-6
ROWS = ("grid", "rec", "mt", "mt_pos", "mt_head", "step_count", "done", "error")


def _emu(i=None, K=4, Bn=B, **kw):
    import hostemu_edits
    if i is None:
        kw["level_edits"] = K
    with EE.registered():
        return hostemu_edits.EditsEmu(EE.name_of(i, K), Bn, SEED0 + np.arange(Bn), auto_reset=True, par=True,
                                      max_steps=MAX_STEPS, **kw)


def _started(emu):
    emu.reseed()
    emu.reset()
    return emu


def _same_rows(emu, twin, m, what):
    for k in ROWS:
        a, b = getattr(emu, k)[m], getattr(twin, k)[m]
        bad = np.nonzero((a != b).reshape(a.shape[0], -1).any(axis=1))[0]
        assert bad.size == 0, (what, k, np.nonzero(m)[0][bad][:8].tolist())


def _untouched(emu):
    """the grid tail [W * H, cells_stride) is zero and nothing behind the edit table was written"""
    assert not emu.grid[:, EE.W * EE.H:].any()
    assert (emu._last_prog._keep[-64:] == 0xA5).all()


@pytest.mark.parametrize("K", [4, 7])           # (K = 7: a row of 28 bytes, no multiple of 16)
def test_mixed_batch_equals_the_twins_env_by_env(K):
    tab, which = EE.table(K, B)
    emu = _emu(K=K)
    emu.set_edits(tab)
    assert np.array_equal(emu.env.edits_t, tab)
    _started(emu)
    twins = {}
    for i in range(4):
        twins[i] = t = _started(_emu(i, K))
        _same_rows(emu, t, which == i, "K %d reset, list %d" % (K, i))
    # the lists did what they say (against the twins this would hold vacuously if neither side applied anything)
    g = emu.grid[:, :EE.W * EE.H].reshape(B, EE.W, EE.H)
    assert (g[which == 1, 7, 7] == EE.WALL).all()
    assert (g[which == 2, 4, 9] == EE.WALL).all() and (g[which == 2, 3, 3] == EE.GOAL).all() and (g[which == 2, 13, 13] == 0).all()
    assert (g[which == 3, 1, 7] == 0).all() and (g[which == 3, 2, 2] == EE.WALL).all()
    assert (g[which != 2, 13, 13] == EE.GOAL).all()
    rng = np.random.RandomState(7)
    ends = np.zeros(B, np.int64)
    for step in range(T):
        a = rng.randint(0, 7, size=(B, emu.n))
        r, d = emu.step(a)
        ends += d
        for i, t in twins.items():
            r2, d2 = t.step(a)
            m = which == i
            assert np.array_equal(d[m], d2[m]) and np.abs(r[m] - r2[m]).max() <= REW_TOL, (K, i, step)
            _same_rows(emu, t, m, "K %d step %d, list %d" % (K, step, i))
    assert ends.min() >= T // MAX_STEPS - 1                               # every env was reset inside a launch, repeatedly
    assert not emu.error.any()
    _untouched(emu)


ORACLE_TWINS = [(K, i) for K in (4, 7) for i in range(4)]


@pytest.mark.parametrize("K,i", ORACLE_TWINS, ids=["K%d-L%d" % c for c in ORACLE_TWINS])
def test_twins_against_the_oracle(K, i):
    """the oracle runs the hand-written spec — the base scenario's entries plus the fills —, not what the recorder made"""
    import hostemu
    import wide_diff
    Bn = 64
    seeds = SEED0 + np.arange(Bn)
    with EE.registered():
        emu = hostemu.HostEmu(EE.name_of(i, K), Bn, seeds, auto_reset=True, par=True, max_steps=MAX_STEPS)
    sub = wide_diff.HostEmuSubject(emu)
    out = wide_diff.run(sub, EE.name_of(i, K), seeds, T, deep_every=20, spec=EE.spec(i, K, max_steps=MAX_STEPS))
    assert out["episodes"].min() >= T // MAX_STEPS - 1                     # (run() itself asserts that no env recorded an error)


def _garbage_tables(K, Bn):
    """every byte 0xFF; then x = W, y = H, kind = n_obj, each alone, with on = 1 — in every slot of every env"""
    n_obj = 3
    yield "0xFF", np.full((Bn, K, 4), 0xFF, np.uint8)
    for what, entry in (("x = W", (EE.W, 5, EE.WALL, 1)), ("y = H", (5, EE.H, EE.WALL, 1)), ("kind = n_obj", (5, 5, n_obj, 1))):
        yield what, np.tile(np.asarray(entry, np.uint8), (Bn, K, 1))


@pytest.mark.parametrize("K", [4, 7])
def test_a_garbage_table_changes_nothing(K):
    Bn = 32
    everyone = np.ones(Bn, bool)
    for what, tab in _garbage_tables(K, Bn):
        emu = _emu(K=K, Bn=Bn)
        assert len(emu.env.obj_reg.objs) == 3
        emu.edit_table = tab
        _started(emu)
        twin = _started(_emu(0, K, Bn=Bn))
        _same_rows(emu, twin, everyone, "%s reset" % what)
        rng = np.random.RandomState(9)
        for step in range(25):
            a = rng.randint(0, 7, size=(Bn, emu.n))
            r, d = emu.step(a)
            r2, d2 = twin.step(a)
            assert np.array_equal(d, d2) and np.abs(r - r2).max() <= REW_TOL, (what, step)
            _same_rows(emu, twin, everyone, "%s step %d" % (what, step))
        _untouched(emu)


def test_set_edits_changes_nothing_until_the_env_resets():
    Bn, K = 64, 4
    emu = _started(_emu(K=K, Bn=Bn))

    def goal_at_77():
        return emu.grid[:, 7 * EE.H + 7] == EE.GOAL          # (nothing else puts a goal there: the scenario's sits in the corner)
    assert not goal_at_77().any()
    rng = np.random.RandomState(11)
    current = np.zeros(Bn, bool)
    for step in range(30):
        if step == 4:
            before = emu.grid.copy()
            emu.set_edits([(7, 7, EE.GOAL, 1)])
            assert np.array_equal(emu.grid, before)
        if step == 15:
            emu.set_edits([], env_ids=np.arange(0, Bn, 2))
        r, d = emu.step(rng.randint(0, 7, size=(Bn, emu.n)))
        current[d] = emu.env.edits_t[d, 0, 3] != 0                        # an env that reset in the launch read its list then
        assert np.array_equal(goal_at_77(), current), step
    assert current[1::2].all() and not current[0::2].any()
