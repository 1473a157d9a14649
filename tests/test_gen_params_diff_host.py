"""CPU: `reset_env` with PARAM ops and symbolic counts (marlgrid_amd/csrc/mg_core.h, built for the host) — a batch whose envs
hold different parameter values against the constant TWINS of tests/param_envs.py, env by env, and the twins against the CPU
oracle (all four kinds: it reads their forks as `if` blocks), so that `parameter env == twin == oracle == reference` closes.  The parameter table lies behind the template as on
the device (tests/native/hostemu_params.py).

The constructor's reset of a parameter env runs with the defaults and draws other RNG words than a twin's: both sides are
seeded again (`MultiGridEnv.seed()`'s seeds) after the values are set, then reset."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "native"))

import param_envs as PE  # noqa: E402

B, T, MAX_STEPS = 256, 40, 10
SEED0 = 616100
REW_TOL = 1e-6


def _emu(kind, twin_value=None, Bn=B, **kw):
    import hostemu_params
    PE.register()
    return hostemu_params.ParamEmu(PE.name_of(kind, twin_value), Bn, SEED0 + np.arange(Bn), auto_reset=True, par=True,
                                   max_steps=MAX_STEPS, **kw)


def _same_rows(emu, twin, m, what):
    for k in ("grid", "rec", "mt", "mt_pos", "mt_head", "step_count", "done", "error"):
        a, b = getattr(emu, k)[m], getattr(twin, k)[m]
        bad = np.nonzero((a != b).reshape(a.shape[0], -1).any(axis=1))[0]
        assert bad.size == 0, (what, k, np.nonzero(m)[0][bad][:8].tolist())


@pytest.mark.parametrize("kind", sorted(PE.KINDS))
def test_mixed_batch_equals_the_twins_env_by_env(kind):
    pname = PE.KINDS[kind][2]
    lo, hi = PE.interval(kind)
    vals = PE.values(kind, B)
    assert set(vals.tolist()) == set(range(lo, hi))                       # the whole interval
    emu = _emu(kind)
    emu.set_params(**{pname: vals})
    emu.reseed()
    emu.reset()
    twins = {}
    for v in range(lo, hi):
        twins[v] = t = _emu(kind, v)
        t.reseed()
        t.reset()
        _same_rows(emu, t, vals == v, "%s reset, value %d" % (kind, v))
    rng = np.random.RandomState(7)
    ends = np.zeros(B, np.int64)
    for step in range(T):
        a = rng.randint(0, 7, size=(B, emu.n))
        r, d = emu.step(a)
        ends += d
        for v, t in twins.items():
            r2, d2 = t.step(a)
            m = vals == v
            assert np.array_equal(d[m], d2[m]) and np.abs(r[m] - r2[m]).max() <= REW_TOL, (kind, v, step)
            _same_rows(emu, t, m, "%s step %d, value %d" % (kind, step, v))
    assert ends.min() >= T // MAX_STEPS - 1                               # every env was reset inside a launch, repeatedly
    # the guard band behind the table and the grid's tail: nothing was written outside the grid slice
    W, H = emu.env.width, emu.env.height
    assert not emu.grid[:, W * H:].any()
    assert (emu._last_prog._keep[-64:] == 0xA5).all()


# the twins against the oracle, every value of every kind: the oracle runs the hand-written twin spec (tests/param_envs.py:spec
# — an `if` block where `kind` and `long` fork on a `_rand_bool`), not what the product's recorder made of the twin
ORACLE_TWINS = [(kind, v) for kind in sorted(PE.KINDS) for v in range(*PE.interval(kind))]


@pytest.mark.parametrize("kind,v", ORACLE_TWINS, ids=["%s-%d" % c for c in ORACLE_TWINS])
def test_twins_against_the_oracle(kind, v):
    import hostemu
    import wide_diff
    PE.register()
    Bn = 64
    seeds = SEED0 + np.arange(Bn)
    sub = wide_diff.HostEmuSubject(hostemu.HostEmu(PE.name_of(kind, v), Bn, seeds, auto_reset=True, par=True, max_steps=MAX_STEPS))
    out = wide_diff.run(sub, PE.name_of(kind, v), seeds, T, deep_every=20, spec=PE.spec(kind, v, max_steps=MAX_STEPS))
    assert out["episodes"].min() >= T // MAX_STEPS - 1


def test_a_table_of_0xff_is_the_upper_end_everywhere():
    for kind in sorted(PE.KINDS):
        lo, hi = PE.interval(kind)
        Bn = 32
        emu = _emu(kind, Bn=Bn)
        emu.table = np.full((Bn, 8), 0xFF, np.uint8)
        emu.reseed()
        emu.reset()
        twin = _emu(kind, hi - 1, Bn=Bn)
        twin.reseed()
        twin.reset()
        everyone = np.ones(Bn, bool)
        _same_rows(emu, twin, everyone, "%s reset" % kind)
        rng = np.random.RandomState(9)
        for step in range(25):
            a = rng.randint(0, 7, size=(Bn, emu.n))
            r, d = emu.step(a)
            r2, d2 = twin.step(a)
            assert np.array_equal(d, d2) and np.abs(r - r2).max() <= REW_TOL
            _same_rows(emu, twin, everyone, "%s step %d" % (kind, step))
        W, H = emu.env.width, emu.env.height
        assert not emu.grid[:, W * H:].any()                             # the grid tail stays zero
        assert (emu._last_prog._keep[-64:] == 0xA5).all()                # ... and nothing behind the table was touched
    # below the interval as well: `split` starts at 2, a table of zeros is its lower end
    emu = _emu("split", Bn=16)
    emu.table = np.zeros((16, 8), np.uint8)
    emu.reseed()
    emu.reset()
    twin = _emu("split", 2, Bn=16)
    twin.reseed()
    twin.reset()
    _same_rows(emu, twin, np.ones(16, bool), "split, a table of zeros")


def test_set_params_changes_nothing_until_the_env_resets():
    kind, pname = "clutter", "n"
    Bn = 64
    emu = _emu(kind, Bn=Bn)
    wall = 1
    W, H = emu.env.width, emu.env.height

    def walls():
        return (emu.grid[:, :W * H].reshape(Bn, W, H)[:, 1:W - 1, 1:H - 1] == wall).sum(axis=(1, 2))
    emu.set_params(**{pname: 3})
    emu.reseed()
    emu.reset()
    assert (walls() == 3).all()
    rng = np.random.RandomState(11)
    current = np.full(Bn, 3)
    for step in range(30):
        if step == 4:
            before = emu.grid.copy()
            emu.set_params(**{pname: 17})
            assert np.array_equal(emu.grid, before)
        if step == 15:
            emu.set_params(env_ids=np.arange(0, Bn, 2), **{pname: 0})
        r, d = emu.step(rng.randint(0, 7, size=(Bn, emu.n)))
        current[d] = emu.env.params[pname][d]                             # an env that reset in the launch read its value then
        assert np.array_equal(walls(), current), step
    assert set(current.tolist()) == {0, 17}
