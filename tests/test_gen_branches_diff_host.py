"""CPU: the interpreter of guarded ops, PARAM ops and symbolic counts (`reset_env`, marlgrid_amd/csrc/mg_core.h, built for the
host) beside the CPU oracle at width — 4 096 envs, 120 steps, every env compared (tests/wide_diff.py).  The oracle has the
branches as `if` blocks and the parameters as plain values (tests/test_oracle_gen_branches.py pins it to the reference), so
unlike the host emulation's comparisons with the HIP kernels, and unlike the constant twins (which the same recorder records
and the same interpreter runs), this one catches a WRONG interpreter or recorder, not only a miscompiled one.

Every case must meet its coverage on the oracle's side (tests/branch_diff.py:Coverage): every path; for ColoredDoorKey every
colour, split column and door row; for a parameter every value of its interval, under both `_rand_bool` outcomes where the
text has one; a symbolic count of 0; in Deep the draw that only one path makes both made and not made."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "native"))

import branch_diff  # noqa: E402
import param_envs as PE  # noqa: E402

B, T, MAX_STEPS = 4096, 120, 10
CASES = [branch_diff.CHOICE7, branch_diff.SIDES9, branch_diff.LONG12, branch_diff.CDK8, branch_diff.DEEP] + sorted(branch_diff.PARAM)


@pytest.mark.parametrize("name", CASES)
def test_host_emulation_vs_oracle_4096_envs(name):
    seeds = branch_diff.SEED0 + np.arange(B)
    sub = branch_diff.host_subject(name, B, seeds, MAX_STEPS)
    out, cov = branch_diff.run(sub, name, seeds, T, MAX_STEPS, deep_every=40)
    assert out["episodes"].min() >= T // MAX_STEPS - 1
    assert cov.resets >= B * (T // MAX_STEPS - 1)
    if name in branch_diff.PARAM:           # the values of the second half were read: every other env holds another one now
        kind = branch_diff.PARAM[name]
        env, pname = sub.emu.env, PE.KINDS[kind][2]
        vals = PE.values(kind, B)
        want = vals.copy()
        want[::2] = branch_diff.second_values(kind, vals[::2])
        assert np.array_equal(np.asarray(env.params[pname]).astype(np.int64), want)


def test_a_count_below_zero_places_nothing():
    """`count` of a placement evaluated below 0 is no placement at all (marlgrid_hip.h; `for _ in range(count)`).  The recorder
    refuses a `_gen_grid` whose count can go below 0, so no recorded program reaches the interpreter's `cnt < 0` — the program
    is made by hand here: Param-clutter's own, its count operand rewritten from `n` to `n - 3` where it is packed, and the
    oracle's spec with ("place", wall, n - 3, 100).  Values 0 .. 20: three of them count below 0, one counts 0."""
    import hostemu_params
    import wide_diff
    import draw_envs as D
    PE.register()
    Bs, Ts, kind, pname = 512, 60, "clutter", "n"
    sym_n, sym_n_minus_3 = 0x40000000, 0x40000000 | (-3 & 0xFFFF)      # MG_GEN_SYM `const + draw[0]`, restated

    class Emu(hostemu_params.ParamEmu):
        def _prog(self, trace):
            template, ops = trace
            ops = [tuple(op[:1]) + (sym_n_minus_3,) + tuple(op[2:]) if op[1] == sym_n else tuple(op) for op in ops]
            assert sum(op[1] == sym_n_minus_3 for op in ops) == 1
            return super()._prog((template, ops))
    seeds = branch_diff.SEED0 + np.arange(Bs)
    sub = wide_diff.HostEmuSubject(Emu(PE.name_of(kind), Bs, seeds, auto_reset=True, par=True, max_steps=MAX_STEPS))
    spec = PE.spec(kind, max_steps=MAX_STEPS)
    for which in ("gen_ctor", "gen_reset"):
        spec[which] = [("place", 1, D.dr(0, -3), 100) if g[0] == "place" else g for g in spec[which]]
    vals = PE.values(kind, Bs)
    counts = set()

    def between(t, subject, envs):
        if t == 0:
            subject.emu.set_params(**{pname: vals})
            for b, e in enumerate(envs):
                e.set_params(**{pname: int(vals[b])})

    def watch(t, envs, mask):
        if t > 0:
            counts.update(int(envs[b].draws()[0][0]) - 3 for b in np.nonzero(mask)[0])
    out = wide_diff.run(sub, "Param-clutter, count n - 3", seeds, Ts, deep_every=20, spec=spec, watch=watch, between=between)
    assert out["episodes"].min() >= 3 and counts == set(range(-3, 18))
    W, H = sub.emu.env.width, sub.emu.env.height
    walls = (sub.emu.grid[:, :W * H].reshape(Bs, W, H)[:, 1:W - 1, 1:H - 1] == 1).sum(axis=(1, 2))
    assert np.array_equal(walls, np.maximum(vals - 3, 0))


def test_the_half_time_values_are_other_values_of_the_interval():
    for kind in PE.KINDS:
        lo, hi = PE.interval(kind)
        vals = PE.values(kind, 64)
        new = branch_diff.second_values(kind, vals)
        assert (new != vals).all() and new.min() >= lo and new.max() < hi and set(new.tolist()) == set(range(lo, hi))


def test_a_wrong_branch_is_caught_and_named():
    """the driver's own check on a guarded program: in one env the wall that only the `_rand_bool() == True` paths put at
    (1, 1) is toggled by hand between two steps"""
    import wide_diff
    name, Bs, env = branch_diff.SIDES9, 256, 77
    seeds = branch_diff.SEED0 + np.arange(Bs)
    sub = branch_diff.host_subject(name, Bs, seeds, 40)

    def inject(t, subject):
        if t == 12:
            g = subject.emu.grid[env, :81].reshape(9, 9)
            g[1, 1] = 0 if g[1, 1] == 1 else 1
    with pytest.raises(wide_diff.Mismatch) as ei:
        wide_diff.run(sub, name, seeds, 30, deep_every=15, spec=branch_diff.spec_for(name, 40), after_step=inject)
    assert ei.value.envs == [env] and 12 < ei.value.step <= 15


def test_g_cases_name_the_kernels_the_launcher_picks():
    """the kernel names of tests/test_hip_gen_branches_oracle.py:CASES, read off dry envs (no device); the GPU tests confirm
    each on the device, before and after the run"""
    import test_hip_gen_branches_oracle as G
    from marlgrid_amd import _native as N
    for case, (name, max_steps, Bc, Tc, obs_every, deep_every, kw, stagger, kernel) in sorted(G.CASES.items()):
        env = G.build(case, _dry=True)
        assert env.batch_size == Bc and env.max_steps == max_steps and Tc // max_steps >= 4, case
        if kw.get("obs_format") == "encoded":
            assert kernel == "mg::encode_views_kernel<%d>" % env.agents[0].view_size
        else:
            cfg, _raw, _flat, _atlas = env._host_tables()
            assert N.render_kernel_name(cfg)[0] == kernel, case
