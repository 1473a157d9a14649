"""CPU: the interpreter of `_rand_int` draws (`reset_env`, marlgrid_amd/csrc/mg_core.h, built for the host) beside the CPU
oracle at width — 4 096 envs, 120 steps, every env compared (tests/wide_diff.py).  The oracle restates the draws in the
reference's terms (plain ints, no packed register, no device clamp; tests/test_oracle_gen_draws.py pins it to the reference),
so unlike the host emulation's own comparisons with the HIP kernels this one catches a WRONG interpreter, not only a
miscompiled one: with `gen_operand`'s half-select wrong for registers 4 - 7 (the low half read for every register), the
eight-draw case fails and names the envs, while Split and DoorKey — two draws, registers 0 and 1 — still pass."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "native"))

import draw_diff  # noqa: E402

B, T = 4096, 120
CASES = [(draw_diff.SPLIT7, 10), (draw_diff.DOORKEY8, 20), (draw_diff.EIGHT, 10)]


@pytest.mark.parametrize("name,max_steps", CASES, ids=[c[0] for c in CASES])
def test_host_emulation_vs_oracle_4096_envs(name, max_steps):
    seeds = draw_diff.SEED0 + np.arange(B)
    sub = draw_diff.host_subject(name, B, seeds, max_steps)
    out, cov = draw_diff.run(sub, name, seeds, T, max_steps, deep_every=40)
    assert out["episodes"].min() >= T // max_steps - 1
    assert cov.resets >= B * (T // max_steps)


def test_a_wrong_layout_is_caught_and_named():
    """the driver's own check on a draw program: one env's split column moved by hand between two steps"""
    import wide_diff
    name, max_steps, Bs, env = draw_diff.SPLIT7, 40, 256, 131
    seeds = draw_diff.SEED0 + np.arange(Bs)
    sub = draw_diff.host_subject(name, Bs, seeds, max_steps)

    def inject(t, subject):
        if t == 12:
            g = subject.emu.grid[env, :49].reshape(7, 7)
            s = int(np.nonzero((g[:, 1:6] == 1).sum(axis=1) >= 4)[0][1])     # (column 0 is the first such column)
            g[s, 1:6] = 0
    with pytest.raises(wide_diff.Mismatch) as ei:
        wide_diff.run(sub, name, seeds, 30, deep_every=15, spec=draw_diff.spec_for(name, max_steps), after_step=inject)
    assert ei.value.envs == [env] and 12 < ei.value.step <= 15


def test_d_cases_name_the_kernels_the_launcher_picks():
    """the kernel names of tests/test_hip_gen_draws_oracle.py:CASES, read off dry envs (no device); the GPU tests confirm each
    on the device, before and after the run"""
    import test_hip_gen_draws_oracle as G
    from marlgrid_amd import _native as N
    for case, (name, max_steps, Bc, Tc, obs_every, deep_every, kw, stagger, kernel) in sorted(G.CASES.items()):
        env = G.build(case, _dry=True)
        assert env.batch_size == Bc and env.max_steps == max_steps and Tc // max_steps >= 4, case
        if kw.get("obs_format") == "encoded":
            assert kernel == "mg::encode_views_kernel<%d>" % env.agents[0].view_size
        else:
            cfg, _raw, _flat, _atlas = env._host_tables()
            assert N.render_kernel_name(cfg)[0] == kernel, case
    assert G.CASES["D6-67"][8] == G.CASES["D6-130"][8] == "mg::render_kernel<0, 0, 4, 8, 3>"
