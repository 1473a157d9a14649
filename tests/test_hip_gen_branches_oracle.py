"""GPU (-m gpu): `_gen_grid` programs that branch on their draws or read per-env parameters — guarded ops (mg_core.h: gen_skipped,
the copy registers of nested forks), PARAM ops and symbolic counts in `reset_env`, inside every kernel that resets — against the
CPU oracle at width.  The oracle has the branches as `if` blocks and the parameters as plain values and is pinned to the
reference by tests/test_oracle_gen_branches.py; the same differential runs on the host build of `reset_env` in
tests/test_gen_branches_diff_host.py.

Everything is exact except rewards (<= 1e-6); all envs are compared (tests/wide_diff.py:run).  Coverage is a condition of each
case and is read on the oracle's side (tests/branch_diff.py:Coverage): every path of Choice, Sides, Long and Deep; every colour,
split column and door row of ColoredDoorKey; every value of a parameter, under both `_rand_bool` outcomes in `kind` and `long`; a
symbolic count of 0 in `clutter` and Deep; Deep's in-branch draw both made and not made; every env reset inside a launch at
least three times."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "native"))

import branch_diff  # noqa: E402
import gen_branch_envs as G  # noqa: E402
import param_envs as PE  # noqa: E402
import wide_diff  # noqa: E402

pytestmark = pytest.mark.gpu

K16, K4 = "mg::render_kernel<7, 8, 16, 0, 0>", "mg::render_kernel<7, 8, 4, 0, 0>"
K4_TS5 = "mg::render_kernel<7, 5, 4, 0, 2>"
CHOICE_TS5, SIDES9, LONG12, CDK8, DEEP = branch_diff.CHOICE7_TS5, branch_diff.SIDES9, branch_diff.LONG12, branch_diff.CDK8, branch_diff.DEEP
# id -> (scenario, max_steps, B, steps, obs_every, deep_every, constructor keywords beside auto_reset, stagger, kernel)
CASES = {
    "G1": (SIDES9, 10, 4099, 150, 25, 50, {}, False, K16),
    "G2": (CDK8, 20, 4099, 200, 25, 50, {}, False, K16),
    "G3": (CDK8, 20, 4099, 200, 25, 50, {"obs_format": "encoded"}, False, "mg::encode_views_kernel<7>"),
    "G4": (CDK8, 20, 4099, 220, 55, 55, {"auto_reset": "next_step", "episode_info": True}, True, K16),
    "G5-67": (LONG12, 10, 67, 150, 25, 50, {}, False, K4),
    "G5-4099": (LONG12, 10, 4099, 150, 25, 50, {}, False, K16),
    "G5-67-two-launches": (LONG12, 10, 67, 150, 25, 50, {"fused_step": False}, False, K4),
    "G5-67-encode-in-step": (LONG12, 10, 67, 150, 25, 50, {"encode_in_step": True}, False, K4),
    "G6": (CHOICE_TS5, 10, 67, 150, 25, 50, {}, False, K4_TS5),
    "G7-67": (DEEP, 10, 67, 150, 25, 50, {}, False, K4),
    "G7-4099": (DEEP, 10, 4099, 150, 25, 50, {}, False, K16),
    "G7-67-two-launches": (DEEP, 10, 67, 150, 25, 50, {"fused_step": False}, False, K4),
    # the soak: 64 envs, 2 000 steps, episodes of at most 25 steps, MultiGrid.encode written by the step's own launch
    "G9": (CDK8, 25, 64, 2000, 50, 250, {"encode_in_step": True}, False, K4),
}
for _kind in sorted(PE.KINDS):          # G8: the four parameter scenarios, mixed values, set_params at half time
    CASES["G8-%s-67" % _kind] = (PE.name_of(_kind), 10, 67, 150, 25, 50, {}, False, K4)
    CASES["G8-%s-4099" % _kind] = (PE.name_of(_kind), 10, 4099, 150, 25, 50, {}, False, K16)


def build(case, **more):
    name, max_steps, B, T, obs_every, deep_every, kw, stagger, kernel = CASES[case]
    kw = dict({"auto_reset": True}, **kw)
    kw.update(more)
    kw.update(batch_size=B, seeds=branch_diff.SEED0 + np.arange(B), place_obs=False, max_steps=max_steps)
    if name in branch_diff.PARAM:
        return PE.build(branch_diff.PARAM[name], **kw)
    if name == CDK8:
        from marlgrid_amd.envs import make
        return make(name, **kw)
    return G.build(name, **kw)


def run_case(case):
    name, max_steps, B, T, obs_every, deep_every, kw, stagger, kernel = CASES[case]
    env = build(case)
    assert env.kernel_name == kernel, (case, env.kernel_name)
    mode = "next_step" if kw.get("auto_reset") == "next_step" else "same_step"
    out, cov = branch_diff.run(wide_diff.HipSubject(env), name, branch_diff.SEED0 + np.arange(B), T, max_steps,
                               obs_every=obs_every, deep_every=deep_every, mode=mode, episode_info=bool(kw.get("episode_info")),
                               obs_format=kw.get("obs_format", "image"), stagger=stagger)
    assert env.kernel_name == kernel, (case, env.kernel_name)
    return env, out, cov


@pytest.mark.parametrize("case", [c for c in sorted(CASES) if c not in ("G4", "G9")])
def test_branch_program_vs_oracle(case):
    """G1 Sides, G2 ColoredDoorKey pixels, G3 its encoded views, G5 Long (guarded ops behind the LDS copy's 32) and G7 Deep on
    the launch paths, G6 Choice at 5-pixel tiles, G8 the parameter scenarios: same-step auto-reset, `max_steps` short enough
    that every env is reset inside a launch many times"""
    name, max_steps, B, T = CASES[case][:4]
    env, out, cov = run_case(case)
    assert out["episodes"].min() >= T // max_steps - 1
    if CASES[case][6].get("fused_step") is False:
        assert env.fused_step is False
    if CASES[case][6].get("encode_in_step"):
        assert env.encode_in_step


def test_g4_next_step_reset_with_episode_info_staggered():
    """ColoredDoorKey under auto_reset="next_step": every terminal observation and every info field of every env; the hand
    resets of the first 100 steps spread the episode ends over every later step"""
    env, out, cov = run_case("G4")
    assert out["terminal_obs"].min() >= 3 and out["partial_done_steps"] >= 100


def test_g9_soak_colored_doorkey():
    """64 envs x 2 000 steps.  The oracle alone (same seeds and actions, on the CPU) reaches 80 episodes in every env (80 - 80
    over the batch: no pair of agents reaches the goal behind a locked door by chance, every episode runs its 25 steps) and
    3 245 RNG words — 5.20 blocks of 624 — in the env that draws least (5.20 - 5.67 over the batch: two agents draw one shuffle
    word a step, a ColoredDoorKey reset about thirty)."""
    env, out, cov = run_case("G9")
    assert out["episodes"].min() >= 80, out["episodes"].min()
    assert out["blocks"].min() >= 5.2, out["blocks"].min()
