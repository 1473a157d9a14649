"""GPU (-m gpu): `_gen_grid` programs with `_rand_int` draws — the interpreter in `reset_env` (mg_core.h: gen_operand, the 64-bit
draw register, the device clamp, the packed rectangle), inside every kernel that resets — against the CPU oracle at width.
The oracle restates the draws in the reference's terms and is pinned to the reference by tests/test_oracle_gen_draws.py; the
same differential runs on the host build of `reset_env` in tests/test_gen_draws_diff_host.py.

Everything is exact except rewards (<= 1e-6); all envs are compared (tests/wide_diff.py:run).  Coverage is a condition of
each case and is read on the oracle's side (tests/draw_diff.py:Coverage): every legal split column and gap / door row; in D5
registers 4 - 7 with two values each, the overhanging place_obj clamped in some envs and not in others, a draw that took more
than one RNG word; in D6 draws on both sides of 128; every env reset inside a launch at least three times."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "native"))

import draw_diff  # noqa: E402
import draw_envs as D  # noqa: E402
import wide_diff  # noqa: E402

pytestmark = pytest.mark.gpu

K16, K4 = "mg::render_kernel<7, 8, 16, 0, 0>", "mg::render_kernel<7, 8, 4, 0, 0>"
SPLIT7, DOORKEY8, EIGHT, IN_PLACE = draw_diff.SPLIT7, draw_diff.DOORKEY8, draw_diff.EIGHT, draw_diff.IN_PLACE
# id -> (scenario, max_steps, B, steps, obs_every, deep_every, constructor keywords beside auto_reset, stagger, kernel)
CASES = {
    "D1": (SPLIT7, 10, 4099, 150, 25, 50, {}, False, K16),
    "D2": (DOORKEY8, 20, 4099, 200, 25, 50, {}, False, K16),
    "D3": (DOORKEY8, 20, 4099, 200, 25, 50, {"obs_format": "encoded"}, False, "mg::encode_views_kernel<7>"),
    "D4": (DOORKEY8, 20, 4099, 220, 55, 55, {"auto_reset": "next_step", "episode_info": True}, True, K16),
    "D5-67": (EIGHT, 10, 67, 150, 25, 50, {}, False, K4),
    "D5-4099": (EIGHT, 10, 4099, 150, 25, 50, {}, False, K16),
    "D5-67-two-launches": (EIGHT, 10, 67, 150, 25, 50, {"fused_step": False}, False, K4),
    "D5-67-encode-in-step": (EIGHT, 10, 67, 150, 25, 50, {"encode_in_step": True}, False, K4),
    "D6-67": (IN_PLACE, 10, 67, 60, 10, 20, {}, False, D.IN_PLACE_KERNEL),
    "D6-130": (IN_PLACE, 10, 130, 60, 10, 20, {}, False, D.IN_PLACE_KERNEL),
    # the soak: 64 envs, 2 000 steps, episodes of at most 25 steps, MultiGrid.encode written by the step's own launch
    "D7": (DOORKEY8, 25, 64, 2000, 50, 250, {"encode_in_step": True}, False, K4),
}


def build(case, **more):
    name, max_steps, B, T, obs_every, deep_every, kw, stagger, kernel = CASES[case]
    D.register()
    kw = dict({"auto_reset": True}, **kw)
    kw.update(more)
    return D.build(name, batch_size=B, seeds=draw_diff.SEED0 + np.arange(B), place_obs=False, max_steps=max_steps, **kw)


def run_case(case):
    name, max_steps, B, T, obs_every, deep_every, kw, stagger, kernel = CASES[case]
    env = build(case)
    assert env.kernel_name == kernel, (case, env.kernel_name)
    mode = "next_step" if kw.get("auto_reset") == "next_step" else "same_step"
    out, cov = draw_diff.run(wide_diff.HipSubject(env), name, draw_diff.SEED0 + np.arange(B), T, max_steps,
                             obs_every=obs_every, deep_every=deep_every, mode=mode, episode_info=bool(kw.get("episode_info")),
                             obs_format=kw.get("obs_format", "image"), stagger=stagger)
    assert env.kernel_name == kernel, (case, env.kernel_name)
    return env, out, cov


@pytest.mark.parametrize("case", [c for c in sorted(CASES) if c not in ("D4", "D7")])
def test_draw_program_vs_oracle(case):
    """D1 Split, D2 DoorKey pixels, D3 DoorKey encoded views, D5 the eight-draw scenario on every launch path, D6 the
    grid-in-place kernel: same-step auto-reset, `max_steps` short enough that every env is reset inside a launch many times"""
    name, max_steps, B, T = CASES[case][:4]
    env, out, cov = run_case(case)
    assert out["episodes"].min() >= T // max_steps - 1
    if CASES[case][6].get("fused_step") is False:
        assert env.fused_step is False
    if CASES[case][6].get("encode_in_step"):
        assert env.encode_in_step


def test_d4_next_step_reset_with_episode_info_staggered():
    """DoorKey under auto_reset="next_step": every terminal observation and every info field of every env; the hand resets of
    the first 100 steps spread the episode ends over every later step"""
    env, out, cov = run_case("D4")
    assert out["terminal_obs"].min() >= 3 and out["partial_done_steps"] >= 100


def test_d7_soak_doorkey():
    """64 envs x 2 000 steps.  The oracle alone (same seeds and actions, on the CPU) reaches 80 episodes in every env (80 - 81
    over the batch) and 5.02 blocks of 624 RNG words in the env that draws least (5.02 - 5.46 over the batch: two agents draw
    one shuffle word a step, a DoorKey reset about thirty)."""
    env, out, cov = run_case("D7")
    assert out["episodes"].min() >= 80, out["episodes"].min()
    assert out["blocks"].min() >= 5.0, out["blocks"].min()
