"""GPU (-m gpu): WHOLE LEVELS — seed, parameters, cell edits — against the CPU oracle at width, rows L1 - L7 of DESIGN.md §4.1: the
EDITS op of `reset_env` inside every kernel that resets, and `mg_level_apply_rows`, the wave-shaped launch that hands an env its
level (a ballot, readfirstlane / readlane, a 64-lane copy loop over 161 + 2 + K items), at more than one wave, with a ragged last
wave, with all 64 lanes of a wave selected and with exactly one, at K = 1, 5, 7 and 64, inside a 16-wave-workgroup step.

The oracle holds a level as a freshly seeded env with plain parameter values and a plain ordered list (tests/level_ref.py) and is
pinned to the reference first: tests/test_oracle_gen_edits.py (the list), tests/test_oracle_gen_branches.py (parameters),
tests/test_levels_host.py (the seed).  The same plans run on the host build in tests/test_levels_diff_host.py.

All envs are compared (tests/wide_diff.py:run through tests/level_diff.py): rewards to 1e-6, everything else exact — done, every
info field and info["level"], every terminal observation, `episode_level`, the envs' own `params_t` / `edits_t` rows every step;
whole observation tensors every `obs_every`-th step; canonical state, RNG and look-ahead words every `deep_every`-th.
`place_obs=False`, seeds SEED0 + arange(B), `max_steps` 10 (25 in the soak).  Coverage is a condition of every case and is read on
the oracle's side (tests/level_diff.py:Coverage)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "native"))

import level_diff as LD  # noqa: E402
import level_envs as LE  # noqa: E402
import wide_diff  # noqa: E402

pytestmark = pytest.mark.gpu

K16, K4 = "mg::render_kernel<7, 8, 16, 0, 0>", "mg::render_kernel<7, 8, 4, 0, 0>"
ENC = "mg::encode_views_kernel<7>"
NEXT = {"auto_reset": "next_step", "episode_info": True}
BOX64 = (1, 1, 9, 9)        # L5: 64 cells for up to 64 edits — with 25 blocks of clutter and the goal >= 60 of 169 cells stay free
# id -> (scenario, plan, K, max_steps, B, steps, obs_every, deep_every, constructor keywords, stagger, kernel)
CASES = {
    "L1-4099": (LE.EDITS, "edits", 7, 10, 4099, 150, 25, 50, {"auto_reset": True}, False, K16),
    "L1-67": (LE.EDITS, "edits", 7, 10, 67, 150, 25, 50, {"auto_reset": True}, False, K4),
    "L1-67-two-launches": (LE.EDITS, "edits", 7, 10, 67, 150, 25, 50, {"auto_reset": True, "fused_step": False}, False, K4),
    "L1-67-encode-in-step": (LE.EDITS, "edits", 7, 10, 67, 150, 25, 50, {"auto_reset": True, "encode_in_step": True}, False, K4),
    "L1-67-encoded": (LE.EDITS, "edits", 7, 10, 67, 150, 25, 50, {"auto_reset": True, "obs_format": "encoded"}, False, ENC),
    "L2-4099": (LE.CURRICULUM, "bank", 5, 10, 4099, 200, 50, 50, NEXT, True, K16),
    "L2-67": (LE.CURRICULUM, "bank", 5, 10, 67, 200, 50, 50, NEXT, True, K4),
    "L3": (LE.CURRICULUM, "bank", 5, 10, 4099, 200, 50, 50, dict(NEXT, obs_delta=True), True, K16),
    "L4": (LE.CURRICULUM, "seeds", 5, 10, 4099, 220, 55, 55, NEXT, True, K16),
    "L5-K64": (LE.EDITS, "bank", 64, 10, 67, 150, 25, 50, NEXT, True, K4),
    "L5-K1": (LE.EDITS, "bank", 1, 10, 67, 150, 25, 50, NEXT, True, K4),
    "L6": (LE.CURRICULUM, "masks", 5, 10, 131, 60, 20, 20, {"auto_reset": False}, False, K4),
    "L7": (LE.CURRICULUM, "bank", 5, 25, 64, 2000, 50, 250, dict(NEXT, encode_in_step=True), True, K4),
}


def plan_for(case):
    name, kind, K, max_steps, B, T = CASES[case][:6]
    if kind == "edits":
        return LD.EditsPlan(B, K, T)
    if kind == "seeds":
        return LD.SeedsPlan(B, K, T)
    if kind == "masks":
        return LD.MaskPlan(name, B, K, T, assign_at=(22,))
    assign_at = tuple(range(100, T, 100)) if case == "L7" else (T // 4, T // 2, 3 * T // 4)
    return LD.BankPlan(name, B, K, T, assign_at=assign_at, box=BOX64 if case.startswith("L5") else (1, 1, LE.W - 1, LE.H - 1))


def mode_of(case):
    ar = CASES[case][8].get("auto_reset")
    return "next_step" if ar == "next_step" else "same_step" if ar else None


def build(case):
    name, kind, K, max_steps, B = CASES[case][:5]
    kw = dict(CASES[case][8], batch_size=B, seeds=LD.SEED0 + np.arange(B), place_obs=False, max_steps=max_steps, level_edits=K)
    return LE.build(name, **kw)


def run_case(case):
    name, kind, K, max_steps, B, T, obs_every, deep_every, kw, stagger, kernel = CASES[case]
    env = build(case)
    assert env.kernel_name == kernel, (case, env.kernel_name)
    plan = plan_for(case)
    out, cov = LD.run(wide_diff.HipSubject(env), name, plan, T, max_steps, mode_of(case), obs_every=obs_every, deep_every=deep_every,
                      episode_info=bool(kw.get("episode_info")), obs_format=kw.get("obs_format", "image"), stagger=stagger)
    assert env.kernel_name == kernel, (case, env.kernel_name)
    print("%s: seconds %s" % (case, out["seconds"]))
    return env, plan, out, cov


@pytest.mark.parametrize("case", [c for c in sorted(CASES) if c.startswith("L1")])
def test_l1_edit_lists_same_step(case):
    """`Edits-Cluttered15`, K = 7, same-step reset.  Every env has its own random list (a RandomState's), set from a device
    tensor that also holds garbage entries in random slots; a third of the envs get new lists every 20 steps, by mask and by ids in
    turn.  Among the lists: one cell twice, entries that are off, a Key, a Ball, the goal moved, nothing at all.  The oracle alone,
    at 67 and at 4 099 envs: every garbage class (off, x outside, y outside, unknown kind) is in a table; a Key and a Ball placed
    by an edit are both seen in an agent's hands (every env is looked at every 5th step); every env ends 15 episodes."""
    env, plan, out, cov = run_case(case)
    plan.require(out)
    T, max_steps = CASES[case][5], CASES[case][3]
    assert out["episodes"].min() >= T // max_steps - 1
    kw = CASES[case][8]
    assert env.fused_step is not False or kw.get("fused_step") is False
    assert bool(env.encode_in_step) == bool(kw.get("encode_in_step"))


@pytest.mark.parametrize("case", ["L2-4099", "L2-67", "L3"])
def test_l2_l3_full_bank_next_step(case):
    """The curriculum scenario with `level_edits=5` (a row of 20 bytes) and a full bank of 37 slots under auto_reset="next_step"
    with episode_info, staggered: `set_levels(bank, ids, env_mask=done)` before every step — ids with -1, a slot outside the
    bank and an emptied slot —, `bank.assign(slots, seeds, params=, edits=)` from device tensors at steps 50, 100 and 150.  L3 is
    the same under obs_delta=True: every step is the delta launch.  200 steps, not L4's 220: at 220 the row cost 2.06 times G4's
    seconds on the same machine, and a row that costs more than twice G4 gives up steps, never width.  The oracle alone, at 4 099
    envs (67): every env but the 64 (1) free-running ones starts 11 (13) or more episodes from a level, every slot is played, up
    to 121 (14) envs take one slot in one launch, the first reset selects all 64 lanes of wave 0, 4 703 (98) times a launch
    selects exactly one lane of a wave, the last env of the ragged wave takes a level 17 (19) times, 1 397 (23) episodes are
    running across an assign to their slot; the free-running envs keep their own rows throughout."""
    env, plan, out, cov = run_case(case)
    plan.require(out)
    T = CASES[case][5]
    assert out["terminal_obs"].min() >= 3 and out["partial_done_steps"] >= 100
    assert env._level_launches == T + 1 + 100 and plan.bank.launches == 1 + 3       # one small launch per reset, hand reset and step
    if case == "L3":
        assert env._delta_launches == T


def test_l4_seeds_form_with_set_params_and_set_edits():
    """The README's "parameters together with `set_levels`": `set_levels(seeds=..., env_mask=done)` before every step, and plain
    `set_params` / `set_edits` on a third of the same envs every 15 steps — the env takes the generator alone and its reset
    reads its own rows.  4 099 envs."""
    env, plan, out, cov = run_case("L4")
    plan.require(out)
    assert out["terminal_obs"].min() >= 3


@pytest.mark.parametrize("case", ["L5-K64", "L5-K1"])
def test_l5_bank_at_k64_and_k1(case):
    """`Edits-Cluttered15` with a full bank whose lists hold a Key and a Ball: K = 64 is four rounds of the 64-lane copy loop
    (161 + 2 + 64 items), K = 1 a row of 4 bytes.  At K = 64 the edits stay inside an 8 x 8 box: >= 60 cells are free."""
    env, plan, out, cov = run_case(case)
    plan.require(out, wide=False)
    assert cov.full_waves >= 1                                                       # (the first reset: all of wave 0)
    if case == "L5-K64":
        assert max(len(lst) for lst in plan.bankref.edits) > 48                      # a list that needs the fourth round


def test_l6_masked_resets_without_auto_reset():
    """auto_reset=False, 131 envs: `set_levels(bank, ids, env_mask=mask)` then `reset(env_mask=mask)` every 5 steps with masks of
    one env (the first: the last env of the ragged wave), one whole wave, every other env, and all; state and RNG of every env
    after each reset"""
    env, plan, out, cov = run_case("L6")
    plan.require(out)


def test_l7_soak():
    """64 envs x 2 000 steps of L2's plan with `encode_in_step`, episodes of at most 25 steps, `assign` every 100 steps.  The
    oracle alone: every env but the free-running one starts 70 or more episodes from a level."""
    env, plan, out, cov = run_case("L7")
    plan.require(out, wide=False)
    assert env.encode_in_step
    assert plan.lo.levelled[~plan.free].min() >= 60, plan.lo.levelled[~plan.free].min()
