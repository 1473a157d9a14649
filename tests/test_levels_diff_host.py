"""CPU: whole levels — seed, parameters, cell edits — on the host build against the CPU oracle, through the driver the GPU rows
L1 - L7 use (tests/level_diff.py, tests/wide_diff.py:run with a LevelOracle as the reference): `reset_env` with its PARAM and
EDITS ops (tests/native/hostemu_edits.py), the body of mg_level_apply_rows (tests/native/mg_level_rows.cpp) in front of every
reset and step, and the host seed path (level_seed_row).  ALL envs are compared: done, rewards, every info field and
info["level"] every step, `episode_level` and the envs' own rows every step, canonical state, RNG and look-ahead words at every
deep check.  The launch itself — a wave's ballot and its 64-lane copy loop — is the GPU's to test
(tests/test_hip_levels_oracle.py); here `lanes` is 64 lanes taking turns, and 1.

The oracle is pinned to the reference first: tests/test_oracle_gen_edits.py (the edit list), tests/test_oracle_gen_branches.py
(parameters), tests/test_levels_host.py (a level is `env.seed(s); env.reset()`)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "native"))

import edit_envs as EE  # noqa: E402
import level_diff as LD  # noqa: E402
import level_envs as LE  # noqa: E402

MAX_STEPS = 10


def host_spec(name):
    """the hand-written spec as the HOST harness runs it: ClutteredMultiGrid(n_clutter_max=) records its reset program at the
    end of its constructor, and hostemu.HostEmu, which replays the constructor's reset from the dry env's last recording, then
    runs THAT — the reset program with every parameter at its default and no list — where the device ran the constructor's own
    (a random goal, no clutter; the GPU rows use the spec as it is)"""
    s = LE.spec_of(name, MAX_STEPS)
    if name == LE.CURRICULUM:
        s["gen_ctor"] = list(s["gen_reset"])
    return s


def subject(name, B, K, lanes=64, mode="next_step"):
    import hostemu_levels
    from marlgrid_amd.objects import Ball, Key
    with EE.registered():
        emu = hostemu_levels.LevelsEmu(name, B, LD.SEED0 + np.arange(B), lanes=lanes, mode=mode, level_edits=K, max_steps=MAX_STEPS)
    if name == LE.EDITS:
        assert (emu.env.edit_key(Key("blue")), emu.env.edit_key(Ball(color="red"))) == (LE.KEY, LE.BALL)
    return hostemu_levels.LevelsSubject(emu)


@pytest.mark.parametrize("name,lanes", [(LE.CURRICULUM, 64), (LE.EDITS, 64), (LE.CURRICULUM, 1)], ids=["curriculum", "edits-kinds", "one-lane"])
def test_full_bank_512_envs(name, lanes):
    """512 envs, K = 7 (a row of 28 bytes), 37 slots, 130 steps of episodes of at most 10: mixed lists, mixed `n_clutter`, ids
    with -1, a slot outside the bank and an emptied slot, the bank re-assigned at steps 30, 65 and 100 (the slot env 9 plays
    throughout among the slots, every time).  The oracle alone: every env but the 7 free-running ones starts >= 11 episodes from
    a level, every slot is played, 14 or more envs take one slot in one launch."""
    B, K, T = (512, 7, 130) if lanes == 64 else (131, 7, 60)
    sub = subject(name, B, K, lanes)
    plan = LD.BankPlan(name, B, K, T, assign_at=(30, 65, 100) if lanes == 64 else (30,))
    out, cov = LD.run(sub, name, plan, T, MAX_STEPS, "next_step", spec=host_spec(name), deep_every=10, episode_info=True, stagger=True)
    plan.require(out)
    if lanes == 64:
        resets = plan.lo.levelled + cov.free_episodes
        assert resets.min() >= 11, resets.min()                            # every env was reset >= 11 times
        print("levelled episodes per env %d - %d, resets %d - %d, slots shared by up to %d envs in a launch, %d episodes running "
              "across an assign" % (plan.lo.levelled[~plan.free].min(), plan.lo.levelled.max(), resets.min(), resets.max(),
                                    cov.max_shared, cov.across_assign))
    assert sub.emu.level_launches == T + 1 + min(T, 100)              # one launch per reset and step, hand resets included
    assert (sub.emu._last_prog._keep[-64:] == 0xA5).all()               # nothing behind the edit table was written


def test_seeds_form_with_plain_setters():
    """`set_levels(seeds=...)` with `set_params` / `set_edits` on the same envs between steps: the env takes the generator, its
    rows are its own"""
    B, K, T = 192, 5, 120
    sub = subject(LE.CURRICULUM, B, K)
    plan = LD.SeedsPlan(B, K, T)
    out, cov = LD.run(sub, LE.CURRICULUM, plan, T, MAX_STEPS, "next_step", spec=host_spec(LE.CURRICULUM), deep_every=10, episode_info=True, stagger=True)
    plan.require(out)


def test_masked_resets_by_hand():
    """no auto-reset: `set_levels(bank, ids, env_mask=mask)` then `reset(env_mask=mask)` with masks of one env, one whole wave,
    every other env and all; state and RNG after each reset"""
    B, K, T = 131, 5, 60
    sub = subject(LE.CURRICULUM, B, K, mode=None)
    plan = LD.MaskPlan(LE.CURRICULUM, B, K, T, assign_at=(22,))
    out, cov = LD.run(sub, LE.CURRICULUM, plan, T, MAX_STEPS, None, spec=host_spec(LE.CURRICULUM), deep_every=20)
    plan.require(out)


def test_plain_edits_same_step():
    """L1's plan on the host: same-step reset, the lists from a table with garbage entries, a third of the envs given new
    lists every 20 steps"""
    import hostemu_edits
    import wide_diff
    from marlgrid_amd.objects import Ball, Key
    B, K, T = 256, 7, 100
    with EE.registered():
        emu = hostemu_edits.EditsEmu(LE.EDITS, B, LD.SEED0 + np.arange(B), auto_reset=True, par=True, level_edits=K, max_steps=MAX_STEPS)
    assert (emu.env.edit_key(Key("blue")), emu.env.edit_key(Ball(color="red"))) == (LE.KEY, LE.BALL)
    sub = wide_diff.HostEmuSubject(emu)
    sub.level_state = lambda: dict(edits=emu.env.edits_t)
    plan = LD.EditsPlan(B, K, T)
    out, cov = LD.run(sub, LE.EDITS, plan, T, MAX_STEPS, "same_step", deep_every=10)
    plan.require(out)
