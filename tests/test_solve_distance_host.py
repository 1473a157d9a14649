"""solve_distance without a GPU: the bodies of mg_solve_distance (marlgrid_amd/csrc/mg_solve_core.h, the text the kernel of
mg_solve_dist.hip runs) built with g++ (tests/native/mg_solve_dist.cpp, every scratch index asserted) and run with 64 lanes
and with 1 — against tests/solve_ref.py: distance, first action and `exact`, on the host emulation's own state arrays of the
DoorKey scenarios, on grids made by hand and on the edge shapes (tests/solve_cases.py; the device runs the same in
tests/test_hip_solve_distance.py), and a run that follows the policy to the goal."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
NATIVE = os.path.join(HERE, "native")
if NATIVE not in sys.path:
    sys.path.insert(0, NATIVE)

import goal_ref as G  # noqa: E402
import solve_cases as SC  # noqa: E402
import solve_ref as S  # noqa: E402
from marlgrid_amd import _native as N  # noqa: E402


def _check(cfg, state, want, caps=(2, 2), mask=None):
    import hostemu_solve as HS
    for lanes in (64, 1):
        dist, act, exact = HS.run(cfg, state, lanes, mask=mask, max_doors=caps[0], max_items=caps[1])
        sel = slice(None) if mask is None else np.asarray(mask, bool)
        assert np.array_equal(dist[sel], want[0][sel]), (lanes, np.argwhere(dist[sel] != want[0][sel])[:5])
        assert np.array_equal(act[sel], want[1][sel]), (lanes, np.argwhere(act[sel] != want[1][sel])[:5])
        assert np.array_equal(exact[sel], want[2][sel].astype(np.uint8)), lanes
        if mask is not None:
            assert (dist[~sel] == -7).all() and (act[~sel] == -7).all() and (exact[~sel] == 0xF9).all(), lanes


@pytest.mark.parametrize("name,B,steps", SC.SCENARIOS)
def test_scenarios_match_the_reference(name, B, steps):
    emu, grid, kinds, want = SC.emu_batch(name, B, steps)
    _check(emu._cfg(), emu.state, want)
    assert want[2].all()        # one door and one key, or none of either: nothing beyond the default caps


def test_the_stepped_batches_hold_carried_keys_and_half_opened_doors():
    """after 30 random steps: agents that carry the key in every DoorKey batch, and doors unlocked but still shut in two of them
    (the coloured batch's random walk unlocks none)"""
    seen = {}
    for name in (SC.DK8, SC.DK6, SC.CDK8):
        emu, grid, kinds, want = SC.emu_batch(name, 512, 30)
        seen[name] = SC.half_open_and_carried(grid, kinds, emu.rec)
        assert (want[0] > 0).any() and (want[0] < 0).any()
    assert all(c >= 10 for _, c in seen.values()), seen
    assert seen[SC.DK8][0] >= 1 and seen[SC.DK6][0] >= 1, seen


@pytest.mark.parametrize("name,blind,longest", [(SC.DK8, 491, 27), (SC.DK6, 445, 19), (SC.CDK8, 494, 29)])
def test_after_the_reset_every_pair_has_a_path_and_goal_distance_sees_half(name, blind, longest):
    """seeds 1337 + b right after reset(): the static analysis answers -1 for about half of the 1 024 agent-env pairs; through
    the key and the door every pair has a path, and where both have a number it is the same"""
    import hostemu_goal as HG
    emu, grid, kinds, want = SC.emu_batch(name, 512, 0)
    static, _ = HG.run(emu._cfg(), emu.state, "general", 64, field=False)
    free, goal = G.classify(grid, *G.kinds_of(emu.env))
    ref_static = G.agents_from_field(G.field_levels(free, goal), *G.unpack_records(emu.rec))
    assert np.array_equal(static, ref_static)
    assert (want[0] > 0).all() and want[0].size == 1024
    assert ((static < 0).sum(), want[0].max()) == (blind, longest)
    assert np.array_equal(want[0][static >= 0], static[static >= 0])


def test_without_doors_and_items_it_is_goal_distance():
    import hostemu_goal as HG
    import hostemu_solve as HS
    emu, grid, kinds, want = SC.emu_batch(SC.S15, 512, 0)
    static, _ = HG.run(emu._cfg(), emu.state, "general", 64, field=False)
    dist, act, exact = HS.run(emu._cfg(), emu.state, 64)
    assert np.array_equal(dist, static) and exact.all() and (static < 0).any() and (static > 0).any()
    assert ((act == S.DONE) == (dist < 0)).all()


def test_env_mask_leaves_unselected_rows_alone():
    emu, grid, kinds, want = SC.emu_batch(SC.DK8, 512, 30)
    _check(emu._cfg(), emu.state, want, mask=(np.arange(512) % 3 == 1))


# ---- grids made by hand ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hand():
    return SC.hand_cases()


def test_hand_cases_match_the_reference(hand):
    for name, (case, caps, want) in hand.items():
        _check(case.cfg, case.state, want, caps)


def test_hand_cases_say_what_they_are_meant_to(hand):
    d = {name: want[0][0].tolist() for name, (_, _, want) in hand.items()}
    a = {name: want[1][0].tolist() for name, (_, _, want) in hand.items()}
    exact = {name: bool(want[2][0]) for name, (_, _, want) in hand.items()}
    # 6 to stand behind A (turn, forward, turn, toggle, 2 forward), 7 to take the key, 8 back through the open A, 4 to the locked
    # door, 2 toggles, 2 forward
    assert d["door_passed_twice"][0] == 29 and a["door_passed_twice"][0] == S.LEFT
    assert (np.array(d["door_passed_twice"]) > 0).all()
    assert d["two_locked_in_series"] == [-1, -1, 4] and a["two_locked_in_series"] == [S.DONE, S.DONE, S.TOGGLE]
    assert d["ball_plugs_corridor"] == [5, -1] and a["ball_plugs_corridor"] == [S.FORWARD, S.DONE]
    assert d["carries"][:3] == [5, -1, -1] and d["carries"][3] > 5 and d["carries"][4] == -1
    assert a["carries"][0] == S.TOGGLE
    assert d["doors_that_do_not_open"] == [-1, -1]
    assert d["open_door_and_agents_in_no_cell"] == [3, -1, -1, -1, -1, 4]
    assert d["door_is_a_shortcut"][0] == 3 and a["door_is_a_shortcut"][0] == S.TOGGLE
    assert exact["caps_exceeded_uncapped"] and not exact["caps_exceeded"]
    assert d["caps_exceeded_uncapped"][0] == 3 and d["caps_exceeded"][0] > 3 and d["caps_exceeded"][1] == d["caps_exceeded_uncapped"][1]
    assert not exact["items_beyond_the_cap"] and d["items_beyond_the_cap"] == [-1]
    assert exact["items_within_the_cap"] and d["items_within_the_cap"][0] > 0


def test_the_shortcut_beats_goal_distance(hand):
    import hostemu_goal as HG
    case, _, want = hand["door_is_a_shortcut"]
    static, _ = HG.run(case.cfg, case.state, "general", 64, field=False)
    assert (static > 0).all() and want[0][0, 0] < static[0, 0]


@pytest.mark.parametrize("name", SC.EDGE_SHAPES)
def test_edge_shapes(name):
    case, caps, want = SC.edge(name)
    assert (want[0] > 0).any()
    if name in ("H65", "H129"):
        assert want[0][0, 0] == 13 and case.cfg.H == int(name[1:])
    if name == "lanes_64":
        assert 4 * case.cfg.W == 64
    if name == "more_agents_than_planes":
        assert case.cfg.n_agents == 32 > 4 * case.cfg.W
    _check(case.cfg, case.state, want, caps)


# ---- the launcher's arithmetic ----------------------------------------------------------------------------------------------------
def test_lds_arithmetic_and_refusals():
    import hostemu_solve as HS
    L = HS.lib()
    assert L.sd_scratch_bytes(15, 15, 2, 2) == 8 * 15 * (2 + 12 * 12) + 1024 <= 64 * 1024
    assert L.sd_scratch_bytes(15, 15, 4, 3) == 8 * 15 * (2 + 12 * 64) + 1024 <= 160 * 1024
    assert L.sd_scratch_bytes(255, 255, 0, 0) == 8 * 255 * 4 * 14 + 1024 <= 160 * 1024
    assert min(L.sd_scratch_bytes(255, 255, 1, 0), L.sd_scratch_bytes(255, 255, 0, 1)) > 160 * 1024
    g = np.ones((1, 255, 255), np.uint8)
    g[0, 1:254, 1:254] = 0
    g[0, 200, 200] = HS.SolveCase.GOAL
    case = HS.SolveCase(g, [[(199, 200, 0, SC.IN_CELL, 0)]])
    dist, act, exact = HS.run(case.cfg, case.state, 64, max_doors=0, max_items=0)
    assert dist.tolist() == [[1]] and act.tolist() == [[2]] and exact.tolist() == [1]
    for caps in ((1, 0), (0, 1), (2, 2)):
        dist, act, exact = HS.run(case.cfg, case.state, 64, max_doors=caps[0], max_items=caps[1], rc_want=N.E_UNSUPPORTED)
        assert (dist == -7).all() and (act == -7).all() and (exact == 0xF9).all()       # nothing is written
    for caps in ((5, 0), (0, 4), (-1, 0), (0, -1)):
        HS.run(case.cfg, case.state, 64, max_doors=caps[0], max_items=caps[1], rc_want=N.E_ARG)


# ---- following the policy ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", SC.FOLLOW)
def test_following_the_policy_pays_what_optimal_return_says(M):
    """MarlGrid-1AgentDoorKey8x8-v0, 512 envs: every step the analysis again and its first action.  While an env runs its
    distance is the previous one minus 1; the agent is done at exactly step d with exactly optimal_return's return; where
    step_count + d > max_steps nothing is earned."""
    import hostemu
    import hostemu_solve as HS
    from marlgrid_amd import envs as E
    B = 512
    assert SC.SOLO8 in E.solo_envs and SC.SOLO8 not in E._registry
    E._registry[SC.SOLO8] = E._solo_registry[SC.SOLO8]       # (HostEmu builds what `_registry` names; the pinned tests list it)
    try:
        emu = hostemu.HostEmu(SC.SOLO8, B, 1337 + np.arange(B), max_steps=M)
    finally:
        del E._registry[SC.SOLO8]
    emu.reset()
    dist, act, exact = HS.run(emu._cfg(), emu.state, 64)
    d0 = dist[:, 0].astype(np.int64)
    assert (d0 > 0).all() and exact.all() and emu.env.reward_decay and emu.env.max_steps == M
    pays, want = SC.follow_expectation(d0, np.zeros(B, np.int64), M)
    assert pays.any() and (M >= 40 or (~pays).any())
    if M < 40:      # the truncation rule is met on both sides
        assert (d0 == M).any() and (d0 == M + 1).any()
    used = set()
    done_at = np.full(B, -1, np.int64)
    got = np.zeros(B)
    over = np.zeros(B, bool)
    for t in range(1, M + 1):
        dist, act, _ = HS.run(emu._cfg(), emu.state, 64)
        run = ~over
        assert np.array_equal(dist[run, 0], d0[run] - (t - 1)), t
        used |= set(act[run, 0].tolist())
        rew, done = emu.step(act.astype(np.int64))
        got += np.where(over, 0.0, rew[:, 0].astype(np.float64))
        newly = ((G.unpack_records(emu.rec)[2][:, 0] & N.AF_DONE) != 0) & (done_at < 0) & ~over
        done_at = np.where(newly, t, done_at)
        over |= done
    assert over.all()
    assert np.array_equal(done_at[pays], d0[pays])
    assert np.abs(got[pays] - want[pays]).max() <= SC.REW_TOL
    assert (done_at[~pays] < 0).all() and (got[~pays] == 0).all()
    if M >= 40:
        assert used == {0, 1, 2, 3, 5}
