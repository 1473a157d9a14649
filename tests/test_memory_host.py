"""CPU tests of the memory maps: the bodies of mg_memory_update (marlgrid_amd/csrc/mg_explore_core.h with mg_view_triple.h — the
one definition of the hide rules, which mg_encode_views runs too —, mg_occlude.h's shadow cast and mg_core.h's view map) built
with g++ (tests/native/hostemu_memory.py) over HostEmu states, against tests/memory_ref.py — the oracle's post-hide top codes and
vis masks through the reference's crop-and-rotate — on the GPU test's scenario table (tests/memory_cases.py) at 16 to 64 envs
for at most 40 steps.  All six tensors are compared, exactly, after reset() and after every step, with the invariants between
them; beside the kernel's shape (256-lane workgroups, 64-lane waves) every case is emulated with 64-lane and one-lane workgroups
and with the run-time-view instantiation, which must give the same bytes, and mg_explore_update runs beside them on maps of its
own, whose four tensors must be the same."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "native"))

import memory_cases as MC  # noqa: E402
import test_explore_host as TXH  # noqa: E402

SHAPES = ((64, 64, False), (1, 7, False), (256, 64, True))      # (workgroup lanes, lanes that clear a plane, run-time view)
STEPS = 40


class HostSubject(TXH.HostSubject):
    def __init__(self, case, B, shapes=SHAPES):
        import hostemu_memory as HM
        self.emu = TXH.make_emu(case, B)
        self.drv = HM.Driver(self.emu, shapes)
        self.W, self.H, self.n = self.emu.env.width, self.emu.env.height, self.emu.n


def _batch(key):
    return 16 + 12 * (sorted(MC.TABLE).index(key) % 5)      # 16 .. 64


@pytest.mark.parametrize("key", [k for k in MC.TABLE if k not in ("manual_reset", "next_step")])
def test_the_scenario_table_matches_the_reference(key):
    case = MC.Case(key)
    B = _batch(key)
    sub = HostSubject(case, B)
    ref = MC.run(case, sub, B, steps=min(STEPS, case.steps))
    assert ref.ref.memory.any() and (ref.ref.seen_step > 0).any()
    if key == "headline":       # every env has begun a second episode, and cleared
        assert sub.emu.step_count.max() <= 7 and ref.ref.stats["clears"] >= B
    if key == "two_groups":
        assert len(sub.emu.env._groups) == 2 and len(sub.drv.pb) == 2


def test_a_reset_by_hand_leaves_the_other_envs_alone():
    case = MC.Case("manual_reset")
    B = 33
    sub = HostSubject(case, B)
    resets = []

    def after(t, done, ref):
        if not done.any():
            return False
        before = {k: v.copy() for k, v in sub.tensors().items()}
        sub.reset(done)
        ref.reset(done)
        now = sub.tensors()
        for k in MC.KEYS:
            assert np.array_equal(now[k][~done], before[k][~done]), (t, k)
        assert (now["seen_step"][done] <= 0).all()
        resets.append(int(done.sum()))
        return True
    MC.run(case, sub, B, after_step=after)
    assert resets and sum(resets) >= B


def test_next_step_reset_remembers_the_terminal_step_and_clears_in_the_reset_call():
    case = MC.Case("next_step")
    B = 33
    sub = HostSubject(case, B)
    seen_resets = []

    def after(t, done, ref):
        stamp = sub.tensors()["seen_step"]
        fresh = (stamp <= 0).all(axis=(1, 2, 3))
        assert np.array_equal(fresh, ref.was_reset), t
        seen_resets.append(int(fresh.sum()))
        return False
    MC.run(case, sub, B, after_step=after)
    assert sum(seen_resets) >= 3 * B


def test_a_launch_writes_only_its_own_agents_rows_and_selected_envs():
    """two view groups, sentinel-filled tensors: the launch of group 0 leaves agent 1's rows alone, and a masked one the
    unselected envs"""
    import hostemu_memory as HM
    case = MC.Case("two_groups")
    B = 19
    sub = HostSubject(case, B, shapes=())
    sub.reset()
    assert [g.members for g in sub.emu.env._groups] == [[0, 2], [1]]
    maps = HM.Maps(B, sub.n, sub.W, sub.H, fill=0x5A)
    mask = np.arange(B) % 3 != 0
    HM.update(sub.emu, maps, mask=mask, groups=[0])
    want = sub.tensors()
    for k in MC.KEYS:
        t = getattr(maps, k)
        sentinel = np.asarray(0x5A, t.dtype)
        assert (t[:, 1] == sentinel).all() and (t[~mask] == sentinel).all(), k
        got = t[mask][:, [0, 2]]
        assert np.array_equal(got.astype(bool) if k == "seen" else got, want[k][mask][:, [0, 2]]), k


def test_clearing_writes_the_pairs_planes_and_nothing_beyond():
    """odd plane sizes, a masked launch on sentinel-filled tensors with guard rows before and after: the selected envs (fresh:
    their step count is 0) come out as a cleared plane plus one observation — memory 0 and seen_step -1 where nothing was seen
    —, the unselected envs and the guards keep the sentinel"""
    import hostemu_memory as HM
    case = MC.Case("geo_9x6")
    B = 7
    sub = HostSubject(case, B, shapes=())
    sub.reset()
    assert (sub.W * sub.H) % 4 != 0 and (sub.emu.step_count == 0).all()
    want = sub.tensors()
    assert (want["seen_step"] == -1).any() and (want["seen_step"] == 0).any()
    mask = np.arange(B) % 2 == 0
    for lanes in (64, 1, 5):
        big = HM.Maps(B + 2, sub.n, sub.W, sub.H, fill=0x5A)
        maps = HM.Maps.__new__(HM.Maps)
        for k in MC.KEYS:
            setattr(maps, k, getattr(big, k)[1:-1])      # (views: rows 0 and B + 1 are the guards)
        HM.update(sub.emu, maps, mask=mask, wave=lanes)
        for k in MC.KEYS:
            t, g = getattr(maps, k), getattr(big, k)
            sentinel = np.asarray(0x5A, t.dtype)
            assert (g[0] == sentinel).all() and (g[-1] == sentinel).all() and (t[~mask] == sentinel).all(), (lanes, k)
            assert np.array_equal(t[mask].astype(bool) if k == "seen" else t[mask], want[k][mask]), (lanes, k)


def test_the_scratch_grows_by_the_two_tables_and_the_halving_rule_stays():
    import hostemu_explore as HX
    import hostemu_memory as HM
    sub = HostSubject(MC.Case("geo_v8"), 16, shapes=())
    sub.reset()
    maps = HM.Maps(16, sub.n, sub.W, sub.H)
    (pb, lds), = HM.update(sub.emu, maps)
    pb0, = HX.update(sub.emu, HX.Maps(16, sub.n, sub.W, sub.H))
    env_cap = (pb - 1) // sub.n + 2
    assert pb == pb0 == 256 and lds == 256 + env_cap * sub.n * 8 + pb * 8 + pb * 8 * 4 * 2 + 2048 <= 48 * 1024
