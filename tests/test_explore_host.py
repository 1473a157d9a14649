"""CPU tests of the exploration maps: the bodies of mg_explore_update (marlgrid_amd/csrc/mg_explore_core.h, with mg_occlude.h's
shadow cast and mg_core.h's view map) built with g++ (tests/native/hostemu_explore.py) over HostEmu states, against
tests/explore_ref.py — the oracle's own vis masks through the reference's crop-and-rotate — on the GPU test's scenario table
(tests/explore_cases.py) at 16 to 64 envs for 40 steps.  The four tensors are compared, exactly, after reset() and after every
step; beside the kernel's shape (256-lane workgroups, 64-lane waves) every case is emulated with 64-lane and one-lane workgroups
and with the run-time-view instantiation, which must give the same bytes."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "native"))

import explore_cases as XC  # noqa: E402
import product_envs  # noqa: E402
from marlgrid_amd import _native as N  # noqa: E402

SHAPES = ((64, 64, False), (1, 7, False), (256, 64, True))      # (workgroup lanes, lanes that clear a plane, run-time view)
STEPS = 40


def make_emu(case, B):
    """the HostEmu (EpisodeEmu for next-step reset) of a case; a case that is no registered id builds its env itself"""
    import hostemu
    import hostemu_episode
    name = case.c.get("name", case.key)
    orig = product_envs.build
    if "name" not in case.c:
        product_envs.build = lambda _name, **kw: case.build(**kw)
    try:
        kw = dict(case.kw) if "name" in case.c else {}
        if case.mode == "next_step":
            return hostemu_episode.EpisodeEmu(name, B, case.seeds(B), mode="next_step", **kw)
        return hostemu.HostEmu(name, B, case.seeds(B), auto_reset=case.mode == "same_step", **kw)
    finally:
        product_envs.build = orig


class HostSubject(object):
    def __init__(self, case, B, shapes=SHAPES):
        import hostemu_explore as HX
        self.emu = make_emu(case, B)
        self.drv = HX.Driver(self.emu, shapes)
        self.W, self.H, self.n = self.emu.env.width, self.emu.env.height, self.emu.n

    def reset(self, mask=None):
        self.drv.reset(mask)

    def step(self, a):
        return self.drv.step(a)[1]

    def tensors(self):
        return self.drv.tensors()

    def place(self, k, x, y, d):
        """MultiGridEnv.set_agent on the emu's records: position, heading, and the highest arrival rank"""
        rec = self.emu.rec
        rk = (rec >> np.uint64(8 * N.AG_RANK)) & np.uint64(0xFF)
        old = rk[:, k:k + 1]
        rk = np.where(rk > old, rk - np.uint64(1), rk)
        rk[:, k] = self.n - 1
        rec[...] = (rec & ~np.uint64(0xFF << (8 * N.AG_RANK))) | (rk << np.uint64(8 * N.AG_RANK))
        col = rec[:, k]
        for i, v in ((N.AG_X, x), (N.AG_Y, y), (N.AG_DIR, d)):
            col = (col & ~np.uint64(0xFF << (8 * i))) | np.uint64(int(v) << (8 * i))
        rec[:, k] = col


def _batch(key):
    return 16 + 12 * (sorted(XC.TABLE).index(key) % 5)      # 16 .. 64


@pytest.mark.parametrize("key", [k for k in XC.TABLE if k not in ("manual_reset", "next_step")])
def test_the_scenario_table_matches_the_reference(key):
    case = XC.Case(key)
    B = _batch(key)
    sub = HostSubject(case, B)
    ref = XC.run(case, sub, B, steps=min(STEPS, case.steps))
    assert ref.ref.seen.any() and ref.ref.visits.any()
    if key == "headline":       # every env has begun a second episode, and cleared
        assert sub.emu.step_count.max() <= 7
    if key == "two_groups":
        assert len(sub.emu.env._groups) == 2 and len(sub.drv.pb) == 2


def test_a_reset_by_hand_leaves_the_other_envs_alone():
    """auto_reset=False with reset(env_mask=done): the unselected envs' visits are not counted twice"""
    case = XC.Case("manual_reset")
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
        for k in XC.KEYS:
            assert np.array_equal(now[k][~done], before[k][~done]), (t, k)
        assert (now["visits"][done].reshape(int(done.sum()), sub.n, -1).sum(axis=2) <= 1).all()
        resets.append(int(done.sum()))
        return True
    XC.run(case, sub, B, after_step=after)
    assert resets and sum(resets) >= B


def test_next_step_reset_accumulates_the_terminal_step_and_clears_in_the_reset_call():
    case = XC.Case("next_step")
    B = 33
    sub = HostSubject(case, B)
    seen_resets = []

    def after(t, done, ref):
        t_ = sub.tensors()
        fresh = (t_["new_cells"] == t_["seen"].reshape(B, sub.n, -1).sum(axis=2)).all(axis=1)
        assert np.array_equal(fresh, ref.was_reset), t
        assert np.array_equal(sub.emu.out_flags & N.EPF_RESET != 0, ref.was_reset), t
        seen_resets.append(int(fresh.sum()))
        return False
    XC.run(case, sub, B, after_step=after)
    assert sum(seen_resets) >= 3 * B


def test_a_launch_writes_only_its_own_agents_rows_and_selected_envs():
    """two view groups, sentinel-filled tensors: the launch of group 0 leaves agent 1's rows alone, and a masked one the
    unselected envs"""
    import hostemu_explore as HX
    case = XC.Case("two_groups")
    B = 19
    sub = HostSubject(case, B, shapes=())
    sub.reset()
    groups = sub.emu.env._groups
    assert [g.members for g in groups] == [[0, 2], [1]]
    maps = HX.Maps(B, sub.n, sub.W, sub.H, fill=0x5A)
    mask = np.arange(B) % 3 != 0
    HX.update(sub.emu, maps, mask=mask, groups=[0])
    want = sub.tensors()
    for k, t in (("seen", maps.seen), ("visits", maps.visits), ("new_cells", maps.new_cells), ("visit_count", maps.visit_count)):
        sentinel = np.asarray(0x5A, t.dtype)
        assert (t[:, 1] == sentinel).all() and (t[~mask] == sentinel).all(), k
        got = t[mask][:, [0, 2]]
        assert np.array_equal(got.astype(bool) if k == "seen" else got, want[k][mask][:, [0, 2]]), k


def test_the_planes_are_cleared_whatever_their_alignment():
    """explore_clear_planes: odd plane sizes put the planes of a batch at every byte phase; the neighbours' bytes stay"""
    import hostemu_explore as HX
    case = XC.Case("geo_9x6")
    B = 7
    sub = HostSubject(case, B, shapes=())
    sub.reset()
    assert (sub.W * sub.H) % 4 != 0
    maps = HX.Maps(B, sub.n, sub.W, sub.H, fill=0x5A)
    mask = np.arange(B) % 2 == 0
    for lanes in (64, 1, 5):
        maps.seen[...] = 0x5A
        maps.visits[...] = 0x5A
        HX.update(sub.emu, maps, mask=mask, wave=lanes)
        assert np.array_equal(maps.seen[mask].astype(bool), sub.tensors()["seen"][mask]) and (maps.seen[mask] <= 1).all()
        assert (maps.seen[~mask] == 0x5A).all() and (maps.visits[~mask] == 0x5A).all()
        assert np.array_equal(maps.visits[mask], sub.tensors()["visits"][mask])
