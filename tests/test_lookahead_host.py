"""CPU tests of lookahead: the bodies of mg_fork_rows and mg_rollout (marlgrid_amd/csrc/mg_lookahead_core.h) built with g++
(tests/native/hostemu_lookahead.py) over a HostEmu's numpy state, against the oracle: a fresh oracle env per (env, plan), replayed
through the same prefix and stepped through the plan with the freeze rule applied on the test's side (tests/lookahead_cases.py,
which tests/test_hip_lookahead.py shares).  done exactly, rewards within 1e-6, the state every row was left in and its
generator; the source state bit-identical before and after; the coverage conditions on the oracle's side."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "native"))

import lookahead_cases as LC  # noqa: E402
from marlgrid_amd import _native as N  # noqa: E402


def _shadow_state(emu, sh):
    W, H = emu.env.width, emu.env.height
    return dict(grid=sh.grid[:, :W * H].reshape(sh.R, W, H), rec=sh.rec, step_count=sh.step_count, mt=sh.mt, mt_pos=sh.mt_pos,
                mt_head=sh.mt_head)


def _unchanged(emu, snap):
    import hostemu_lookahead as HL
    for k in HL.STATE_ARRAYS:
        assert np.array_equal(getattr(emu, k), snap[k]), "the source's %s changed" % k


def _look(emu, K, plans, ids=None, S=64, lanes=64):
    import hostemu_lookahead as HL
    m = emu.B if ids is None else len(ids)
    sh = HL.Shadow(emu, K * m)
    HL.fork(emu, sh, K, ids, lanes)
    return (sh,) + HL.rollout(emu, sh, plans, m, S)


@pytest.mark.parametrize("key", LC.ORACLE_CASES)
def test_plans_match_the_oracle(key):
    import hostemu_lookahead as HL
    cs = LC.case(key)
    emu = cs.emu()
    snap = HL.snapshot(emu)
    plans = cs.plans(emu.n)
    sh, rew, done, err = _look(emu, cs.K, plans)
    _unchanged(emu, snap)
    assert not err.any() and not emu.error.any()
    want = LC.Want(cs)
    want.coverage(cs)
    LC.compare(want, rew, done, _shadow_state(emu, sh), emu.env.scenario_spec(), key)
    if key == "prestige":       # the shadow's own prestige_t went through the plan
        assert emu._cfg().prestige_mask and np.abs(sh.prestige - np.stack([e.prestige() for e in want.envs])).max() <= 1e-12
    # the workgroup shapes and the one-lane fork give the same bytes
    for S, lanes in ((256, 1), (1, 7)):
        sh2, rew2, done2, _ = _look(emu, cs.K, plans, S=S, lanes=lanes)
        assert rew2.tobytes() == rew.tobytes() and np.array_equal(done2, done)
        for k in HL.STATE_ARRAYS:
            assert np.array_equal(getattr(sh2, k), getattr(sh, k)), (S, lanes, k)


def test_the_truncated_case_freezes_and_pays_nothing_afterwards():
    cs = LC.case("truncated")
    emu = cs.emu()
    _, rew, done, _ = _look(emu, cs.K, cs.plans(emu.n))
    first = done.argmax(axis=1)                      # (K, m): every row ends, at step 7 at the latest
    assert done.any(axis=1).all() and first.max() == 6 and first.min() < 6
    for p in range(cs.K):
        for j in range(cs.B):
            assert done[p, first[p, j]:, j].all() and not rew[p, first[p, j] + 1:, j].any()


def test_an_ended_episode_is_frozen_from_the_first_row():
    """after the 7 steps of the time limit every env has ended: the lookahead steps nothing and leaves the copies as they are"""
    import hostemu_lookahead as HL
    cs = LC.case("truncated")
    emu = cs.emu()
    for t in range(7):
        emu.step(cs.plans(emu.n)[1, t])
    assert emu.done.all()
    snap = HL.snapshot(emu)
    sh, rew, done, err = _look(emu, 2, cs.plans(emu.n)[:2])
    assert done.all() and not rew.any() and not err.any()
    _unchanged(emu, snap)
    for k in HL.STATE_ARRAYS:
        if k not in ("error", "prestige"):      # (the row's error is the rollout's own; no 'prestige' agent here: not copied)
            assert np.array_equal(getattr(sh, k), np.concatenate([snap[k]] * 2)), k


def test_env_ids_pick_rows_and_an_id_outside_the_batch_is_inert():
    cs = LC.case("wide_k3")
    emu = cs.emu()
    plans = cs.plans(emu.n)
    _, rew_all, done_all, _ = _look(emu, cs.K, plans)
    ids = np.array([66, 3, 200, 3, -1, 0], np.int64)
    ok = (ids >= 0) & (ids < cs.B)
    sub = np.ascontiguousarray(plans[:, :, np.where(ok, ids, 0)])
    sh, rew, done, err = _look(emu, cs.K, sub, ids=ids)
    assert np.array_equal(rew[:, :, ok].view(np.uint32), rew_all[:, :, ids[ok]].view(np.uint32))
    assert np.array_equal(done[:, :, ok], done_all[:, :, ids[ok]])
    assert done[:, :, ~ok].all() and not rew[:, :, ~ok].any() and not err.any()
    inert = np.nonzero(np.tile(~ok, cs.K))[0]
    assert (sh.step_count[inert] == 2 ** 31 - 1).all() and not sh.grid[inert].any() and not sh.mt[inert].any()


def test_an_unknown_action_is_recorded_in_the_row_and_nowhere_else():
    import hostemu_lookahead as HL
    cs = LC.case("wide_k3")
    emu = cs.emu()
    emu.error[5] = N.ERR_RECURSION                  # an error the env itself carries: not the plan's
    snap = HL.snapshot(emu)
    plans = cs.plans(emu.n).copy()
    plans[1, 2, 40, 1] = 9
    plans[2, 0, 7, 0] = -3
    for dtype in (np.int64, np.int32):
        sh, rew, done, err = _look(emu, cs.K, plans.astype(dtype))
        want = np.zeros((cs.K, cs.B), np.int32)
        want[1, 40] = want[2, 7] = N.ERR_VALUE
        assert np.array_equal(err, want)
        _unchanged(emu, snap)
    _, rew8, done8, _ = _look(emu, cs.K, cs.plans(emu.n).astype(np.uint8))
    _, rew64, done64, _ = _look(emu, cs.K, cs.plans(emu.n))
    assert rew8.tobytes() == rew64.tobytes() and np.array_equal(done8, done64)


@pytest.mark.parametrize("stride, offset", [(80, 0), (77, 0), (77, 3), (16, 8), (5, 1)])
def test_fork_copies_grid_slices_of_any_stride_and_alignment(stride, offset):
    """the vector path needs both slices 16-byte aligned; everything else goes as bytes — to a destination that scatters"""
    import hostemu_lookahead as HL
    B, n, R = 5, 2, 6
    r = np.random.RandomState(stride * 16 + offset)

    def state(rows, fill):
        a = dict(grid=np.full(rows * stride + 32, fill, np.uint8), rec=np.full((rows, n), fill, np.uint64),
                 mt=np.full((rows, N.MT_N), fill, np.uint32), mt_pos=np.full(rows, fill, np.int32),
                 mt_head=np.full((rows, N.MT_HEAD), fill, np.uint32), step_count=np.full(rows, fill, np.int32),
                 done=np.full(rows, fill, np.uint8), error=np.full(rows, fill, np.int32))
        base = a["grid"].ctypes.data
        skew = (-base) % 16 + offset
        st = N.State(base + skew, a["rec"].ctypes.data, a["mt"].ctypes.data, a["mt_pos"].ctypes.data, a["step_count"].ctypes.data,
                     a["done"].ctypes.data, a["error"].ctypes.data, None, a["mt_head"].ctypes.data, None)
        return a, st, skew

    src, s_st, s_skew = state(B, 0)
    for k, v in src.items():
        v[...] = r.randint(0, 250, v.shape).astype(v.dtype)
    dst, d_st, d_skew = state(R + 2, 0xEE)
    cfg = N.Config()
    cfg.B, cfg.n_agents, cfg.cells_stride = B, n, stride
    src_of = np.array([4, 0, 9], np.int64)           # m = 3, K = 2: rows 0..5 <- 4, 0, inert, 4, 0, inert
    dst_of = np.array([7, 1, 0, 3, 99, 5], np.int64)  # row 4 has no destination; rows 2, 4 and 6 of dst stay as they are
    rc = HL.lib().la_fork(C.byref(cfg), C.byref(s_st), C.byref(d_st), src_of.ctypes.data, dst_of.ctypes.data, R + 2, R, 3, 64)
    assert rc == 0
    sg = src["grid"][s_skew:s_skew + B * stride].reshape(B, stride)
    dg = dst["grid"][d_skew:d_skew + (R + 2) * stride].reshape(R + 2, stride)
    assert (dst["grid"][:d_skew] == 0xEE).all() and (dst["grid"][d_skew + (R + 2) * stride:] == 0xEE).all()
    for row, s in ((7, 4), (1, 0), (3, 4)):
        assert np.array_equal(dg[row], sg[s])
        for k in ("rec", "mt", "mt_pos", "mt_head", "step_count", "done", "error"):
            assert np.array_equal(dst[k][row], src[k][s]), k
    for row in (0, 5):                              # inert
        assert not dg[row].any() and not dst["mt"][row].any() and dst["step_count"][row] == 2 ** 31 - 1 and dst["done"][row] == 1
        assert dst["error"][row] == 0 and (dst["rec"][row] == (N.AF_DONE << (8 * N.AG_FLAGS))).all()
    for row in (2, 4, 6):
        assert (dg[row] == 0xEE).all() and (dst["mt"][row] == 0xEE).all() and dst["done"][row] == 0xEE


def test_the_row_footprint_the_readme_states():
    from marlgrid_amd import lookahead as LA
    assert LA.row_bytes(240, 3) == 240 + 8 * 3 + 2496 + 64 + 4 + 4 + 1 + 4 == 2837
    assert LA.row_bytes(96, 3, prestige=True) == LA.row_bytes(96, 3) + 8 * 3
    assert {"mg_fork_rows", "mg_rollout"} <= set(N.SYMBOLS) and N.ABI_VERSION == 6


def test_shards_refuse_a_fork_across_shards_before_any_env_is_touched():
    from marlgrid_amd import sharding as S
    sh = object.__new__(S._Shards)
    sh.ranges, sh.envs = [(0, 8), (8, 16)], []
    with pytest.raises(NotImplementedError, match="shard"):
        sh.fork([1, 9], [2, 3])                     # env 9 lives on shard 1, env 3 on shard 0
    with pytest.raises(ValueError):
        sh.fork([1, 2], [3, 3])
    with pytest.raises(ValueError):
        sh.fork([1, 16], [3, 4])
    sh.fork([1, 9], [2, 15])                        # (within the shards: passed on — to no env here)
