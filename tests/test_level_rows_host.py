"""Levels that carry their parameters and edits, without a GPU: the body of mg_level_apply_rows (marlgrid_amd/csrc/
mg_level_core.h, the text level_apply_rows_kernel runs) built with g++ (tests/native/mg_level_rows.cpp) over numpy arrays.
B = 67 envs, L = 5 slots, K = 7 edit entries (a row of 28 bytes); a guard band behind every table."""
import ctypes as C
import fcntl
import os
import subprocess

import numpy as np
import pytest

from marlgrid_amd import _native as N

HERE = os.path.dirname(os.path.abspath(__file__))
NATIVE = os.path.join(HERE, "native")
CSRC = os.path.join(os.path.dirname(HERE), "marlgrid_amd", "csrc")
vp = C.c_void_p
B, L, K, N_AGENTS, MAX_STEPS = 67, 5, 7, 2, 10
GUARD = 64


def _p(a):
    return None if a is None else vp(a.ctypes.data)


@pytest.fixture(scope="module")
def lvr():
    out = os.path.join(NATIVE, "libmg_level_rows.so")
    with open(os.path.join(NATIVE, ".build.lock"), "w") as lock:        # (one builder at a time, as tests/native/hostemu.py)
        fcntl.flock(lock, fcntl.LOCK_EX)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Wno-unused-function",
                               "-Wno-unknown-pragmas", "-I", os.path.join(os.path.dirname(HERE), "include"), "-I", CSRC,
                               os.path.join(NATIVE, "mg_level_rows.cpp"), "-o", out])
    lib = C.CDLL(out)
    lib.lvr_seed.argtypes = [C.c_int, vp, C.c_int, vp, vp, vp, vp]
    lib.lvr_seed.restype = None
    lib.lvr_apply_rows.argtypes = [C.POINTER(N.Config), C.POINTER(N.State), C.c_int, vp, vp, C.c_int, vp, vp, vp, vp, vp, vp,
                                   vp, vp, C.c_int, vp, vp, C.c_int]
    lib.lvr_apply_rows.restype = None
    return lib


def _guarded(shape, rng):
    """a table of random bytes with a 0xA5 band behind it: (the whole buffer, the table's view)"""
    n = int(np.prod(shape))
    buf = np.full(n + GUARD, 0xA5, np.uint8)
    buf[:n] = rng.randint(0, 256, n)
    return buf, buf[:n].reshape(shape)


class World(object):
    def __init__(self, lvr, seed=3):
        rng = np.random.RandomState(seed)
        self.lvr = lvr
        self.cfg = N.Config()
        self.cfg.B, self.cfg.n_agents, self.cfg.max_steps = B, N_AGENTS, MAX_STEPS
        self.rec = np.zeros((B, N_AGENTS), np.uint64)
        self.mt = rng.randint(0, 2 ** 32, (B, N.MT_N), dtype=np.int64).astype(np.uint32)
        self.mt_pos = rng.randint(0, 600, B).astype(np.int32)
        self.mt_head = rng.randint(0, 2 ** 32, (B, N.MT_HEAD), dtype=np.int64).astype(np.uint32)
        self.step_count = np.zeros(B, np.int32)
        self.st = N.State()
        self.st.agents, self.st.mt, self.st.mt_pos = self.rec.ctypes.data, self.mt.ctypes.data, self.mt_pos.ctypes.data
        self.st.step_count, self.st.mt_head = self.step_count.ctypes.data, self.mt_head.ctypes.data
        self.bank_mt = np.zeros((L, N.MT_N), np.uint32)
        self.bank_pos = np.zeros(L, np.int32)
        self.bank_head = np.zeros((L, N.MT_HEAD), np.uint32)
        self.bank_seed = np.full(L, -1, np.int64)
        seeds = np.array([11, 22, -1, 44, 55], np.int64)                  # slot 2 is empty
        lvr.lvr_seed(L, _p(seeds), L, _p(self.bank_mt), _p(self.bank_pos), _p(self.bank_head), _p(self.bank_seed))
        self._bp, self.bank_params = _guarded((L, N.GEN_DRAWS), rng)
        self._be, self.bank_edits = _guarded((L, K, 4), rng)
        self._ep, self.env_params = _guarded((B, N.GEN_DRAWS), rng)
        self._ee, self.env_edits = _guarded((B, K, 4), rng)
        self.episode_level = np.full(B, -7, np.int64)
        self.out_level = np.full(B, -9, np.int64)
        # envs 0 .. B-1 over the slots, with shared slots, a free-running one (-1), the empty slot and one outside the bank
        self.level_of_env = (np.arange(B) % (L + 2) - 1).astype(np.int64)

    def apply(self, rule, mask, params=True, edits=True, lanes=64):
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        self.lvr.lvr_apply_rows(C.byref(self.cfg), C.byref(self.st), rule, _p(m), _p(self.level_of_env), L, _p(self.bank_mt),
                                _p(self.bank_pos), _p(self.bank_head), _p(self.bank_seed), _p(self.episode_level), _p(self.out_level),
                                _p(self.bank_params) if params else None, _p(self.bank_edits) if edits else None, K if edits else 0,
                                _p(self.env_params) if params else None, _p(self.env_edits) if edits else None, lanes)

    def snapshot(self):
        return {k: getattr(self, k).copy() for k in ("mt", "mt_pos", "mt_head", "env_params", "env_edits")}

    def guards_intact(self):
        return all((b[-GUARD:] == 0xA5).all() for b in (self._bp, self._be, self._ep, self._ee))


def _takes(w, selected):
    lv = w.level_of_env
    ok = (lv >= 0) & (lv < L)
    return selected & ok & (w.bank_seed[np.clip(lv, 0, L - 1)] >= 0)


@pytest.mark.parametrize("lanes", [64, 1])
def test_selected_envs_with_a_slot_take_generator_parameters_and_edits(lvr, lanes):
    w = World(lvr)
    before = w.snapshot()
    bank = (w.bank_params.copy(), w.bank_edits.copy(), w.bank_mt.copy())
    mask = np.arange(B) % 3 != 1                                          # unselected envs in between
    takes = _takes(w, mask)
    assert takes.sum() > 20 and (mask & ~takes).sum() > 10 and (~mask).sum() > 20
    w.apply(N.LEVEL_MASK, mask, lanes=lanes)
    lv = w.level_of_env
    for b in range(B):
        if takes[b]:
            assert np.array_equal(w.mt[b], w.bank_mt[lv[b]]) and np.array_equal(w.mt_head[b], w.bank_head[lv[b]]), b
            assert w.mt_pos[b] == w.bank_pos[lv[b]], b
            assert np.array_equal(w.env_params[b], w.bank_params[lv[b]]), b
            assert np.array_equal(w.env_edits[b], w.bank_edits[lv[b]]), b
            assert w.episode_level[b] == w.bank_seed[lv[b]]
        else:                                                             # free-running and unselected envs keep all three
            for k, v in before.items():
                assert np.array_equal(getattr(w, k)[b], v[b]), (b, k)
            assert w.episode_level[b] == (-1 if mask[b] else -7)
    assert np.array_equal(w.out_level, w.episode_level)
    assert w.guards_intact()
    assert all(np.array_equal(a, b) for a, b in zip(bank, (w.bank_params, w.bank_edits, w.bank_mt)))     # the bank is only read


def test_a_null_pair_copies_nothing_of_that_part(lvr):
    for params, edits in ((False, True), (True, False), (False, False)):
        w = World(lvr, seed=5)
        before = w.snapshot()
        takes = _takes(w, np.ones(B, bool))
        w.apply(N.LEVEL_MASK, None, params=params, edits=edits)
        lv = w.level_of_env
        assert np.array_equal(w.mt[takes], w.bank_mt[lv[takes]])           # the generator goes either way
        for on, name, bank in ((params, "env_params", w.bank_params), (edits, "env_edits", w.bank_edits)):
            if on:
                assert np.array_equal(getattr(w, name)[takes], bank[lv[takes]])
                assert np.array_equal(getattr(w, name)[~takes], before[name][~takes])
            else:
                assert np.array_equal(getattr(w, name), before[name])
        assert w.guards_intact()


def test_pending_rule_selects_the_envs_whose_episode_ended(lvr):
    w = World(lvr, seed=7)
    before = w.snapshot()
    ended = np.arange(B) % 4 == 0
    w.step_count[ended] = MAX_STEPS
    takes = _takes(w, ended)
    assert takes.sum() > 5
    w.apply(N.LEVEL_PENDING, None)
    lv = w.level_of_env
    assert np.array_equal(w.env_params[takes], w.bank_params[lv[takes]]) and np.array_equal(w.env_edits[takes], w.bank_edits[lv[takes]])
    for k, v in before.items():
        assert np.array_equal(getattr(w, k)[~takes], v[~takes]), k
    w2 = World(lvr, seed=7)
    w2.apply(N.LEVEL_PUBLISH, None)                                       # nobody is selected
    for k, v in before.items():
        assert np.array_equal(getattr(w2, k), v), k
    assert w.guards_intact() and w2.guards_intact()


def test_the_full_bank_of_a_dry_env():
    """`env.level_bank(..., full=True)`: the rows, their defaults, what `assign` checks"""
    from marlgrid_amd import envs as E
    env = E.make("MarlGrid-3AgentClutteredCurriculum15x15-v0", batch_size=4, level_edits=3, _dry=True)
    bank = env.level_bank(L, full=True)
    col = env._params.decl["n_clutter"]["col"]
    assert bank.full and bank.params.shape == (L, N.GEN_DRAWS) and bank.edits.shape == (L, 3, 4) and not bank.edits.any()
    assert bank.params[:, col].tolist() == [25] * L
    bank.assign([3, 1], [70, 71], params=dict(n_clutter=[5, 50]), edits=[(2, 2, 1, 1)])
    assert bank.seeds.tolist() == [-1, 71, -1, 70, -1] and bank.params[:, col].tolist() == [25, 50, 25, 5, 25]
    assert (bank.edits[[1, 3], 0] == (2, 2, 1, 1)).all() and not bank.edits[[0, 2, 4]].any() and not bank.edits[:, 1:].any()
    bank.assign([0], [72])                                                # what is not given stays
    assert bank.params[0, col] == 25
    per = np.zeros((2, 1, 4), np.int64)
    per[0, 0], per[1, 0] = (3, 3, 2, 1), (4, 4, 0, 1)
    bank.assign(None, [80, 81], edits=per)
    assert (bank.edits[0, 0] == (3, 3, 2, 1)).all() and (bank.edits[1, 0] == (4, 4, 0, 1)).all()
    for kw, exc in ((dict(params=dict(n_clutter=51)), ValueError), (dict(params=dict(nope=1)), KeyError),
                    (dict(edits=[(15, 1, 1, 1)]), ValueError), (dict(edits=[(1, 1, 3, 1)]), ValueError),
                    (dict(edits=[(1, 1, 1, 1)] * 4), ValueError)):
        with pytest.raises(exc):
            bank.assign([2], [9], **kw)
    assert bank.seeds[2] == -1                                            # a refused call wrote nothing
    plain = env.level_bank(L)
    assert not plain.full and plain.params is None and plain.edits is None
    with pytest.raises(ValueError, match="full=True"):
        plain.assign([0], [1], edits=[(1, 1, 1, 1)])
    other = E.make("MarlGrid-3AgentClutteredCurriculum15x15-v0", batch_size=4, level_edits=2, auto_reset="next_step", _dry=True)
    with pytest.raises(ValueError, match="level_edits"):
        other.set_levels(bank, 0)
