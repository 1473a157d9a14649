"""Replayable levels without a GPU: the bodies of mg_level_seed / mg_level_apply (marlgrid_amd/csrc/mg_level_core.h, the text
the kernels of mg_levels.hip run per lane) built with g++ (tests/native/mg_levels.cpp) — the seed hash against
seeding.seed_words, the seeding against numpy, the apply emulated lane by lane over numpy arrays, whole trajectories of
hostemu_episode.EpisodeEmu against the level oracle (tests/level_ref.py) — and the host API on `_dry` envs."""
import ctypes as C
import fcntl
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
NATIVE = os.path.join(HERE, "native")
CSRC = os.path.join(os.path.dirname(HERE), "marlgrid_amd", "csrc")
sys.path.insert(0, NATIVE)

import canon  # noqa: E402
import level_ref  # noqa: E402
import product_envs  # noqa: E402
import scenarios  # noqa: E402
from marlgrid_amd import LevelBank  # noqa: E402
from marlgrid_amd import _native as N  # noqa: E402
from marlgrid_amd import seeding, sharding  # noqa: E402

vp = C.c_void_p
BENCH = "MarlGrid-3AgentCluttered15x15-v0"


def _p(a):
    return None if a is None else vp(a.ctypes.data)


@pytest.fixture(scope="module")
def lv():
    out = os.path.join(NATIVE, "libmg_levels.so")
    with open(os.path.join(NATIVE, ".build.lock"), "w") as lock:        # (one builder at a time, as tests/native/hostemu.py)
        fcntl.flock(lock, fcntl.LOCK_EX)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Wno-unused-function",
                               "-Wno-unknown-pragmas", "-I", os.path.join(os.path.dirname(HERE), "include"), "-I", CSRC,
                               os.path.join(NATIVE, "mg_levels.cpp"), "-o", out])
    L = C.CDLL(out)
    L.lv_key.argtypes = [C.c_longlong, vp]
    L.lv_key_rule.argtypes = [C.c_uint32, C.c_uint32, vp]
    L.lv_seed.argtypes = [C.c_int, vp, vp, vp, C.c_int, vp, vp, vp, vp]
    L.lv_seed.restype = None
    L.lv_apply.argtypes = [C.POINTER(N.Config), C.POINTER(N.State), C.c_int, vp, vp, C.c_int, vp, vp, vp, vp, vp, vp]
    L.lv_apply.restype = None
    L.lv_episode_ended.argtypes = [C.POINTER(N.Config), vp, C.c_int]
    return L


class Bank(object):
    """a bank in numpy arrays"""

    def __init__(self, L):
        self.L = L
        self.mt = np.zeros((L, N.MT_N), np.uint32)
        self.pos = np.zeros(L, np.int32)
        self.head = np.zeros((L, N.MT_HEAD), np.uint32)
        self.seeds = np.full(L, -1, np.int64)

    def seed(self, lv, seeds, slots=None, mask=None):
        seeds = np.ascontiguousarray(seeds, np.int64)
        slots = None if slots is None else np.ascontiguousarray(slots, np.int64)
        mask = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        lv.lv_seed(len(seeds), _p(seeds), _p(slots), _p(mask), self.L, _p(self.mt), _p(self.pos), _p(self.head), _p(self.seeds))

    def args(self):
        return (self.L, _p(self.mt), _p(self.pos), _p(self.head), _p(self.seeds))


# ---- 1. the seed hash ------------------------------------------------------------------------------------------------------
def _key_seeds():
    s = list(range(4097))
    for k in range(1, 63):
        s += [2 ** k - 1, 2 ** k, 2 ** k + 1]
    s.append(2 ** 63 - 1)
    for k in range(1, 19):
        s += [10 ** k - 1, 10 ** k]
    rng = np.random.RandomState(20)
    s += [int(hi) << 32 | int(lo) for hi, lo in zip(rng.randint(0, 2 ** 31, 5000), rng.randint(0, 2 ** 32, 5000, dtype=np.int64))]
    return s


def test_level_key_is_seed_words(lv):
    key = np.zeros(N.KEY_WORDS, np.uint32)
    seeds = _key_seeds()
    assert max(seeds) == 2 ** 63 - 1 and len(seeds) > 9000
    for s in seeds:
        key[:] = 0xDEADBEEF
        klen = lv.lv_key(s, _p(key))
        want = seeding.seed_words(s)
        assert klen == len(want) and [int(w) for w in key[:klen]] == want, s


def test_word_to_key_rule(lv):
    """chosen words (a hash with a zero high word cannot be searched for): numpy's key of w0 + w1 * 2^32 is its base-2^32
    digits, [0] for zero; mt_seed_env reads key[0 .. klen)"""
    key = np.zeros(N.KEY_WORDS, np.uint32)
    x, y = 0x9E3779B9, 0x85EBCA6B
    for (w0, w1), klen in (((0, 0), 1), ((x, 0), 1), ((0, x), 2), ((x, y), 2)):
        key[:] = 0xDEADBEEF
        assert lv.lv_key_rule(w0, w1, _p(key)) == klen
        big = w0 | w1 << 32
        digits = [0] if big == 0 else [big & 0xFFFFFFFF] + ([big >> 32] if big >> 32 else [])
        assert [int(w) for w in key[:klen]] == digits


# ---- 2. the seeding body ---------------------------------------------------------------------------------------------------
def test_seeded_rows_are_numpys_streams(lv):
    seeds = [0, 1, 2 ** 32, 2 ** 63 - 1] + list(range(1000, 1060))
    bank = Bank(len(seeds) + 3)
    slots = np.random.RandomState(1).permutation(bank.L)[:len(seeds)]       # (rows out of order: slot != row)
    bank.mt[:] = 0xA5A5A5A5
    bank.seed(lv, seeds, slots)
    for s, slot in zip(seeds, slots):
        assert bank.seeds[slot] == s
        got = seeding.numpy_form(bank.mt[slot], bank.pos[slot], N.MT_HEAD)
        st = np.random.RandomState(seeding.seed_words(s)).get_state()
        assert seeding.same_stream(got, (st[1], st[2])), s
        # ... and the head is the stream's first outputs
        assert np.array_equal(bank.head[slot], np.random.RandomState(seeding.seed_words(s)).randint(0, 2 ** 32, N.MT_HEAD, dtype=np.uint64).astype(np.uint32))
    rest = np.setdiff1d(np.arange(bank.L), slots)
    assert (bank.seeds[rest] == -1).all() and (bank.mt[rest] == 0xA5A5A5A5).all()
    # an empty seed: the row's bytes stay, the slot is empty; a slot outside the bank is skipped; a masked row is kept
    before = (bank.mt.copy(), bank.pos.copy(), bank.head.copy())
    keep = bank.seeds.copy()
    bank.seed(lv, [-1, 77, 78, 79], [slots[0], bank.L, -1, slots[1]], mask=[1, 1, 1, 0])
    keep[slots[0]] = -1
    assert np.array_equal(bank.seeds, keep)
    for a, b in zip(before, (bank.mt, bank.pos, bank.head)):
        assert np.array_equal(a, b)


def test_bank_seeding_is_mt_seed_env_for_chosen_keys(lv):
    """the bank's seeding body walks init_by_array its own way (mg_level_core.h: level_seed_mt): word for word what mt_seed_env
    leaves, and numpy's RandomState(key) — also for one-word keys, which no seed's hash can be made to give"""
    lv.lv_seed_key.argtypes = [C.c_int, vp, C.c_int, vp, vp, vp]
    lv.lv_seed_key.restype = None
    for key in ([0], [1], [0xFFFFFFFF], [0x9E3779B9], [0, 1], [0, 0xFFFFFFFF], [0x9E3779B9, 0x85EBCA6B], [0xFFFFFFFF, 0xFFFFFFFF]):
        k = np.zeros(N.KEY_WORDS, np.uint32)
        k[:len(key)] = key
        got = []
        for which in (0, 1):
            mt, pos, head = np.full(N.MT_N, 0xA5A5A5A5, np.uint32), np.zeros(1, np.int32), np.zeros(N.MT_HEAD, np.uint32)
            lv.lv_seed_key(which, _p(k), len(key), _p(mt), _p(pos), _p(head))
            got.append((mt, pos, head))
        for a, b in zip(*got):
            assert np.array_equal(a, b), key
        st = np.random.RandomState(key).get_state()
        assert seeding.same_stream(seeding.numpy_form(got[1][0], got[1][1][0], N.MT_HEAD), (st[1], st[2])), key


# ---- 3. the apply body -----------------------------------------------------------------------------------------------------
class Envs(object):
    """the part of an env batch's state the apply reads and writes, in numpy arrays"""

    def __init__(self, B, n, max_steps):
        self.B, self.n = B, n
        self.cfg = N.Config()
        self.cfg.B, self.cfg.n_agents, self.cfg.max_steps = B, n, max_steps
        rng = np.random.RandomState(3)
        self.rec = rng.randint(0, 2 ** 62, (B, n), dtype=np.int64).astype(np.uint64) & ~np.uint64(N.AF_DONE << (8 * N.AG_FLAGS))
        self.mt = rng.randint(0, 2 ** 32, (B, N.MT_N), dtype=np.int64).astype(np.uint32)
        self.mt_pos = rng.randint(0, N.MT_N, B).astype(np.int32)
        self.mt_head = rng.randint(0, 2 ** 32, (B, N.MT_HEAD), dtype=np.int64).astype(np.uint32)
        self.step_count = np.zeros(B, np.int32)
        self.done = np.full(B, 0x5A, np.uint8)          # (never read: garbage)
        self.error = np.zeros(B, np.int32)
        self.grid = np.zeros((B, 16), np.uint8)
        self.state = N.State(_p(self.grid), _p(self.rec), _p(self.mt), _p(self.mt_pos), _p(self.step_count), _p(self.done),
                             _p(self.error), None, _p(self.mt_head))
        self.level_of_env = np.full(B, -1, np.int64)
        self.episode_level = np.full(B, -7, np.int64)
        self.out_level = np.full(B, -9, np.int64)

    def set_done(self, b, agents):
        for k in agents:
            self.rec[b, k] |= np.uint64(N.AF_DONE << (8 * N.AG_FLAGS))

    def rng(self):
        return self.mt.copy(), self.mt_pos.copy(), self.mt_head.copy()

    def apply(self, lv, rule, bank, mask=None, out=True):
        mask = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        lv.lv_apply(C.byref(self.cfg), C.byref(self.state), rule, _p(mask), _p(self.level_of_env), *bank.args(),
                    _p(self.episode_level), _p(self.out_level) if out else None)


def _check_apply(e, bank, before, selected):
    """envs of `selected` with a filled slot hold the slot's generator and its seed; selected ones without are free-running;
    the others keep every byte"""
    ep_before = before[3]
    for b in range(e.B):
        lvl = e.level_of_env[b]
        filled = 0 <= lvl < bank.L and bank.seeds[lvl] >= 0
        if selected[b] and filled:
            assert np.array_equal(e.mt[b], bank.mt[lvl]) and e.mt_pos[b] == bank.pos[lvl] and np.array_equal(e.mt_head[b], bank.head[lvl]), b
            assert e.episode_level[b] == bank.seeds[lvl], b
            # ... and its agents face heading 0 (a reset keeps the heading: the level starts as in an env made for it); nothing else
            assert np.array_equal(e.rec[b], before[4][b] & ~np.uint64(0xFF << (8 * N.AG_DIR))), b
        else:
            assert np.array_equal(e.rec[b], before[4][b]), b
            assert np.array_equal(e.mt[b], before[0][b]) and e.mt_pos[b] == before[1][b] and np.array_equal(e.mt_head[b], before[2][b]), b
            assert e.episode_level[b] == (-1 if selected[b] else ep_before[b]), b
    assert np.array_equal(e.out_level, e.episode_level)


def test_apply_pending_rule_is_episode_ended(lv):
    B, n, T = 12, 3, 9
    e = Envs(B, n, T)
    bank = Bank(4)
    bank.seed(lv, [11, 12, -1, 14])
    e.level_of_env[:] = [0, 1, 2, 3, -1, 4, 0, 0, 1, 3, 3, 0]      # (2: an empty slot; 4: outside the bank)
    e.step_count[:] = [T, T - 1, T, T, T, T, 0, 0, 0, T + 1, T - 1, 1]
    e.set_done(6, [0, 1, 2])            # all agents done
    e.set_done(7, [0, 2])               # all but one
    e.set_done(10, [0, 1, 2])
    ended = np.array([bool(lv.lv_episode_ended(C.byref(e.cfg), _p(e.rec[b]), int(e.step_count[b]))) for b in range(B)])
    assert ended.tolist() == [True, False, True, True, True, True, True, False, False, True, True, False]
    before = e.rng() + (e.episode_level.copy(), e.rec.copy())
    e.apply(lv, N.LEVEL_PENDING, bank)
    _check_apply(e, bank, before, ended)
    assert e.episode_level.tolist() == [11, -7, -1, 14, -1, -1, 11, -7, -7, 14, 14, -7]
    assert (e.done == 0x5A).all()
    # neither rule: nothing but the published copy
    e.episode_level[:] = np.arange(B)
    before = e.rng() + (e.episode_level.copy(), e.rec.copy())
    e.apply(lv, N.LEVEL_PUBLISH, bank)
    _check_apply(e, bank, before, np.zeros(B, bool))
    # no out_level: the same without it
    e.out_level[:] = -9
    e.apply(lv, N.LEVEL_PENDING, bank, out=False)
    assert (e.out_level == -9).all() and e.episode_level.tolist() == [11, 1, -1, 14, -1, -1, 11, 7, 8, 14, 14, 11]


def test_apply_mask_rule_has_mg_resets_polarity(lv):
    B = 70
    e = Envs(B, 2, 5)
    bank = Bank(3)
    bank.seed(lv, [5, -1, 2 ** 63 - 1])
    rng = np.random.RandomState(9)
    e.level_of_env[:] = rng.randint(-1, 5, B)
    mask = rng.randint(0, 3, B).astype(np.uint8)           # (any non-zero byte selects, as mg_reset's env_mask)
    before = e.rng() + (e.episode_level.copy(), e.rec.copy())
    e.apply(lv, N.LEVEL_MASK, bank, mask=mask)
    _check_apply(e, bank, before, mask != 0)
    assert (mask == 0).any() and (mask == 2).any()
    before = e.rng() + (e.episode_level.copy(), e.rec.copy())
    e.apply(lv, N.LEVEL_MASK, bank)                         # no mask: every env
    _check_apply(e, bank, before, np.ones(B, bool))
    assert set(e.episode_level.tolist()) == {5, -1, 2 ** 63 - 1}


# ---- 4. whole trajectories -------------------------------------------------------------------------------------------------
P_ACT = [.15, .15, .5, .05, .05, .05, .05]
REW_TOL = 1e-6      # per step: tests/test_core_hostemu.py


class LevelEmu(object):
    """hostemu_episode.EpisodeEmu as it is, with the apply body run on its state arrays in front of every reset and step —
    the seeds form: a bank with row b for env b"""

    def __init__(self, lv, name, B, seeds, par, **kw):
        import hostemu_episode
        self.lv = lv
        self.emu = hostemu_episode.EpisodeEmu(name, B, seeds, mode="next_step", par=par, **kw)
        self.B = B
        self.bank = Bank(B)
        self.level_of_env = np.arange(B, dtype=np.int64)
        self.episode_level = np.full(B, -1, np.int64)
        self.out_level = np.full(B, -1, np.int64)

    def set_levels(self, seeds, mask):
        self.bank.seed(self.lv, np.broadcast_to(np.asarray(seeds, np.int64), (self.B,)), mask=mask)

    def _apply(self, rule):
        e = self.emu
        self.lv.lv_apply(C.byref(e._cfg()), C.byref(e.state), rule, None, _p(self.level_of_env), *self.bank.args(),
                         _p(self.episode_level), _p(self.out_level))

    def reset(self):
        self._apply(N.LEVEL_MASK)
        self.emu.reset()

    def step(self, a):
        self._apply(N.LEVEL_PENDING)
        r, d, info = self.emu.step(a)
        info["level"] = self.out_level.copy()
        return r, d, info


@pytest.mark.parametrize("par", [False, True])
def test_trajectories_with_levels_vs_oracle(lv, par):
    B, T = 40, 60
    seeds = 4200 + np.arange(B)
    emu = LevelEmu(lv, BENCH, B, seeds, par, max_steps=9)
    spec = dict(scenarios.registered(BENCH), max_steps=9)
    ref = level_ref.LevelOracle(spec, seeds)
    # what a finished env is given next: fresh seeds, repeats of earlier ones, now and then none
    pool = [7, 2 ** 32 + 5, 2 ** 63 - 1, 0]
    rng = np.random.RandomState(5)
    first = 100 + np.arange(B)
    first[::7] = -1
    emu.set_levels(first, None)
    ref.set_levels(first)
    emu.reset()
    ref.reset()
    assert np.array_equal(emu.episode_level, ref.episode_level)
    fresh = 50000
    had_free = first < 0        # (one free-running episode per env at the most: six or more of an env's seven resets take a level)
    for t in range(T):
        a = rng.choice(7, size=(B, emu.emu.n), p=P_ACT)
        r, d, info = emu.step(a)
        _o, r2, d2, want = ref.step(a)
        what = "step %d" % t
        assert np.abs(r.astype(np.float64) - r2).max() <= REW_TOL, what
        assert np.array_equal(d, d2), what
        level_ref.assert_info(info, want, what)
        assert np.array_equal(emu.episode_level, ref.episode_level), what
        st = emu.emu.canonical()
        for b in range(B):
            canon.assert_same(st[b], canon.oracle_canonical(ref.envs[b]), "%s env %d" % (what, b))
        if d.any():
            nxt = np.full(B, -1, np.int64)
            for b in np.nonzero(d)[0]:
                kind = rng.randint(0, 10)
                if kind < 5:
                    nxt[b] = fresh
                    fresh += 1
                elif kind < 9 or had_free[b]:
                    nxt[b] = pool[rng.randint(len(pool))] if kind < 7 else first[(b + 1) % B] if first[(b + 1) % B] >= 0 else 3
                had_free[b] |= nxt[b] < 0
                if nxt[b] >= 0 and len(pool) < 64:
                    pool.append(int(nxt[b]))
            emu.set_levels(nxt, d)
            ref.set_levels(nxt, d)
    for b in range(B):
        assert seeding.same_stream(emu.emu.numpy_rng_state(b), ref.envs[b].mt_state()), "RNG of env %d" % b
    assert not emu.emu.error.any()
    assert ref.levelled.min() >= 5, ref.levelled       # every env started at least 5 episodes from a level
    assert had_free.sum() > (first < 0).sum()           # ... and some went back to their running stream in between


# ---- 5. the host API --------------------------------------------------------------------------------------------------------
def _dry(B=6, **kw):
    return product_envs.build(BENCH, batch_size=B, seeds=list(range(B)), _dry=True, **kw)


def test_set_levels_needs_next_step_reset():
    env = _dry(auto_reset=True)
    with pytest.raises(ValueError, match="next_step") as e:
        env.set_levels(seeds=3)
    assert "same-step reset happens inside the launch that ends the episode" in str(e.value)
    for mode in (False, "next_step"):
        _dry(auto_reset=mode).set_levels(seeds=3)


def test_set_levels_validation():
    env = _dry(auto_reset="next_step")
    bank = env.level_bank(4)
    assert isinstance(bank, LevelBank) and len(bank) == 4 and (bank.seeds == -1).all()
    bank.assign([0, 3], [10, 2 ** 63 - 1])
    assert bank.seeds.tolist() == [10, -1, -1, 2 ** 63 - 1]
    for bad in (dict(slots=[4], seeds=[1]), dict(slots=[-1], seeds=[1]), dict(slots=[0], seeds=[-2]), dict(slots=[1, 1], seeds=[1, 2]),
                dict(slots=[0, 1], seeds=[1]), dict(slots=None, seeds=[1] * 5), dict(slots=[0], seeds=[1.5])):
        with pytest.raises(ValueError):
            bank.assign(**bad)
    assert bank.seeds.tolist() == [10, -1, -1, 2 ** 63 - 1]
    with pytest.raises(ValueError):
        LevelBank(0, _dry=True)
    ok = [dict(bank=bank, ids=[0, 1, 2, 3, -1, 0]), dict(bank=bank, ids=3), dict(bank=bank, ids=[1, 2], env_ids=[5, 0]),
          dict(bank=bank, ids=-1, env_mask=[1, 0, 0, 0, 0, 1])]
    for kw in ok:
        env.set_levels(**kw)
    assert env._level_of_env.tolist() == [-1, 3, 3, 3, 3, -1]
    bad = [dict(bank=bank, ids=4), dict(bank=bank, ids=[0, 0, 0, 0, 0, -2]), dict(bank=bank, ids=[0, 1]), dict(bank=bank, ids=[[0] * 6]),
           dict(bank=bank, ids=0, env_mask=[1] * 6, env_ids=[0]), dict(bank=bank, ids=0, env_mask=[1] * 5), dict(bank=bank, ids=0, env_ids=[6]),
           dict(bank=bank, ids=[0, 1, 2], env_ids=[0, 1]), dict(bank=bank), dict(ids=[0] * 6), dict(), dict(bank=bank, ids=0, seeds=1),
           dict(seeds=-2), dict(seeds=[0, 1, 2, 3, 4, -2]), dict(seeds=[1, 2]), dict(seeds=2 ** 63), dict(seeds=1.0),
           dict(seeds=1, env_mask=[1] * 6, env_ids=[0]), dict(seeds=[1, 2, 3], env_ids=[0, 1]),
           dict(seeds=5, env_ids=[0])]       # (a change of bank for some of the envs only)
    for kw in bad:
        with pytest.raises(ValueError):
            env.set_levels(**kw)
    assert env._level_of_env.tolist() == [-1, 3, 3, 3, 3, -1]
    env.set_levels(seeds=[5, 6, 7, -1, 2 ** 63 - 1, 0])
    env.set_levels(seeds=[9, 9], env_ids=[1, 3])
    env.set_levels(seeds=-1, env_mask=[1, 0, 0, 0, 0, 0])
    assert env._own_bank.seeds.tolist() == [-1, 9, 7, 9, 2 ** 63 - 1, 0] and env._level_of_env.tolist() == list(range(6))


def test_split_levels_over_uneven_ranges():
    ranges = sharding.shard_ranges(7, 3)
    assert ranges == [(0, 3), (3, 5), (5, 7)]
    ids = np.arange(7) + 10
    parts = sharding.split_levels(ranges, ids=ids)
    assert [p["ids"].tolist() for p in parts] == [[10, 11, 12], [13, 14], [15, 16]] and all(set(p) == {"ids"} for p in parts)
    mask = np.array([1, 0, 0, 1, 1, 0, 1], bool)
    parts = sharding.split_levels(ranges, seeds=ids, env_mask=mask)
    assert [p["seeds"].tolist() for p in parts] == [[10, 11, 12], [13, 14], [15, 16]]
    assert [p["env_mask"].tolist() for p in parts] == [[True, False, False], [True, True], [False, True]]
    parts = sharding.split_levels(ranges, seeds=[70, 71, 72], env_ids=[6, 0, 5])
    assert parts[1] is None
    assert parts[0]["env_ids"].tolist() == [0] and parts[0]["seeds"].tolist() == [71]
    assert parts[2]["env_ids"].tolist() == [1, 0] and parts[2]["seeds"].tolist() == [70, 72]
    parts = sharding.split_levels(ranges, ids=-1, env_ids=[4])
    assert parts[0] is None and parts[2] is None and parts[1] == {"env_ids": parts[1]["env_ids"], "ids": -1} and parts[1]["env_ids"].tolist() == [1]
    for bad in (dict(), dict(ids=1, seeds=1), dict(ids=[1, 2]), dict(seeds=1, env_ids=[7]), dict(seeds=1, env_mask=mask, env_ids=[0]),
                dict(seeds=1, env_mask=mask[:6])):
        with pytest.raises(ValueError):
            sharding.split_levels(ranges, **bad)


def test_state_dicts_merge_and_split_with_and_without_level_keys():
    import torch
    from marlgrid_amd.base import STATE_DICT_VERSION

    def sd(rows, levels, at=0):
        d = {"grid_state": torch.arange(rows * 4).reshape(rows, 4) + at, "version": torch.tensor(STATE_DICT_VERSION)}
        if levels:
            d["episode_level_t"] = torch.arange(rows, dtype=torch.int64) + at
            d["level_next_t"] = torch.arange(rows, dtype=torch.int64) * 3 - 1 + at
        return d
    for levels in (False, True):
        parts = [sd(3, levels), sd(2, levels, 100), sd(2, levels, 200)]
        whole = sharding.merge_state_dicts(parts)
        assert ("level_next_t" in whole) == ("episode_level_t" in whole) == levels
        if levels:
            assert whole["episode_level_t"].tolist() == [0, 1, 2, 100, 101, 200, 201]
            assert whole["level_next_t"].tolist() == [-1, 2, 5, 99, 102, 199, 202]
        back = sharding.split_state_dict(whole, [(0, 3), (3, 5), (5, 7)])
        for a, b in zip(parts, back):
            assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)
    # in every shard or in none
    with pytest.raises(KeyError):
        sharding.merge_state_dicts([sd(3, True), sd(2, False)])
