"""TEST INFRASTRUCTURE — whole levels on the host: hostemu_edits.EditsEmu (the step bodies with the parameter and edit tables
behind the template) stepped through an MgEpisode in next-step mode (hostemu_episode.EpisodeEmu), with the body of
mg_level_apply_rows (marlgrid_amd/csrc/mg_level_core.h, built by tests/native/mg_level_rows.cpp) run on its state arrays in front
of every reset and step, as MultiGridEnv does on the device.  Everything around it is the product's own host side on a `_dry`
env: `env.level_bank(L, full=True)` / `bank.assign` / `env.set_levels` / `set_params` / `set_edits` keep numpy tables, which the
emulated launch reads and — an env that takes a level — writes.  The bank's generators are the host seed path's (lvr_seed:
level_seed_row).  Nothing under marlgrid_amd/ imports it."""
import ctypes as C
import fcntl
import os
import subprocess

import numpy as np

import hostemu_edits
import hostemu_episode
import wide_diff
from marlgrid_amd import _native as N

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
vp = C.c_void_p
_lvr = None


def lvr():
    """libmg_level_rows.so, built as tests/test_level_rows_host.py builds it"""
    global _lvr
    if _lvr is None:
        out = os.path.join(HERE, "libmg_level_rows.so")
        with open(os.path.join(HERE, ".build.lock"), "w") as lock:
            fcntl.flock(lock, fcntl.LOCK_EX)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Wno-unused-function",
                                   "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "include"), "-I",
                                   os.path.join(ROOT, "marlgrid_amd", "csrc"), os.path.join(HERE, "mg_level_rows.cpp"), "-o", out])
        lib = C.CDLL(out)
        lib.lvr_seed.argtypes = [C.c_int, vp, C.c_int, vp, vp, vp, vp]
        lib.lvr_seed.restype = None
        lib.lvr_apply_rows.argtypes = [C.POINTER(N.Config), C.POINTER(N.State), C.c_int, vp, vp, C.c_int, vp, vp, vp, vp, vp, vp,
                                       vp, vp, C.c_int, vp, vp, C.c_int]
        lib.lvr_apply_rows.restype = None
        _lvr = lib
    return _lvr


def _p(a):
    if a is None:
        return None
    assert a.flags.c_contiguous, a.shape
    return vp(a.ctypes.data)


class LevelsEmu(hostemu_edits.EditsEmu, hostemu_episode.EpisodeEmu):
    """lanes: how many lanes share a level's copy (64: the kernel's wave; 1: one lane walks every item); mode: "next_step", or
    None — no reset inside a step, the caller resets by hand"""

    def __init__(self, name, B, seeds, lanes=64, mode="next_step", **kw):
        hostemu_episode.EpisodeEmu.__init__(self, name, B, seeds, mode=mode, par=True, **kw)
        self.lvr, self.lanes = lvr(), lanes
        self.episode_level = np.full(B, -1, np.int64)
        self.out_level = np.full(B, -1, np.int64)
        self.level_launches = 0
        self._gen = None            # the generators of the bank the batch reads: (bank, seeds they were made from, mt, pos, head)

    def _generators(self, bank):
        g = self._gen
        if g is None or g[0] is not bank or not np.array_equal(g[1], bank.seeds):
            L = bank.capacity
            seeds = np.ascontiguousarray(bank.seeds, np.int64).copy()
            mt = np.zeros((L, N.MT_N), np.uint32) if g is None or g[0] is not bank else g[2]
            pos = np.zeros(L, np.int32) if g is None or g[0] is not bank else g[3]
            head = np.zeros((L, N.MT_HEAD), np.uint32) if g is None or g[0] is not bank else g[4]
            seed_of = np.full(L, -1, np.int64)
            self.lvr.lvr_seed(L, _p(seeds), L, _p(mt), _p(pos), _p(head), _p(seed_of))
            assert np.array_equal(seed_of, seeds)
            self._gen = g = (bank, seeds, mt, pos, head)
        return g

    def _apply(self, rule, mask):
        lv, env = self.env._levels, self.env
        if not lv.on or lv.bank is None:
            return
        bank = lv.bank
        _, seeds, mt, pos, head = self._generators(bank)
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        par = bank.full and env.params_t is not None
        K = env.level_edits if bank.full else 0
        assert not bank.full or (bank.params.dtype == np.uint8 and bank.edits.dtype == np.uint8)
        self.lvr.lvr_apply_rows(C.byref(self._cfg()), C.byref(self.state), rule, _p(m), _p(lv.level_of_env), bank.capacity,
                                _p(mt), _p(pos), _p(head), _p(seeds), _p(self.episode_level), _p(self.out_level),
                                _p(bank.params) if par else None, _p(bank.edits) if K else None, K,
                                _p(env.params_t) if par else None, _p(env.edits_t) if K else None, self.lanes)
        self.level_launches += 1

    def reset(self, env_mask=None):
        self._apply(N.LEVEL_MASK, env_mask)
        hostemu_episode.EpisodeEmu.reset(self, env_mask)
        # (mg_reset knows nothing of the episode accumulators: MultiGridEnv.reset zeroes them itself, and so does this)
        self.ep_return[slice(None) if env_mask is None else np.asarray(env_mask, bool)] = 0.0

    def step(self, actions):
        # (MultiGridEnv.step: the pending rule under next-step reset; without auto-reset no env resets in a step: publish only)
        self._apply(N.LEVEL_PENDING if self.auto_reset else N.LEVEL_PUBLISH, None)
        r, d, info = hostemu_episode.EpisodeEmu.step(self, actions)
        info["level"] = self.out_level.copy()
        return r, d, info


class LevelsSubject(wide_diff.HostEmuSubject):
    """a LevelsEmu as tests/wide_diff.py:run steps it"""
    kernel_name = "host build of the step bodies and of mg_level_apply_rows"

    def step(self, a):
        r, d, info = self.emu.step(a)
        return None, r, d, info

    def level_state(self):
        env = self.emu.env
        return dict(episode_level=self.emu.episode_level,
                    params=None if env.params_t is None else {k: np.asarray(v) for k, v in env.params.items()},
                    edits=env.edits_t)
