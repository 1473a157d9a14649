"""TEST INFRASTRUCTURE — mg_fork_rows / mg_rollout on the host: tests/native/mg_lookahead.cpp (the bodies of
marlgrid_amd/csrc/mg_lookahead_core.h under g++) over numpy arrays — a HostEmu's own MgState as the source, a `Shadow` of
the same arrays as the destination.  Nothing under marlgrid_amd/ imports it."""
import ctypes as C
import fcntl
import os
import subprocess

import numpy as np

from marlgrid_amd import _native as N

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SOURCE = os.path.join(HERE, "mg_lookahead.cpp")
INCLUDES = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "marlgrid_amd", "csrc")]
vp = C.c_void_p
_lib = None

STATE_ARRAYS = ("grid", "rec", "mt", "mt_pos", "mt_head", "step_count", "done", "error", "prestige")


def lib():
    """libmg_lookahead.so, built on demand (one builder at a time, as hostemu_solve.lib())"""
    global _lib
    if _lib is None:
        out = os.path.join(HERE, "libmg_lookahead.so")
        with open(os.path.join(HERE, ".build.lock"), "w") as lock:
            fcntl.flock(lock, fcntl.LOCK_EX)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function",
                                   "-Wno-unknown-pragmas", "-UNDEBUG"] + INCLUDES + [SOURCE, "-o", out])
        L = C.CDLL(out)
        L.la_fork.argtypes = [C.POINTER(N.Config), C.POINTER(N.State), C.POINTER(N.State), vp, vp, C.c_int, C.c_int, C.c_int, C.c_int]
        L.la_fork.restype = C.c_int
        L.la_rollout.argtypes = [C.POINTER(N.Config), C.POINTER(N.State), vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, C.c_int]
        L.la_rollout.restype = C.c_int
        _lib = L
    return _lib


def _p(a):
    return None if a is None else vp(a.ctypes.data)


class Shadow(object):
    """R rows of state arrays named as a HostEmu's, filled with a pattern (a fork has to write every byte it owns)"""

    def __init__(self, emu, R, fill=0xA5):
        self.R, self.n = R, emu.n
        for k in STATE_ARRAYS:
            a = getattr(emu, k)
            setattr(self, k, np.frombuffer(bytes([fill]) * (R * a[0].nbytes), a.dtype).reshape((R,) + a.shape[1:]).copy())
        self.state = N.State(_p(self.grid), _p(self.rec), _p(self.mt), _p(self.mt_pos), _p(self.step_count), _p(self.done),
                             _p(self.error), _p(self.prestige), _p(self.mt_head), None)


def snapshot(emu):
    """the source's state arrays, copied: what a lookahead must leave bit-identical"""
    return {k: getattr(emu, k).copy() for k in STATE_ARRAYS}


def config(emu, rows):
    cfg = N.Config.from_buffer_copy(emu._cfg())
    cfg.B = rows
    return cfg


def fork(emu, shadow, K, ids=None, lanes=64):
    """mg_fork_rows: K copies of the envs `ids` (None: all) of `emu` into `shadow`, plan-major"""
    m = emu.B if ids is None else len(ids)
    i64 = None if ids is None else np.ascontiguousarray(ids, np.int64)
    rc = lib().la_fork(C.byref(emu._cfg()), C.byref(emu.state), C.byref(shadow.state), _p(i64), None, K * m, K * m, m, lanes)
    assert rc == 0, rc
    return m


def rollout(emu, shadow, actions, m, S=64):
    """mg_rollout over the first K * m rows of `shadow`: actions (K, T, m, n) -> rewards (K, T, m, n), done (K, T, m) bool,
    errors (K, m); outputs start as a pattern: every element has to be written"""
    a = np.ascontiguousarray(actions)
    K, T = a.shape[:2]
    assert a.shape == (K, T, m, emu.n) and a.dtype in (np.int64, np.int32, np.uint8), (a.shape, a.dtype)
    rewards = np.full((K, T, m, emu.n), np.float32(-77.0), np.float32)
    done = np.full((K, T, m), 0xA5, np.uint8)
    errors = np.full((K, m), -77, np.int32)
    rc = lib().la_rollout(C.byref(config(emu, K * m)), C.byref(shadow.state), _p(a), a.dtype.itemsize, T, m, _p(rewards), _p(done),
                          _p(errors), S)
    assert rc == 0, rc
    assert np.isin(done, (0, 1)).all()
    return rewards, done.astype(bool), errors
