"""TEST INFRASTRUCTURE — mg_explore_update on the host: tests/native/mg_explore.cpp (the bodies of
marlgrid_amd/csrc/mg_explore_core.h under g++) over a HostEmu's numpy state.  `Maps` are the four tensors as numpy arrays;
`update` is one call of the entry point per view group, as marlgrid_amd/explore.py launches it; `Driver` is a HostEmu (or an
EpisodeEmu, for the auto-reset modes) whose reset() and step() end with that call, as the env's do.  Nothing under marlgrid_amd/
imports it."""
import ctypes as C
import fcntl
import os
import subprocess

import numpy as np

from marlgrid_amd import _native as N
from marlgrid_amd import launch_tables as LT

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SOURCE = os.path.join(HERE, "mg_explore.cpp")
INCLUDES = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "marlgrid_amd", "csrc")]
vp = C.c_void_p
_lib = None


def lib():
    """libmg_explore.so, built on demand (one builder at a time, as hostemu_lookahead.lib())"""
    global _lib
    if _lib is None:
        out = os.path.join(HERE, "libmg_explore.so")
        with open(os.path.join(HERE, ".build.lock"), "w") as lock:
            fcntl.flock(lock, fcntl.LOCK_EX)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function",
                                   "-Wno-unknown-pragmas", "-UNDEBUG"] + INCLUDES + [SOURCE, "-o", out])
        L = C.CDLL(out)
        L.ex_update.argtypes = [C.POINTER(N.Config), C.POINTER(N.State), vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int,
                                C.POINTER(C.c_int)]
        L.ex_update.restype = C.c_int
        _lib = L
    return _lib


def _p(a):
    return None if a is None else vp(a.ctypes.data)


class Maps(object):
    def __init__(self, B, n, W, H, fill=0):
        self.seen = np.full((B, n, W, H), fill, np.uint8)
        self.visits = np.full((B, n, W, H), fill, np.int32)
        self.new_cells = np.full((B, n), fill, np.int32)
        self.visit_count = np.full((B, n), fill, np.int32)

    def tensors(self):
        return dict(seen=self.seen.astype(bool), visits=self.visits, new_cells=self.new_cells, visit_count=self.visit_count)


def group_cfgs(emu):
    """the launch config of every view group of the emu's env, as HostEmu._cfg() makes the first one's (kept on the emu)"""
    env = emu.env
    emu._cfg()      # (the tables and settings of the first group, and the spawn's reject table)
    key = (env.obj_reg.version, LT.read_settings(env))
    if getattr(emu, "_explore_cfgs_key", None) != key:
        keep = []
        for g in env._groups:
            t = LT.group_tables(env, g)
            t.cfg.obj = t.obj_raw.ctypes.data
            t.cfg.hide_by_obj = None if t.hide_by is None else t.hide_by.ctypes.data
            LT.apply_settings(t.cfg, key[1], None if emu._spawn_rej is None else emu._spawn_rej.ctypes.data)
            keep.append(t)
        emu._explore_cfgs, emu._explore_cfgs_key = keep, key
    return [t.cfg for t in emu._explore_cfgs]


def update(emu, maps, mask=None, block=256, wave=64, rt=False, groups=None):
    """one observation more: mg_explore_update for every view group (`groups`: only these indices) -> the launches' PB"""
    m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
    out = []
    for i, cfg in enumerate(group_cfgs(emu)):
        if groups is not None and i not in groups:
            continue
        pb = C.c_int(0)
        rc = lib().ex_update(C.byref(cfg), C.byref(emu.state), _p(m), _p(maps.seen), _p(maps.visits), _p(maps.new_cells),
                             _p(maps.visit_count), block, wave, int(rt), C.byref(pb))
        assert rc == 0, rc
        out.append(pb.value)
    return out


class Driver(object):
    """an emu with its Maps: reset(mask) and step(actions) -> done, each followed by one update; `shapes`: further (block, wave,
    rt) emulations run beside the first on Maps of their own, which must stay identical to it"""

    def __init__(self, emu, shapes=()):
        self.emu = emu
        env = emu.env
        self.maps = Maps(emu.B, emu.n, env.width, env.height)
        self.others = [(s, Maps(emu.B, emu.n, env.width, env.height)) for s in shapes]
        self.pb = None

    def _update(self, mask):
        self.pb = update(self.emu, self.maps, mask)
        for (block, wave, rt), m in self.others:
            update(self.emu, m, mask, block, wave, rt)

    def reset(self, mask=None):
        self.emu.reset(None if mask is None else np.asarray(mask, bool))
        self._update(mask)

    def step(self, actions):
        out = self.emu.step(actions)
        self._update(None)
        return out

    def tensors(self):
        t = self.maps.tensors()
        for shape, m in self.others:
            for k, v in m.tensors().items():
                assert np.array_equal(v, t[k]), ("the emulation shapes disagree", shape, k)
        return t
