"""TEST INFRASTRUCTURE — mg_memory_update on the host: tests/native/mg_memory.cpp (the bodies of
marlgrid_amd/csrc/mg_explore_core.h and mg_view_triple.h under g++) over a HostEmu's numpy state, as hostemu_explore.py runs
mg_explore_update.  `Maps` are the six tensors as numpy arrays; `update` is one call of the entry point per view group, as
marlgrid_amd/explore.py launches it; `Driver` is an emu whose reset() and step() end with that call.  Nothing under
marlgrid_amd/ imports it."""
import ctypes as C
import fcntl
import os
import subprocess

import numpy as np

import hostemu_explore as HX
from marlgrid_amd import _native as N

HERE = HX.HERE
SOURCE = os.path.join(HERE, "mg_memory.cpp")
vp = C.c_void_p
_lib = None


def lib():
    """libmg_memory.so, built on demand (one builder at a time)"""
    global _lib
    if _lib is None:
        out = os.path.join(HERE, "libmg_memory.so")
        with open(os.path.join(HERE, ".build.lock"), "w") as lock:
            fcntl.flock(lock, fcntl.LOCK_EX)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function",
                                   "-Wno-unknown-pragmas", "-UNDEBUG"] + HX.INCLUDES + [SOURCE, "-o", out])
        L = C.CDLL(out)
        L.mem_update.argtypes = [C.POINTER(N.Config), C.POINTER(N.State), vp, vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int,
                                 C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.mem_update.restype = C.c_int
        _lib = L
    return _lib


class Maps(HX.Maps):
    def __init__(self, B, n, W, H, fill=0, fill_step=None):
        super(Maps, self).__init__(B, n, W, H, fill)
        self.memory = np.full((B, n, W, H, 4), fill, np.uint8)
        self.seen_step = np.full((B, n, W, H), (-1 if fill == 0 else fill) if fill_step is None else fill_step, np.int32)

    def tensors(self):
        return dict(super(Maps, self).tensors(), memory=self.memory, seen_step=self.seen_step)


def update(emu, maps, mask=None, block=256, wave=64, rt=False, groups=None):
    """one observation more: mg_memory_update for every view group (`groups`: only these indices) -> the launches' (PB, LDS bytes)"""
    m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
    out = []
    for i, cfg in enumerate(HX.group_cfgs(emu)):
        if groups is not None and i not in groups:
            continue
        pb, lds = C.c_int(0), C.c_int(0)
        rc = lib().mem_update(C.byref(cfg), C.byref(emu.state), HX._p(m), HX._p(maps.seen), HX._p(maps.visits), HX._p(maps.new_cells),
                              HX._p(maps.visit_count), HX._p(maps.memory), HX._p(maps.seen_step), block, wave, int(rt), C.byref(pb),
                              C.byref(lds))
        assert rc == 0, rc
        out.append((pb.value, lds.value))
    return out


class Driver(object):
    """an emu with its Maps, as hostemu_explore.Driver; `shapes`: further (block, wave, rt) emulations on Maps of their own,
    which must stay identical to the first.  `explore`: Maps that mg_explore_update keeps beside them (the four tensors of the
    two entry points must agree)"""

    def __init__(self, emu, shapes=()):
        self.emu = emu
        env = emu.env
        dims = (emu.B, emu.n, env.width, env.height)
        self.maps = Maps(*dims)
        self.others = [(s, Maps(*dims)) for s in shapes]
        self.explore = HX.Maps(*dims)
        self.pb = None

    def _update(self, mask):
        self.pb = update(self.emu, self.maps, mask)
        for (block, wave, rt), m in self.others:
            update(self.emu, m, mask, block, wave, rt)
        HX.update(self.emu, self.explore, mask)

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
        for k, v in self.explore.tensors().items():
            assert np.array_equal(v, t[k]), ("mg_explore_update and mg_memory_update disagree", k)
        return t
