"""TEST INFRASTRUCTURE — hostemu.HostEmu stepped through an MgEpisode (tests/native/mg_hostemu_episode.cpp): the step
bodies of marlgrid_amd/csrc/mg_core.h with next-step / same-step reset and the episode outputs, on the host.  Builds its
own library (libmg_hostemu_episode.so) next to the sources; nothing under marlgrid_amd/ imports it.
"""
import ctypes as C
import os
import subprocess

import numpy as np

import hostemu
from marlgrid_amd import _native as N

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
_SRC = os.path.join(HERE, "mg_hostemu_episode.cpp")
_SO = os.path.join(HERE, "libmg_hostemu_episode.so")
_DEPS = [_SRC, os.path.join(ROOT, "marlgrid_amd", "csrc", "mg_core.h"), os.path.join(ROOT, "include", "marlgrid_hip.h")]
_lib = None


def lib():
    global _lib
    if _lib is None:
        import fcntl
        with open(os.path.join(HERE, ".build.lock"), "w") as lock:
            fcntl.flock(lock, fcntl.LOCK_EX)
            if not os.path.exists(_SO) or os.path.getmtime(_SO) < max(os.path.getmtime(p) for p in _DEPS):
                subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function",
                                       "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "include"),
                                       "-I", os.path.join(ROOT, "marlgrid_amd", "csrc"), _SRC, "-o", _SO])
        L = C.CDLL(_SO)
        assert L.emu_ep_sizeof() == C.sizeof(N.Episode), (L.emu_ep_sizeof(), C.sizeof(N.Episode))
        _lib = L
    return _lib


class EpisodeEmu(hostemu.HostEmu):
    """mode: "next_step" | "same_step" (needs the reset program: auto_reset) | None (no reset, accumulators only)"""

    def __init__(self, name, B, seeds, mode="next_step", par=False, **kw):
        hostemu.HostEmu.__init__(self, name, B, seeds, auto_reset=mode is not None, par=par, **kw)
        self.LE = lib()
        self.ep_return = np.zeros((B, self.n), np.float64)
        self.out_return = np.full((B, self.n), np.nan, np.float64)
        self.out_length = np.full(B, -1, np.int32)
        self.out_flags = np.full(B, 0xFF, np.uint8)
        self.ep = N.Episode(N.RESET_NEXT_STEP if mode == "next_step" else N.RESET_SAME_STEP, 0,
                            self.ep_return.ctypes.data, self.out_return.ctypes.data, self.out_length.ctypes.data,
                            self.out_flags.ctypes.data)

    def step(self, actions):
        a = np.ascontiguousarray(actions, np.int64).reshape(self.B, self.n)
        prog = None
        if self.auto_reset:
            self.env.reset()
            self._last_prog = self._prog(self.env._dry_trace)
            prog = C.byref(self._last_prog)
        rc = self.LE.emu_ep_step(C.byref(self._cfg()), C.byref(self.state), hostemu._ptr(a), 8, hostemu._ptr(self.rewards), prog,
                                 C.byref(self.ep), int(self.par), C.byref(self.n_serial))
        assert rc == 0, rc
        f = self.out_flags
        info = dict(terminated=(f & N.EPF_TERMINATED) != 0, truncated=(f & N.EPF_TRUNCATED) != 0, reset=(f & N.EPF_RESET) != 0,
                    episode_return=self.out_return.copy(), episode_length=self.out_length.copy())
        return self.rewards.copy(), self.done.astype(bool), info
