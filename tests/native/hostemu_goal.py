"""TEST INFRASTRUCTURE — mg_goal_distance on the host: tests/native/mg_goal_dist.cpp (the bodies of
marlgrid_amd/csrc/mg_goal_core.h under g++) over numpy arrays — a HostEmu's own MgState, or a grid made by hand (`raw_case`).
Nothing under marlgrid_amd/ imports it."""
import ctypes as C
import fcntl
import os
import subprocess

import numpy as np

from marlgrid_amd import _native as N

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SOURCE = os.path.join(HERE, "mg_goal_dist.cpp")
INCLUDES = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "marlgrid_amd", "csrc")]
vp = C.c_void_p
_lib = None


def lib():
    """libmg_goal_dist.so, built on demand (one builder at a time, as hostemu_levels.lvr())"""
    global _lib
    if _lib is None:
        out = os.path.join(HERE, "libmg_goal_dist.so")
        with open(os.path.join(HERE, ".build.lock"), "w") as lock:
            fcntl.flock(lock, fcntl.LOCK_EX)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Wno-unused-function",
                                   "-Wno-unknown-pragmas"] + INCLUDES + [SOURCE, "-o", out])
        L = C.CDLL(out)
        L.gd_general.argtypes = [C.POINTER(N.Config), C.POINTER(N.State), vp, vp, vp, C.c_int]
        L.gd_general.restype = C.c_int
        L.gd_reg.argtypes = [C.POINTER(N.Config), C.POINTER(N.State), vp, vp, vp]
        L.gd_reg.restype = C.c_int
        L.gd_scratch_bytes.argtypes = [C.c_int, C.c_int]
        L.gd_scratch_bytes.restype = C.c_size_t
        _lib = L
    return _lib


def _p(a):
    return None if a is None else vp(a.ctypes.data)


def run(cfg, state, path="general", lanes=64, mask=None, field=True, dist=None, fld=None, fill=-7):
    """One emulated mg_goal_distance: -> (agent_dist (B, n), field (B, W, H, 4) or None).  `dist` / `fld`: arrays to write into
    (rows of unselected envs keep what they hold); fresh ones are filled with `fill`, a value no result takes."""
    B, W, H, n = cfg.B, cfg.W, cfg.H, cfg.n_agents
    dist = np.full((B, n), fill, np.int32) if dist is None else dist
    if field and fld is None:
        fld = np.full((B, W, H, 4), fill, np.int32)
    m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
    if path == "general":
        rc = lib().gd_general(C.byref(cfg), C.byref(state), _p(m), _p(dist), _p(fld) if field else None, lanes)
    else:
        rc = lib().gd_reg(C.byref(cfg), C.byref(state), _p(m), _p(dist), _p(fld) if field else None)
    assert rc == 0, rc
    return dist, (fld if field else None)


class RawCase(object):
    """A batch made by hand: grid (B, W, H) of ids into a table of kinds given as (flags, reward_kind) pairs (id 0: None), agents
    as (B, n) tuples (x, y, dir, flags)"""
    WALL, GOAL, LAVA, FLOOR, DOOR_OPEN, DOOR_CLOSED = 1, 2, 3, 4, 5, 6
    KINDS = [(0, 0), (0, 0), (N.OF_CAN_OVERLAP | N.OF_ENDS_EPISODE, 1), (N.OF_CAN_OVERLAP | N.OF_ENDS_EPISODE, 0),
             (N.OF_CAN_OVERLAP, 0), (N.OF_CAN_OVERLAP | N.OF_IS_DOOR | N.OF_SEE_BEHIND, 0), (N.OF_IS_DOOR, 0)]

    def __init__(self, grid, agents):
        grid = np.asarray(grid, np.uint8)
        B, W, H = grid.shape
        self.stride = (W * H + 15) // 16 * 16
        self.grid = np.zeros((B, self.stride), np.uint8)
        self.grid[:, :W * H] = grid.reshape(B, -1)
        agents = np.asarray(agents, np.uint64).reshape(B, -1, 4)
        self.rec = np.ascontiguousarray(agents[..., 0] | (agents[..., 1] << np.uint64(8)) | (agents[..., 2] << np.uint64(16))
                                        | (agents[..., 3] << np.uint64(24)))
        self.obj = (N.ObjDesc * len(self.KINDS))()
        for i, (f, rk) in enumerate(self.KINDS):
            self.obj[i].flags, self.obj[i].reward_kind = f, rk
        self.cfg = N.Config()
        self.cfg.B, self.cfg.W, self.cfg.H, self.cfg.n_agents = B, W, H, self.rec.shape[1]
        self.cfg.cells_stride, self.cfg.n_obj = self.stride, len(self.KINDS)
        self.cfg.obj = C.addressof(self.obj)
        self.state = N.State()
        self.state.grid, self.state.agents = self.grid.ctypes.data, self.rec.ctypes.data

    def kinds(self):
        """(free_ids, goal_ids) as goal_ref.kinds_of gives them for an env"""
        flags = np.array([f for f, _ in self.KINDS])
        rk = np.array([r for _, r in self.KINDS])
        ends = (flags & N.OF_ENDS_EPISODE) != 0
        free = ((flags & N.OF_CAN_OVERLAP) != 0) & ~ends
        free[0] = True
        return free, ends & (rk == 1)
