"""TEST INFRASTRUCTURE — mg_solve_distance on the host: tests/native/mg_solve_dist.cpp (the bodies of
marlgrid_amd/csrc/mg_solve_core.h under g++, every scratch index asserted) over numpy arrays — a HostEmu's own MgState, or a
grid made by hand (`SolveCase`).  Nothing under marlgrid_amd/ imports it."""
import ctypes as C
import fcntl
import os
import subprocess

import numpy as np

from marlgrid_amd import _native as N

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SOURCE = os.path.join(HERE, "mg_solve_dist.cpp")
INCLUDES = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "marlgrid_amd", "csrc")]
vp = C.c_void_p
_lib = None


def lib():
    """libmg_solve_dist.so, built on demand (one builder at a time, as hostemu_goal.lib())"""
    global _lib
    if _lib is None:
        out = os.path.join(HERE, "libmg_solve_dist.so")
        with open(os.path.join(HERE, ".build.lock"), "w") as lock:
            fcntl.flock(lock, fcntl.LOCK_EX)
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Wno-unused-function",
                                   "-Wno-unknown-pragmas", "-UNDEBUG"] + INCLUDES + [SOURCE, "-o", out])
        L = C.CDLL(out)
        L.sd_run.argtypes = [C.POINTER(N.Config), C.POINTER(N.State), vp, C.c_int, C.c_int, vp, vp, vp, C.c_int]
        L.sd_run.restype = C.c_int
        L.sd_scratch_bytes.argtypes = [C.c_int] * 4
        L.sd_scratch_bytes.restype = C.c_size_t
        _lib = L
    return _lib


def _p(a):
    return None if a is None else vp(a.ctypes.data)


def run(cfg, state, lanes=64, mask=None, max_doors=2, max_items=2, fill=-7, rc_want=0):
    """One emulated mg_solve_distance: -> (dist (B, n) int32, action (B, n) int8, exact (B,) uint8), each filled with `fill`
    where nothing was written"""
    B, n = cfg.B, cfg.n_agents
    dist = np.full((B, n), fill, np.int32)
    act = np.full((B, n), fill, np.int8)
    exact = np.full(B, fill & 0xFF, np.uint8)
    m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
    rc = lib().sd_run(C.byref(cfg), C.byref(state), _p(m), max_doors, max_items, _p(dist), _p(act), _p(exact), lanes)
    assert rc == rc_want, rc
    return dist, act, exact


class SolveCase(object):
    """A batch made by hand: grid (B, W, H) of ids into KINDS — rows (flags, reward_kind, color_idx, toggle_next, unlock_next) —,
    agents as (B, n) tuples (x, y, dir, flags, carry)"""
    DOOR = N.OF_IS_DOOR
    (WALL, GOAL, LAVA, FLOOR, OPEN_A, SHUT_A, LOCKED_A, OPEN_B, SHUT_B, LOCKED_B, KEY_A, KEY_B, BALL, BOX, STUCK,
     OPEN_TO_LAVA, SHUT_TO_LAVA) = range(1, 18)
    COL_A, COL_B = 1, 4
    KINDS = [(0, 0, 0, 0, 0), (0, 0, 0, 0, 0), (N.OF_CAN_OVERLAP | N.OF_ENDS_EPISODE, 1, 0, 0, 0),
             (N.OF_CAN_OVERLAP | N.OF_ENDS_EPISODE, 0, 0, 0, 0), (N.OF_CAN_OVERLAP, 0, 0, 0, 0),
             (N.OF_CAN_OVERLAP | DOOR | N.OF_SEE_BEHIND, 0, COL_A, 6, 0), (DOOR, 0, COL_A, 5, 0), (DOOR | N.OF_DOOR_LOCKED, 0, COL_A, 7, 6),
             (N.OF_CAN_OVERLAP | DOOR | N.OF_SEE_BEHIND, 0, COL_B, 9, 0), (DOOR, 0, COL_B, 8, 0), (DOOR | N.OF_DOOR_LOCKED, 0, COL_B, 10, 9),
             (N.OF_CAN_PICKUP | N.OF_IS_KEY, 0, COL_A, 0, 0), (N.OF_CAN_PICKUP | N.OF_IS_KEY, 0, COL_B, 0, 0),
             (N.OF_CAN_PICKUP, 0, COL_A, 0, 0), (N.OF_CAN_PICKUP | N.OF_IS_BOX, 0, COL_A, 0, 0),
             (DOOR, 0, COL_A, 15, 0),                                        # STUCK: a closed door that toggles to itself
             (N.OF_CAN_OVERLAP | N.OF_ENDS_EPISODE, 0, 0, 17, 0), (DOOR, 0, COL_A, 16, 0)]      # a door that opens into lava

    def __init__(self, grid, agents):
        grid = np.asarray(grid, np.uint8)
        B, W, H = grid.shape
        self.grid3 = grid
        self.stride = (W * H + 15) // 16 * 16
        self.grid = np.zeros((B, self.stride), np.uint8)
        self.grid[:, :W * H] = grid.reshape(B, -1)
        a = np.asarray(agents, np.uint64).reshape(B, -1, 5)
        self.rec = np.ascontiguousarray(a[..., 0] | (a[..., 1] << np.uint64(8)) | (a[..., 2] << np.uint64(16))
                                        | (a[..., 3] << np.uint64(24)) | (a[..., 4] << np.uint64(32)))
        self.obj = (N.ObjDesc * len(self.KINDS))()
        for i, (f, rk, col, tog, unl) in enumerate(self.KINDS):
            o = self.obj[i]
            o.flags, o.reward_kind, o.color_idx, o.toggle_next, o.unlock_next = f, rk, col, tog, unl
        self.cfg = N.Config()
        self.cfg.B, self.cfg.W, self.cfg.H, self.cfg.n_agents = B, W, H, self.rec.shape[1]
        self.cfg.cells_stride, self.cfg.n_obj = self.stride, len(self.KINDS)
        self.cfg.obj = C.addressof(self.obj)
        self.state = N.State()
        self.state.grid, self.state.agents = self.grid.ctypes.data, self.rec.ctypes.data

    @classmethod
    def kinds(cls):
        import solve_ref
        return solve_ref.Kinds(*zip(*cls.KINDS))
