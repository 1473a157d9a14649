"""The env step's LDS layouts and the view map (marlgrid_amd/csrc/mg_step_layout.h, mg_core.h), compiled for the host.

The kernels that host the step carve their scratch with these functions and their launchers ask for these byte counts;
the host harness (tests/native) steps every scenario on buffers of exactly these sizes, garbage-filled, with a guard band
behind them.  Here the geometry itself: no two columns overlap, none leaves the byte count, each is aligned for the
accesses made to it; the workgroup-size rule of mg_step; and view_map / view_world against the reference's rule for
EVERY view size, offset, heading and view cell.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "native"))

LANE = ("obj", "rec", "head", "act", "fb", "ord", "oflags")
FUSED = ("rec", "head", "act", "pflag", "ordp", "psc")
# what the accesses to a column need: 16-byte pieces into the object table (stage_obj_tables), u64 records, u32 words
ALIGN = dict(obj=16, rec=8, head=4, psc=4)
N_AGENTS = range(1, 33)


@pytest.fixture(scope="module")
def L():
    import hostemu
    lib = hostemu.lib()
    lib.emu_reset_scratch_bytes.restype = C.c_int64
    lib.emu_view_map.restype = C.c_uint32
    return lib


def _columns(L, fused, n, S):
    ext = np.zeros((8, 2), np.int64)
    total = C.c_int64(0)
    c = L.emu_step_columns(int(fused), n, S, C.c_void_p(ext.ctypes.data), C.byref(total))
    names = FUSED if fused else LANE
    assert c == len(names)
    return dict(zip(names, ext[:c].tolist())), total.value


def _check_geometry(cols, total, what):
    for name, (lo, hi) in cols.items():
        assert 0 <= lo < hi <= total, (what, name, lo, hi, total)
        assert lo % ALIGN.get(name, 1) == 0, (what, name, lo)
    spans = sorted(cols.values())
    for (_, hi), (lo, _) in zip(spans, spans[1:]):
        assert hi <= lo, (what, cols)
    return spans


@pytest.mark.parametrize("S", [1, 8, 10, 64, 85, 256])
def test_lane_layout_geometry(L, S):
    """step_kernel (S = 64, 256), the step phase of encode_views_kernel (S = envs per workgroup: 8, 10, 85 ...), the
    host harness (S = 1)"""
    for n in N_AGENTS:
        cols, total = _columns(L, False, n, S)
        spans = _check_geometry(cols, total, (n, S))
        # exactly the columns, nothing between them or behind: the byte count is what the launchers ask for
        assert spans[0][0] == 0 and spans[-1][1] == total and sum(hi - lo for lo, hi in spans) == total
        assert cols["rec"][1] - cols["rec"][0] == 8 * n * S and cols["obj"][1] - cols["obj"][0] == 256 * 32


def test_fused_layout_geometry(L):
    """the obs kernel's fused step, S = 8: the byte count is the sum render_scratch_layout has always reserved"""
    for n in N_AGENTS:
        cols, total = _columns(L, True, n, 8)
        _check_geometry(cols, total, n)
        assert total == n * 64 + 512 + 24 * n + 32
        assert cols["rec"][0] == 0 and cols["psc"][1] == total


def test_reset_scratch_bytes(L):
    for n in N_AGENTS:
        assert L.emu_reset_scratch_bytes(n, 256) == n * 256 * 8 + 256


def test_step_workgroup_rule(L):
    """256 lanes exactly for B > 131 072 and at most 13 agents — the bound of 3072 n + 24 832 <= 65 536, the 12 bytes
    per agent and lane the rule was written for (the layout itself takes 11: 2816 n + 24 832)"""
    for n in N_AGENTS:
        for B in (1, 64, 4096, 131071, 131072, 131073, 262144, 1 << 24):
            assert L.emu_step_lanes(n, B) == (256 if B > 131072 and n <= 13 else 64), (n, B)
        _, total = _columns(L, False, n, 256)
        assert total == 2816 * n + 24832
        if L.emu_step_lanes(n, 1 << 20) == 256:
            assert total <= 65536


def _reference_world(x, y, d, vs, off):
    """the reference's rule as the oracle states it (mg_oracle.c: mgo_view / rotate_grid_i32): the window's corner
    topX / topY by heading, rotated rot_k = dir + 1 times; cell [i = va][j = vb] -> world (wx, wy), int arrays [vs][vs]"""
    if d == 0:
        tx, ty = x - off, y - vs // 2
    elif d == 1:
        tx, ty = x - vs // 2, y - off
    elif d == 2:
        tx, ty = x - vs + 1 + off, y - vs // 2
    else:
        tx, ty = x - vs // 2, y - vs + 1 + off
    i, j = np.meshgrid(np.arange(vs), np.arange(vs), indexing="ij")
    r = (d + 1) % 4
    if r == 3:
        si, sj = j, vs - 1 - i
    elif r == 1:
        si, sj = vs - 1 - j, i
    elif r == 2:
        si, sj = vs - 1 - i, vs - 1 - j
    else:
        si, sj = i, j
    return tx + si, ty + sj


def test_view_map_every_case(L):
    x, y = 100, 90
    cases = 0
    for vs in range(1, 32):
        out = np.zeros((vs, vs, 2), np.int32)
        for off in range(vs):
            for d in range(4):
                w0 = L.emu_view_map(x, y, d, vs, off)
                L.emu_view_world(C.c_uint32(w0), vs, C.c_void_p(out.ctypes.data))
                wx, wy = _reference_world(x, y, d, vs, off)
                assert np.array_equal(out[..., 0], wx) and np.array_equal(out[..., 1], wy), (vs, off, d)
                cases += vs * vs
    assert cases == 984064
