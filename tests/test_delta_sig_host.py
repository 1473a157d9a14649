"""The compact signature of mg_step_render_delta without a GPU: the code <-> entry mapping and the slot arithmetic of
marlgrid_amd/csrc/mg_step_layout.h (delta_sig_*), the very functions the kernel and the launcher call, built with g++
(tests/native/mg_delta_sig.cpp).

A tmap entry of the delta instantiations is (orientation * n_tiles + tile) * tile_dwords, tile_dwords = 8 * 8 * 3 / 4 = 48 at the
8-pixel tiles they are compiled for; its code is the quotient, one byte, 0xFF is "no tile"."""
import ctypes as C
import fcntl
import os
import subprocess

import pytest

from marlgrid_amd import _native as N

HERE = os.path.dirname(os.path.abspath(__file__))
NATIVE = os.path.join(HERE, "native")
CSRC = os.path.join(os.path.dirname(HERE), "marlgrid_amd", "csrc")
TILE_DWORDS = 8 * 8 * 3 // 4
VIEW = 7


@pytest.fixture(scope="module")
def sig_lib():
    out = os.path.join(NATIVE, "libmg_delta_sig.so")
    with open(os.path.join(NATIVE, ".build.lock"), "w") as lock:        # (one builder at a time, as tests/native/hostemu.py)
        fcntl.flock(lock, fcntl.LOCK_EX)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Wno-unused-function",
                               "-I", os.path.join(os.path.dirname(HERE), "include"), "-I", CSRC,
                               os.path.join(NATIVE, "mg_delta_sig.cpp"), "-o", out])
    L = C.CDLL(out)
    for f in (L.sig_env_bytes, L.sig_slot, L.sig_alloc_bytes):
        f.restype = C.c_longlong
    L.sig_slot.argtypes = [C.c_longlong, C.c_int, C.c_int]
    for f in (L.sig_code, L.sig_entry, L.sig_none):
        f.restype = C.c_uint
    return L


def test_every_code_round_trips(sig_lib):
    L = sig_lib
    none = L.sig_none()
    assert none == 0xFF and L.sig_slot_bytes() == 64
    for code in range(none):                                    # 0 .. 254: every code a compact configuration can have
        entry = L.sig_entry(code, TILE_DWORDS)
        assert entry == code * TILE_DWORDS and entry < 1 << 16   # (a tmap entry is 16 bits)
        assert L.sig_code(entry, TILE_DWORDS) == code
    # ... and every entry such a configuration can draw has a code of its own below 0xFF
    for n_tiles in (1, 17, 28, 53, 63):
        assert L.sig_compact(n_tiles, 3, VIEW) == 1
        codes = {L.sig_code(vt * TILE_DWORDS, TILE_DWORDS) for vt in range(4 * n_tiles)}
        assert codes == set(range(4 * n_tiles)) and max(codes) < none


def test_none_never_equals_a_tile(sig_lib):
    """0xFF as an ENTRY (what phase 5 compares) is no entry of a compact configuration; the host's 0xFF fill therefore makes
    every band count as changed"""
    L = sig_lib
    none_entry = L.sig_entry(L.sig_none(), TILE_DWORDS)
    for n_tiles in range(1, 64):
        assert L.sig_compact(n_tiles, 3, VIEW) == 1
        assert none_entry not in {vt * TILE_DWORDS for vt in range(4 * n_tiles)}
    assert none_entry > (4 * 63 - 1) * TILE_DWORDS
    # one more tile and the codes no longer fit: the configuration keeps the 16-bit entries
    for n_tiles in (64, 82, 149, 200):
        assert L.sig_compact(n_tiles, 3, VIEW) == 0


@pytest.mark.parametrize("n", [1, 2, 3])
def test_slots_are_aligned_and_inside_the_allocation(sig_lib, n):
    L = sig_lib
    per_env = L.sig_alloc_bytes(n, VIEW)
    assert per_env == N.delta_sig_bytes(n, VIEW)
    assert L.sig_compact(28, n, VIEW) == 1
    assert L.sig_env_bytes(n) == n * 64 <= per_env
    assert VIEW * VIEW <= L.sig_slot_bytes()
    B = 4099
    seen = set()
    for e in (0, 1, 2, 66, 67, 4098):
        for v in range(n):
            o = L.sig_slot(e, v, n)
            assert o % 64 == 0 and o not in seen
            seen.add(o)
            assert o == e * L.sig_env_bytes(n) + v * 64
            assert e * L.sig_env_bytes(n) <= o and o + 64 <= (e + 1) * L.sig_env_bytes(n)    # inside the env's own run ...
            assert o + 64 <= (e + 1) * per_env <= B * per_env                                 # ... and inside the allocation
    # whole slots are what a launch reads, 16 bytes a lane: a staged batch of 8 envs is at most 3 x 64 requests
    assert 8 * L.sig_env_bytes(n) // 16 <= 3 * 64
