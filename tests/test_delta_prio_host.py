"""The delta launch's wave priority without a GPU: delta_wave_prio (marlgrid_amd/csrc/mg_step_layout.h) — the s_setprio level of
a wave that has finished `done` of the `total` view groups of its whole run —, the g++ build of the very text the kernel calls
(tests/native/mg_delta_prio.cpp).  For every total 1 .. 64: a level 0 .. 3; 3 with nothing done; never rising with progress;
3 - min(3, 4 done / total); at the bench shape's four groups exactly 3, 2, 1, 0; a wave with one group keeps 3."""
import ctypes as C
import fcntl
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
NATIVE = os.path.join(HERE, "native")
CSRC = os.path.join(os.path.dirname(HERE), "marlgrid_amd", "csrc")
TOTALS = range(1, 65)


@pytest.fixture(scope="module")
def prio():
    out = os.path.join(NATIVE, "libmg_delta_prio.so")
    with open(os.path.join(NATIVE, ".build.lock"), "w") as lock:        # (one builder at a time, as tests/native/hostemu.py)
        fcntl.flock(lock, fcntl.LOCK_EX)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Wno-unused-function",
                               "-I", os.path.join(os.path.dirname(HERE), "include"), "-I", CSRC,
                               os.path.join(NATIVE, "mg_delta_prio.cpp"), "-o", out])
    L = C.CDLL(out)
    L.delta_prio.argtypes = [C.c_int, C.c_int]
    L.delta_prio.restype = C.c_int
    return L.delta_prio


def test_range(prio):
    for total in TOTALS:
        for done in range(total + 1):
            assert 0 <= prio(done, total) <= 3, (done, total)


def test_three_with_nothing_done(prio):
    for total in TOTALS:
        assert prio(0, total) == 3, total


def test_non_increasing(prio):
    for total in TOTALS:
        levels = [prio(done, total) for done in range(total + 1)]
        assert all(a >= b for a, b in zip(levels, levels[1:])), (total, levels)


def test_scales_with_the_total(prio):
    for total in TOTALS:
        for done in range(total + 1):
            assert prio(done, total) == 3 - min(3, 4 * done // total), (done, total)


def test_bench_shape_steps_3_2_1_0(prio):
    assert [prio(done, 4) for done in range(4)] == [3, 2, 1, 0]


def test_one_group_keeps_three(prio):
    assert prio(0, 1) == 3
