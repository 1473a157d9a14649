"""The observation kernel specialised on demand, without a GPU: the rule that says which instantiation a configuration off the
table would get (marlgrid_amd/csrc/mg_render_pick.h: render_pick_ideal, through a g++ build of the header — tests/native/
mg_render_pick_ideal.cpp) over every configuration of the recorded table tests/golden/render_picks.npz and at hand-derived spot
values; mg_render_specialize in compile-only mode (hipRTC cross-compiles for gfx950 without a device) with its disk cache;
and the headers the library reads for hipRTC against the build id."""
import ctypes as C
import fcntl
import hashlib
import os
import subprocess
import sys
from math import gcd

import numpy as np
import pytest

from marlgrid_amd import _native as N
from test_render_pick import fill

HERE = os.path.dirname(os.path.abspath(__file__))
NATIVE = os.path.join(HERE, "native")
CSRC = os.path.join(os.path.dirname(HERE), "marlgrid_amd", "csrc")
PLAIN, ENCODE, EPISODE, DELTA = range(4)
LDS_MAX = 160 * 1024


@pytest.fixture(scope="module")
def ideal_lib():
    out = os.path.join(NATIVE, "libmg_render_pick_ideal.so")
    with open(os.path.join(NATIVE, ".build.lock"), "w") as lock:        # (one builder at a time, as tests/native/hostemu.py)
        fcntl.flock(lock, fcntl.LOCK_EX)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Wno-unused-function",
                               "-I", os.path.join(os.path.dirname(HERE), "include"), "-I", CSRC,
                               os.path.join(NATIVE, "mg_render_pick_ideal.cpp"), "-o", out])
    L = C.CDLL(out)
    assert L.ideal_sizeof_config() == C.sizeof(N.Config)
    return L


@pytest.fixture(scope="module")
def table():
    d = np.load(os.path.join(HERE, "golden", "render_picks.npz"))
    cols = [str(c) for c in d["cfg_cols"]]
    return {c: d["cfg"][:, i].astype(np.int64) for i, c in enumerate(cols)}


def rows_of(lib, cfgs, n):
    """(ideal, table) [n][4 wants][7: picked, vs, ts, wpb, v, rm, lds] and facts [n][4: big grid, fits(4, 0), fits(4, 2), gather trips]"""
    out = np.zeros((n, 4, 2, 7), np.int32)
    facts = np.zeros((n, 4), np.int32)
    lib.ideal_rows(cfgs, n, C.c_void_p(out.ctypes.data), C.c_void_p(facts.ctypes.data))
    return out[:, :, 0], out[:, :, 1], facts


def gather_period_ok(vs, ts):
    """GatherGeom's NT <= 4, as the issue states it: RB / gcd(16, RB) <= 256 with RB = 3 vs ts"""
    rb = 3 * vs * ts
    return rb // gcd(16, rb) <= 256


def test_render_pick_ideal_over_the_recorded_table(table, ideal_lib):
    n = len(table["B"])
    assert n >= 16776
    cfgs = (N.Config * n)()
    for i in range(n):
        fill(cfgs[i], table, i)
    ideal, tab, facts = rows_of(ideal_lib, cfgs, n)
    vs, ts = table["view_size"], table["tile_size"]
    # the family a configuration's tiles take, by the rule's text: gather where its period is short enough and the padded atlas
    # fits, the chunk raster at 8 / 16 / 32, assemble-and-stream (a run-time tile size) otherwise
    gather = np.array([t >= 5 and t % 8 != 0 and gather_period_ok(v, t) for v, t in zip(vs, ts)]) & (facts[:, 2] == 1)
    trips_ok = np.array([t >= 5 and t % 8 != 0 and gather_period_ok(v, t) for v, t in zip(vs, ts)])
    assert np.array_equal(trips_ok, (ts >= 5) & (ts % 8 != 0) & (facts[:, 3] <= 4)), "gather_trips <= 4 is not RB / gcd(16, RB) <= 256"
    chunk = np.isin(ts, (8, 16, 32))
    fam_ts = np.where(gather | chunk, ts, 0)
    fam_rm = np.where(gather, 2, 0)
    seen = 0
    for w in (PLAIN, ENCODE, EPISODE):
        I, T = ideal[:, w], tab[:, w]
        on = I[:, 0] == 1
        seen += int(on.sum())
        # where it answers: the view compiled in, the family's tile size and raster, the want's variant, a workgroup that fits
        assert (I[on, 1] == vs[on]).all() and (I[on, 2] == fam_ts[on]).all() and (I[on, 5] == fam_rm[on]).all()
        assert (I[on, 4] == (0, 16, 32)[w]).all()
        assert np.isin(I[on, 3], (4, 8, 16)).all() and ((I[on, 6] > 0) & (I[on, 6] <= LDS_MAX)).all()
        small = on & (table["B"] < 4096)
        assert (I[small, 3] == 4).all()
        assert (I[on & (vs > 9), 3] <= 8).all()
        # ... and it is not what the table already gives this want
        same = (T[:, 0] == 1) & (T[:, 1:3] == I[:, 1:3]).all(axis=1) & (T[:, 4:6] == I[:, 4:6]).all(axis=1)
        assert not (on & same).any()
        # never: 'prestige' agents, a grid read in place, an atlas in global memory (every V != 0 of the table's plain pick)
        P = tab[:, PLAIN]
        assert not (on & (table["prestige_mask"] != 0)).any()
        assert not (on & (facts[:, 0] == 1)).any()
        assert not (on & ((P[:, 0] == 0) | (P[:, 4] != 0))).any()
        assert not (on & (vs < 3)).any()
        # never where the table's pick for this want has the view and the family's tile size compiled in — whatever its workgroup
        has = (T[:, 0] == 1) & (T[:, 1] == vs) & (T[:, 2] == fam_ts) & (T[:, 5] == fam_rm)
        assert not (on & has).any()
        # ... and everywhere else that can be specialised, it answers (plain: nothing else is asked of the configuration)
        if w == PLAIN:
            can = (P[:, 0] == 1) & (P[:, 4] == 0) & (vs >= 3) & ~has
            assert np.array_equal(on, can), np.nonzero(on != can)[0][:5]
    assert (ideal[:, DELTA, 0] == 0).all()
    assert seen > 3000      # the table's sweep is mostly off-table shapes: the rule is not vacuous


def base_cfg(table, view, tile, B):
    i = int(np.nonzero((table["grid"] == 15) & (table["n_agents"] == 3) & (table["view_size"] == 13) & (table["tile_size"] == 4) &
                       (table["prestige_mask"] == 0) & (table["any_hide"] == 0) & (table["n_view"] == 0))[0][0])
    c = fill(N.Config(), table, i, B=B)
    c.view_size, c.tile_size = view, tile
    return c


# 3 agents on 15 x 15, derived from the rule by hand: view 13 at 4-pixel tiles is under the gather raster's 5 and off the chunk
# sizes: assemble-and-stream, a run-time tile size; 17 x 5: RB = 255, odd, a period of 255 chunks <= 256: gather — 8 waves at
# 8 192 envs because 17 > 9; 10 x 6: RB = 180, gcd 4, 45 chunks: gather; 11 x 8: the chunk raster; 21 x 5: RB = 315, a period of
# 315 chunks > 256: no gather cycle, assemble-and-stream; 6 x 8 with the encode: the table has <6, 8, ., 0, 0> but no + 16 of it;
# 7 x 8: the table's own headline shape.
SPOTS = [(13, 4, 64, PLAIN, (13, 0, 4, 0, 0)), (17, 5, 64, PLAIN, (17, 5, 4, 0, 2)), (17, 5, 8192, PLAIN, (17, 5, 8, 0, 2)),
         (10, 6, 64, PLAIN, (10, 6, 4, 0, 2)), (11, 8, 64, PLAIN, (11, 8, 4, 0, 0)), (21, 5, 64, PLAIN, (21, 0, 4, 0, 0)),
         (6, 8, 64, ENCODE, (6, 8, 4, 16, 0)), (7, 8, 64, PLAIN, None), (7, 8, 8192, PLAIN, None)]


@pytest.mark.parametrize("view,tile,B,want,expect", SPOTS)
def test_render_pick_ideal_spot_values(table, ideal_lib, view, tile, B, want, expect):
    cfgs = (N.Config * 1)(base_cfg(table, view, tile, B))
    ideal, _, _ = rows_of(ideal_lib, cfgs, 1)
    got = ideal[0, want]
    if expect is None:
        assert got[0] == 0
    else:
        assert got[0] == 1 and tuple(got[1:6]) == expect, got
        assert 0 < got[6] <= LDS_MAX


def spec_call(cfg, want, cache_dir):
    info = N.SpecInfo()
    rc = N.lib().mg_render_specialize(C.byref(cfg), want, N.SPEC_COMPILE_ONLY, b"gfx950", os.fsencode(cache_dir), None, C.byref(info))
    return rc, info.as_dict()


def test_compile_only_and_the_disk_cache(table, tmp_path):
    """view 13 at 4-pixel tiles for gfx950, no device: compiled, named as mg_render_kernel_name names kernels, no scratch; the
    code object is kept in the cache directory — a second call is a hit —, and a cache file cut to half is compiled again and
    replaced, never loaded"""
    cfg = base_cfg(table, 13, 4, 64)
    cache = str(tmp_path / "cache")
    rc, info = spec_call(cfg, N.WANT_PLAIN, cache)
    if rc == N.E_UNSUPPORTED and "libhiprtc" in info["reason"]:
        pytest.skip(info["reason"])
    assert rc == N.OK, info
    assert info["kernel_name"] == "mg::render_kernel<13, 0, 4, 0, 0>"
    assert (info["vs"], info["ts"], info["wpb"], info["v"], info["rm"]) == (13, 0, 4, 0, 0)
    assert info["code_bytes"] > 0 and info["scratch_bytes"] == 0 and 0 < info["lds_bytes"] <= LDS_MAX
    assert info["cache_hit"] == 0 and info["compile_seconds"] > 0
    files = [f for f in os.listdir(cache) if f.endswith(".co")]
    assert len(files) == 1 and "gfx950_13_0_4_0_0" in files[0] and N.lib().mg_build_info().decode().split()[-1] in files[0]
    assert not [f for f in os.listdir(cache) if ".tmp" in f]
    path = os.path.join(cache, files[0])
    whole = open(path, "rb").read()
    assert len(whole) > info["code_bytes"]
    rc, again = spec_call(cfg, N.WANT_PLAIN, cache)
    assert rc == N.OK and again["cache_hit"] != 0 and again["compile_seconds"] == 0
    assert again["code_bytes"] == info["code_bytes"] and again["kernel_name"] == info["kernel_name"]
    # the cache file alone (a fresh process has no code in memory): read and validated in a child; then cut to half
    child = ("import ctypes as C, os, sys; sys.path[:0] = [%r, %r]\n"
             "from marlgrid_amd import _native as N\n"
             "import test_specialize_host as T, numpy as np\n"
             "d = np.load(os.path.join(T.HERE, 'golden', 'render_picks.npz'))\n"
             "table = {str(c): d['cfg'][:, i].astype(np.int64) for i, c in enumerate(d['cfg_cols'])}\n"
             "rc, info = T.spec_call(T.base_cfg(table, 13, 4, 64), N.WANT_PLAIN, %r)\n"
             "print('RESULT', rc, info['cache_hit'], info['code_bytes'], info['scratch_bytes'])\n"
             % (os.path.dirname(HERE), HERE, cache))
    def run_child():
        out = subprocess.run([sys.executable, "-c", child], capture_output=True, text=True, check=True).stdout
        return [int(x) for x in [l for l in out.splitlines() if l.startswith("RESULT")][0].split()[1:]]
    assert run_child() == [N.OK, 2, info["code_bytes"], 0]
    with open(path, "wb") as f:
        f.write(whole[:len(whole) // 2])
    assert run_child() == [N.OK, 0, info["code_bytes"], 0]        # compiled again: no hit
    assert open(path, "rb").read() == whole                        # ... and the file replaced by a whole one


def test_unsupported_answers_carry_a_reason(table):
    """nothing is compiled for the table's own shapes, for 'prestige' agents or for a bad call; the struct is MgSpecInfo"""
    L = N.lib()
    assert L.mg_spec_info_struct_size() == C.sizeof(N.SpecInfo)
    info = N.SpecInfo()
    cfg = base_cfg(table, 7, 8, 64)
    assert L.mg_render_specialize(C.byref(cfg), 0, N.SPEC_COMPILE_ONLY, b"gfx950", None, None, C.byref(info)) == N.E_UNSUPPORTED
    assert info.table_is_ideal == 1 and b"table" in info.reason and info.kernel_name == b"mg::render_kernel<7, 8, 4, 0, 0>"
    cfg = base_cfg(table, 13, 4, 64)
    cfg.prestige_mask = 1
    assert L.mg_render_specialize(C.byref(cfg), 0, N.SPEC_COMPILE_ONLY, b"gfx950", None, None, C.byref(info)) == N.E_UNSUPPORTED
    assert info.table_is_ideal == 0 and b"prestige" in info.reason
    cfg.prestige_mask = 0
    assert L.mg_render_specialize(C.byref(cfg), 3, N.SPEC_COMPILE_ONLY, b"gfx950", None, None, C.byref(info)) == N.E_ARG
    assert L.mg_render_specialize(C.byref(cfg), 0, N.SPEC_COMPILE_ONLY, None, None, None, C.byref(info)) == N.E_ARG     # compile-only needs the arch
    assert L.mg_render_specialize(C.byref(cfg), 0, N.SPEC_COMPILE_ONLY, b"gfx950 -x", None, None, C.byref(info)) == N.E_ARG
    assert L.mg_render_spec_release(None) == N.OK
    assert L.mg_step_render_spec(None, C.byref(cfg), None, None, 8, None, None, None, None, None, None) == N.E_ARG


def test_rtc_sources_hash_to_the_build_id():
    """the headers the library hands to hipRTC (read from beside it, accepted by checksum) are the ones it was built from: with the
    library's other sources, in the Makefile's order, they hash to the src-... id of mg_build_info"""
    L = N.lib()
    if os.path.abspath(N._path) != os.path.abspath(N.LIB_PATH):
        pytest.skip("another build of the library is bound")
    n = L.mg_rtc_source(-1, None, None, None)
    carried = {}
    for i in range(n):
        name, text, length = C.c_char_p(), C.c_void_p(), C.c_int32()
        assert L.mg_rtc_source(i, C.byref(name), C.byref(text), C.byref(length)) == n
        carried[name.value.decode()] = C.string_at(text.value, length.value)
    listed = subprocess.check_output(["make", "-s", "-C", CSRC, "print-sources"], text=True).split()
    headers = [f for f in listed if f.endswith(".h")]
    assert sorted(os.path.basename(f) for f in headers) == sorted(carried) and "mg_render_kernel.h" in carried
    h = hashlib.sha256()
    for f in listed:
        h.update(carried[os.path.basename(f)] if f.endswith(".h") else open(os.path.join(CSRC, f), "rb").read())
    assert "src-" + h.hexdigest()[:12] == L.mg_build_info().decode().split()[-1]
    for f in headers:      # (and they are the files of this tree)
        assert carried[os.path.basename(f)] == open(os.path.join(CSRC, f), "rb").read(), f
