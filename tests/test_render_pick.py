"""Which instantiation of mg::render_kernel a configuration gets (marlgrid_amd/csrc/mg_render_pick.h: render_pick) against a
recorded table, tests/golden/render_picks.npz: the launcher's answers for the plain launch, for mg_step_render_encode and for
mg_step_render_ep, "does not fit LDS" and "no such instantiation" included, recorded from the library before the rules moved
into that header — which configuration gets which instantiation is not to change by accident.  Two halves: the header itself,
built with g++ (tests/native), on every row and all three wants; and the built library's entry points (mg_render_kernel_name, mg_render_obs_lds_bytes, the return codes of the two fused steps on
an empty batch).  No GPU.

The table: `cfg` [rows][cfg_cols] and `pick` [rows][2 + 3 * 7]: mg_render_kernel_name's return (generic bits, or < 0),
mg_render_obs_lds_bytes, then per want (plain, encode, episode) picked / vs / ts / wpb / v / rm / lds.  Its sweep: every view
3 ... 31 x tile 4 ... 12, 16, 32, 33 x B 4095 / 4096 x no / one 'prestige' agent on 15 x 15 with three agents; around the shapes
(7,8) (9,8) (11,8) (7,5) (7,11) (7,16) (5,6) (13,5) grids 15 ... 255 x 1 ... 32 agents x a view group of one / all x
hide_item_types x 8 / 100 / 250 object kinds (n_tiles follows: some atlases stay in global memory) x both B x 'prestige';
32-pixel tiles with an atlas of 4 / 7 / 11 tiles (small enough for LDS); views 1 and 2 (a run-time view that is none of the
fused shapes); and 62 configurations, found by search, whose fused encode is refused because its table does not fit beside FOUR
waves of scratch although a 16- or 8-wave workgroup's leaner layout would leave room (each at its B and at 4 095)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from marlgrid_amd import _native as N

HERE = os.path.dirname(os.path.abspath(__file__))
WANTS = ("plain", "encode", "episode")

# Instantiations of the product build that no configuration reaches: the 8-wave workgroups of the 'prestige' shapes.  The rules
# take them where 12 waves of scratch do not fit next to the atlas but only ask when choose_wpb said 16 — and where 16 waves of
# the smallest layout fit, 12 do.  They are what MG_RENDER_WPB=8 gets from the measurement build (tools/ab_offpath.py); they
# stay in the product build so that its code object is what it was.
UNREACHED = {(7, 8, 8, 9, 0), (7, 0, 8, 9, 0), (7, 5, 8, 9, 2), (7, 11, 8, 9, 2)}


@pytest.fixture(scope="module")
def table():
    d = np.load(os.path.join(HERE, "golden", "render_picks.npz"))
    cols = [str(c) for c in d["cfg_cols"]]
    cfg = {c: d["cfg"][:, i] for i, c in enumerate(cols)}
    return cfg, d["pick"].reshape(len(d["cfg"]), -1)


_PICK_LIB = None


def load_pick_lib():
    """the g++ build of mg_render_pick.h (tests/native/mg_render_pick.cpp)"""
    global _PICK_LIB
    if _PICK_LIB is None:
        import fcntl
        native = os.path.join(HERE, "native")
        with open(os.path.join(native, ".build.lock"), "w") as lock:       # (one builder at a time: tests/native/hostemu.py)
            fcntl.flock(lock, fcntl.LOCK_EX)
            subprocess.check_call(["make", "-s", "-C", native, "libmg_render_pick.so"])
        L = C.CDLL(os.path.join(native, "libmg_render_pick.so"))
        assert L.pick_sizeof_config() == C.sizeof(N.Config)
        _PICK_LIB = L
    return _PICK_LIB


@pytest.fixture(scope="module")
def pick_lib():
    return load_pick_lib()


_KEEP = C.create_string_buffer(64)       # what the never-dereferenced pointers of a config and a state point at


def fill(c, cfg, i, B=None):
    """row i as an MgConfig the C ABI's argument checks accept (nothing of it is ever read on a device)"""
    g = int(cfg["grid"][i])
    c.B = int(cfg["B"][i]) if B is None else B
    c.W = c.H = g
    c.cells_stride = (g * g + 15) // 16 * 16
    for f in ("n_agents", "view_size", "tile_size", "n_obj", "n_tiles", "n_view", "prestige_mask", "any_hide"):
        setattr(c, f, int(cfg[f][i]))
    c.max_steps, c.spawn_x1, c.spawn_y1, c.spawn_max_tries = 1, g, g, 1
    c.obj = c.atlas = C.addressof(_KEEP)
    return c


def test_table_covers_every_instantiation(table, pick_lib):
    cfg, pick = table
    assert len(pick) >= 5000
    buf = (C.c_int32 * (5 * 256))()
    n = pick_lib.pick_list(buf, 256)
    assert 0 < n <= 256
    listed = {tuple(buf[5 * k:5 * k + 5]) for k in range(n)}
    assert len(listed) == n, "an instantiation is listed twice"
    picked = set()
    for w in range(3):
        rows = pick[pick[:, 2 + 7 * w] == 1]
        picked |= {tuple(r) for r in rows[:, 3 + 7 * w:8 + 7 * w].tolist()}
    assert picked <= listed, sorted(picked - listed)         # a pick the list lacks would launch nothing
    assert UNREACHED <= listed
    assert listed - picked == UNREACHED, sorted((listed - picked) ^ UNREACHED)
    # rows the launcher turns down are rows too
    assert (pick[:, 2] == 0).any() and (pick[:, 9] == 0).any() and (pick[:, 16] == 0).any()


def test_render_pick_answers_the_recorded_table(table, pick_lib):
    cfg, pick = table
    n = len(pick)
    cfgs = (N.Config * n)()
    for i in range(n):
        fill(cfgs[i], cfg, i)
    out = np.zeros((n, 3, 7), np.int32)
    min_lds = np.zeros(n, np.int32)
    pick_lib.pick_rows(cfgs, n, C.c_void_p(out.ctypes.data), C.c_void_p(min_lds.ctypes.data))
    assert np.array_equal(min_lds, pick[:, 1])
    want = pick[:, 2:].reshape(n, 3, 7)
    for w, name in enumerate(WANTS):
        bad = np.nonzero((out[:, w] != want[:, w]).any(axis=1))[0]
        assert len(bad) == 0, (name, len(bad), {k: int(v[bad[0]]) for k, v in cfg.items()}, out[bad[0], w], want[bad[0], w])
    # every pick is an entry of MG_RENDER_ALL: the launcher's lookup finds it
    buf = (C.c_int32 * (5 * 256))()
    k = pick_lib.pick_list(buf, 256)
    listed = {tuple(buf[5 * j:5 * j + 5]) for j in range(k)}
    got = {tuple(r) for r in out[out[:, :, 0] == 1][:, 1:6].tolist()}
    assert got <= listed, sorted(got - listed)


def test_library_answers_the_recorded_table(table):
    cfg, pick = table
    L = N.lib()
    st = N.State(*([C.addressof(_KEEP)] * 10))
    p = C.addressof(_KEEP)
    c = N.Config()
    name = C.create_string_buffer(96)
    for i in range(len(pick)):
        fill(c, cfg, i)
        bits = L.mg_render_kernel_name(C.byref(c), name, len(name))
        assert bits == pick[i, 0], (i, bits)
        if pick[i, 2]:
            assert name.value.decode() == "mg::render_kernel<%d, %d, %d, %d, %d>" % tuple(pick[i, 3:8]), i
        else:
            assert bits == N.E_LAUNCH and name.value == b"", i
        assert L.mg_render_obs_lds_bytes(C.byref(c)) == pick[i, 1], i
        if cfg["n_view"][i] != 0:
            continue
        # the fused steps on an empty batch: every check is made, nothing is launched
        fill(c, cfg, i, B=0)
        rc = L.mg_step_render_encode(C.byref(c), C.byref(st), p, 8, p, None, p, p, None)
        assert rc == (N.OK if pick[i, 9] else N.E_UNSUPPORTED), (i, rc)
        rc = L.mg_step_render_ep(C.byref(c), C.byref(st), p, 8, p, None, p, C.byref(N.Episode()), None)
        assert rc == (N.OK if pick[i, 16] else N.E_UNSUPPORTED), (i, rc)
