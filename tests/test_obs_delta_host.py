"""obs_delta without a GPU: the launcher's pick for mg_step_render_delta — the g++ build of marlgrid_amd/csrc/mg_render_pick.h
(tests/native/mg_obs_delta.cpp) — over every configuration of the recorded table tests/golden/render_picks.npz: the fourth
want is answered for exactly view 7 at 8-pixel tiles, 16- or 4-wave workgroups, one view group, at most three agents, no
'prestige' agent, grid and atlas in LDS — i.e. where the plain pick is render_kernel<7, 8, 16 | 4, 0, 0> — with the plain pick's
workgroup and LDS bytes, and with false everywhere else; every answer is an entry of MG_RENDER_DELTA, none of MG_RENDER_ALL;
the first three wants still reproduce the table (tests/test_render_pick.py does that: run here on the same library build).
Then the host's own bookkeeping, on a dry env: who invalidates.

(The band mask itself is a lane-per-band loop inside the kernel's phase 5, not a function a host compiler could share: it is
held by tests/test_hip_obs_delta.py on the GPU.)"""
import ctypes as C
import fcntl
import os
import subprocess

import numpy as np
import pytest

from marlgrid_amd import _native as N

import test_render_pick as TRP

HERE = os.path.dirname(os.path.abspath(__file__))
NATIVE = os.path.join(HERE, "native")
CSRC = os.path.join(os.path.dirname(HERE), "marlgrid_amd", "csrc")


@pytest.fixture(scope="module")
def delta_lib():
    out = os.path.join(NATIVE, "libmg_obs_delta.so")
    with open(os.path.join(NATIVE, ".build.lock"), "w") as lock:        # (one builder at a time, as tests/native/hostemu.py)
        fcntl.flock(lock, fcntl.LOCK_EX)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-Wno-unused-function",
                               "-I", os.path.join(os.path.dirname(HERE), "include"), "-I", CSRC,
                               os.path.join(NATIVE, "mg_obs_delta.cpp"), "-o", out])
    L = C.CDLL(out)
    assert L.delta_sizeof_config() == C.sizeof(N.Config)
    return L


@pytest.fixture(scope="module")
def table():
    d = np.load(os.path.join(HERE, "golden", "render_picks.npz"))
    cols = [str(c) for c in d["cfg_cols"]]
    return {c: d["cfg"][:, i] for i, c in enumerate(cols)}, d["pick"].reshape(len(d["cfg"]), -1)


def test_the_fourth_want_is_appended(delta_lib):
    assert delta_lib.delta_want_value() == 3


def test_delta_list_is_its_own(delta_lib):
    buf = (C.c_int32 * (5 * 16))()
    n = delta_lib.delta_list(buf, 16)
    listed = {tuple(buf[5 * k:5 * k + 5]) for k in range(n)}
    assert listed == {(7, 8, 16, 64, 0), (7, 8, 4, 64, 0)}
    P = TRP.load_pick_lib()
    big = (C.c_int32 * (5 * 256))()
    k = P.pick_list(big, 256)
    assert not listed & {tuple(big[5 * j:5 * j + 5]) for j in range(k)}


def test_delta_pick_over_the_recorded_table(delta_lib, table):
    cfg, pick = table
    n = len(pick)
    cfgs = (N.Config * n)()
    for i in range(n):
        TRP.fill(cfgs[i], cfg, i)
    out = np.zeros((n, 7), np.int32)
    delta_lib.delta_rows(cfgs, n, C.c_void_p(out.ctypes.data))
    plain = pick[:, 2:9]                        # picked, vs, ts, wpb, v, rm, lds of the plain launch
    shape = (plain[:, 0] == 1) & (plain[:, 1] == 7) & (plain[:, 2] == 8) & (plain[:, 4] == 0) & (plain[:, 5] == 0)
    assert set(plain[shape, 3].tolist()) == {4, 16}
    want = shape & (cfg["n_view"] == 0) & (cfg["n_agents"] <= 3) & (cfg["prestige_mask"] == 0)
    assert want.sum() >= 20 and (shape & ~want).sum() >= 20, (want.sum(), (shape & ~want).sum())
    assert np.array_equal(out[:, 0] == 1, want), np.nonzero((out[:, 0] == 1) != want)[0][:10]
    got = out[want]
    assert (got[:, 1] == 7).all() and (got[:, 2] == 8).all() and (got[:, 4] == 64).all() and (got[:, 5] == 0).all()
    assert np.array_equal(got[:, 3], plain[want, 3])        # the plain launch's workgroup ...
    assert np.array_equal(got[:, 6], plain[want, 6])        # ... and not a byte of LDS more


def test_first_three_wants_unchanged(table):
    TRP.test_render_pick_answers_the_recorded_table(table, TRP.load_pick_lib())


def test_library_answers_unsupported_without_launching(table):
    """the C entry point on an empty batch: every check is made, nothing is launched"""
    cfg, pick = table
    L = N.lib()
    keep = C.create_string_buffer(64)
    p = (C.addressof(keep) + 15) & ~15
    st = N.State(*([p] * 10))
    c = N.Config()
    plain = pick[:, 2:9]
    shape = (plain[:, 0] == 1) & (plain[:, 1] == 7) & (plain[:, 2] == 8) & (plain[:, 4] == 0) & (plain[:, 5] == 0)
    want = shape & (cfg["n_agents"] <= 3) & (cfg["prestige_mask"] == 0)
    rows = [i for i in range(len(pick)) if cfg["n_view"][i] == 0]
    rows = rows[::7] + [i for i in rows if want[i]][:50]
    seen = set()
    for i in rows:
        TRP.fill(c, cfg, i, B=0)
        rc = L.mg_step_render_delta(C.byref(c), C.byref(st), p, 8, p, None, p, p, N.DELTA_FORCE, None)
        assert rc == (N.OK if want[i] else N.E_UNSUPPORTED), (i, rc)
        seen.add(rc)
    assert seen == {N.OK, N.E_UNSUPPORTED}
    TRP.fill(c, cfg, rows[-1], B=0)
    assert L.mg_step_render_delta(C.byref(c), C.byref(st), p, 8, p, None, p, None, 0, None) == N.E_ARG        # no signature
    assert L.mg_step_render_delta(C.byref(c), C.byref(st), p, 8, p, None, p, p + 2, 0, None) == N.E_ARG       # misaligned
    assert L.mg_step_render_delta(C.byref(c), C.byref(st), p, 8, p, None, p, p, 2, None) == N.E_ARG           # unknown flag


def test_sig_bytes():
    assert N.delta_sig_bytes(3, 7) == 304
    assert N.delta_sig_bytes(1, 7) == 112


def test_obs_delta_keyword():
    from marlgrid_amd.envs import make
    with pytest.raises(ValueError):
        make("MarlGrid-3AgentCluttered15x15-v0", batch_size=2, obs_delta="yes", _dry=True)
    for v in ("auto", True, False):
        env = make("MarlGrid-3AgentCluttered15x15-v0", batch_size=2, obs_delta=v, _dry=True)
        assert env.obs_delta is v or env.obs_delta == v
        env.invalidate_obs()            # (a dry env has no ring: nothing to do, no error)
