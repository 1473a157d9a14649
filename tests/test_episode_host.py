"""Episode boundaries under auto-reset: what the host side answers without a device — the MgEpisode mirror, the argument
checks of the mg_*_ep entry points, the `auto_reset` / `episode_info` constructor arguments."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from marlgrid_amd import _native as N  # noqa: E402


def test_episode_struct_size_matches_the_binding():
    L = N.lib()
    assert L.mg_episode_struct_size() == C.sizeof(N.Episode) == 40
    assert [f[0] for f in N.Episode._fields_] == ["reset_mode", "reserved0", "ep_return", "out_return", "out_length", "out_flags"]
    assert (N.EPF_TERMINATED, N.EPF_TRUNCATED, N.EPF_RESET) == (1, 2, 4)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "marlgrid_hip.h")).read()
    for name, v in (("MG_EPF_TERMINATED", 1), ("MG_EPF_TRUNCATED", 2), ("MG_EPF_RESET", 4)):
        assert "#define %s %d" % (name, v) in hdr


def _calls(L, ep, prog):
    """the three _ep calls with NOTHING valid but `ep` / the program pointer: an argument error of `ep` is answered first"""
    cfg, st = N.Config(), N.State()
    p = None if prog is None else C.byref(prog)
    e = None if ep is None else C.byref(ep)
    return [L.mg_step_ep(C.byref(cfg), C.byref(st), None, 8, None, p, e, None),
            L.mg_step_render_ep(C.byref(cfg), C.byref(st), None, 8, None, p, None, e, None),
            L.mg_step_encode_views_ep(C.byref(cfg), C.byref(st), None, 8, None, p, None, e, None)]


def test_ep_entry_points_check_their_arguments_without_a_device():
    L = N.lib()
    prog = N.GenProgram()
    one = np.zeros(4, np.float64)
    bad_mode = N.Episode(2, 0, None, None, None, None)
    assert _calls(L, bad_mode, prog) == [N.E_ARG] * 3
    assert _calls(L, N.Episode(-1, 0, None, None, None, None), prog) == [N.E_ARG] * 3
    next_without_program = N.Episode(N.RESET_NEXT_STEP, 0, None, None, None, None)
    assert _calls(L, next_without_program, None) == [N.E_ARG] * 3
    out_without_acc = N.Episode(N.RESET_SAME_STEP, 0, None, one.ctypes.data, None, None)
    assert _calls(L, out_without_acc, prog) == [N.E_ARG] * 3
    # (a valid MgEpisode with an invalid config is still an argument error — of the config)
    assert _calls(L, N.Episode(N.RESET_SAME_STEP, 0, one.ctypes.data, one.ctypes.data, None, None), None) == [N.E_ARG] * 3


def _dry(**kw):
    import product_envs
    return product_envs.build("MarlGrid-2AgentEmpty9x9-v0", batch_size=4, _dry=True, **kw)


def test_auto_reset_modes():
    for arg, flag, mode in ((False, False, None), (True, True, "same_step"), ("same_step", True, "same_step"),
                            ("next_step", True, "next_step")):
        env = _dry(auto_reset=arg)
        assert env.auto_reset is flag and env.auto_reset_mode == mode and env.episode_info is False
    assert _dry().auto_reset is False and _dry().auto_reset_mode is None
    assert _dry(auto_reset="next_step", episode_info=True).episode_info is True
    for bad in ("bogus", "next", 2, "True"):
        with pytest.raises(ValueError):
            _dry(auto_reset=bad)
