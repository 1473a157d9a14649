#!/usr/bin/env python
"""Interleaved A/B of the step launches that do not go through the obs kernel — mg_step alone (MODE=step) and
mg_step_encode_views, the launch behind env.step() with obs_format="encoded" (MODE=views) — between builds of the
library given as paths, in ONE process on one env's state (tools/ab_fused.py is the same for mg_step_render).  First a
parity check of every build against the first one (two envs, same seeds and actions, 130 steps with auto-reset: rewards,
done, records, grids, the whole RNG state and, MODE=views, the views must be equal), then REPS (9) interleaved rounds of
100 launches each.
usage: MODE=step|views [B=32768] [WL=...] [REPS=9] ab_step.py path/to/ref.so path/to/new.so [...]"""
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from marlgrid_amd import _native as N  # noqa: E402
from marlgrid_amd.envs import make  # noqa: E402

names = sys.argv[1:]
MODE = os.environ.get("MODE", "step")
B = int(os.environ.get("B", "32768"))
WL = os.environ.get("WL", "MarlGrid-3AgentCluttered15x15-v0")
g = torch.Generator().manual_seed(0)


def build():
    return make(WL, batch_size=B, auto_reset=True, strict=False, obs_format="encoded")


env = build()
n = env.num_agents
acts = [torch.randint(0, 7, (B, n), generator=g).cuda() for _ in range(16)]
vp, i32 = C.c_void_p, C.c_int32
libs = {}
for nm in names:
    L = C.CDLL(os.path.abspath(nm))
    L.mg_step.argtypes = [C.POINTER(N.Config), C.POINTER(N.State), vp, i32, vp, C.POINTER(N.GenProgram), vp]
    L.mg_step_encode_views.argtypes = [C.POINTER(N.Config), C.POINTER(N.State), vp, i32, vp, C.POINTER(N.GenProgram), vp, vp]
    L.mg_step.restype = L.mg_step_encode_views.restype = i32
    L.mg_build_info.restype = C.c_char_p
    libs[nm] = L
    print("%s: %s" % (nm, L.mg_build_info().decode()))


def launch(L, e, i):
    head = (C.byref(e._cfg), C.byref(e._state), acts[i % 16].data_ptr(), 8, e.rewards.data_ptr(), C.byref(e._reset_prog))
    if MODE == "views":
        rc = L.mg_step_encode_views(*head, e.obs.data_ptr(), e._stream())
    else:
        rc = L.mg_step(*head, e._stream())
    assert rc == 0, rc


env.reset()
env.step(acts[0])          # (traces the reset program)
ref = build()
ref.reset()
ref.step(acts[0])
for nm in names[1:]:
    for i in range(130):
        launch(libs[names[0]], ref, i)
        launch(libs[nm], env, i)
        if i % 10 == 9 or i > 95:
            for k in ("rewards", "done_t", "agent_state", "grid_state", "mt_state", "mt_pos", "mt_head", "step_count_t") + (("obs",) if MODE == "views" else ()):
                assert torch.equal(getattr(env, k), getattr(ref, k)), ("%s differs from %s in %s at step %d" % (nm, names[0], k, i))
    env.check_errors()
    print("%s identical to %s over 130 steps" % (nm, names[0]), flush=True)
del ref
res = {nm: [] for nm in names}
for rep in range(int(os.environ.get("REPS", "9"))):
    for nm in names:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        launch(libs[nm], env, 0)
        a.record()
        for i in range(100):
            launch(libs[nm], env, i)
        b.record()
        b.synchronize()
        res[nm].append(a.elapsed_time(b) / 100)
base = statistics.median(res[names[0]])
for nm in names:
    m = statistics.median(res[nm])
    print("MODE=%s B=%d %s median %.4f ms (min %.4f max %.4f)  %+.2f%% vs %s" % (MODE, B, nm, m, min(res[nm]), max(res[nm]), 100 * (m / base - 1), names[0]))
