#!/usr/bin/env python
"""What lookahead costs: HIP events around `--calls` calls, the legs alternating in ONE process (the GPU's clocks drift between
processes), `--rounds` rounds each; lowest, median and highest round per leg, in microseconds per call.  On
MarlGrid-3AgentCluttered15x15-v0, right after reset (no episode ends inside T = 16 steps), at (m, K, T) = (4096, 8, 16) and
(32768, 1, 16):

    (fork)     mg_fork_rows alone: K * m shadow rows written, m env rows read — against the bytes it moves, TB/s
    (rollout)  mg_fork_rows + mg_rollout, minus (fork): the one launch that steps every row T times
    (steps)    mg_fork_rows + T mg_step launches on the SAME shadow state, minus (fork): the existing kernel — the honest baseline,
               the parent commit has no lookahead
    (call)     env.lookahead(plans), the whole call: simulated agent-steps per second

Every timed leg begins with the fork, so that each repetition steps the same states.  Prints one JSON line.

    python tools/bench_lookahead.py --calls 50
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from marlgrid_amd import _native as N  # noqa: E402
from marlgrid_amd import lookahead as LA  # noqa: E402
from marlgrid_amd.envs import make  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=50)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--shapes", default="4096x8x16,32768x1x16")
args = ap.parse_args()
NAME = "MarlGrid-3AgentCluttered15x15-v0"


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for t in range(calls):
        fn(t)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls * 1e3      # us per call


def measure(legs):
    for k in legs:                  # warm: every tensor made, every kernel loaded
        for t in range(3):
            legs[k](t)
    torch.cuda.synchronize()
    us = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k in legs:
            us[k].append(timed(legs[k], args.calls))
    return us


out = {"env": NAME, "calls": args.calls, "rounds": args.rounds, "shapes": []}
for shape in args.shapes.split(","):
    m, K, T = (int(v) for v in shape.split("x"))
    env = make(NAME, batch_size=m, seed=1337, auto_reset=False, place_obs=False, strict=False)
    env.reset()
    dev, n, R = env.device, env.num_agents, K * m
    gen = torch.Generator(dev).manual_seed(0)
    plans = torch.randint(0, 7, (K, T, m, n), device=dev, generator=gen)
    flat = torch.randint(0, 7, (T, R, n), device=dev, generator=gen)       # the T mg_step launches: one (R, n) block per step
    rewards, _ = env.lookahead(plans)
    look, lib, stream = env._look, env._lib, env._stream()
    sh, cfg = look.shadow, look.cfg
    step_rew = torch.zeros((R, n), dtype=torch.float32, device=dev)
    out_rew, out_done, out_err = look.out[(K, T, m)]

    def fork(t):
        N.check(lib.mg_fork_rows(C.byref(env._cfg), C.byref(env._state), C.byref(sh.state), None, None, R, R, m, stream))

    def rollout(t):
        fork(t)
        N.check(lib.mg_rollout(C.byref(cfg), C.byref(sh.state), plans.data_ptr(), 8, T, m, out_rew.data_ptr(), out_done.data_ptr(),
                               out_err.data_ptr(), stream))

    def steps(t):
        fork(t)
        for i in range(T):
            N.check(lib.mg_step(C.byref(cfg), C.byref(sh.state), flat[i].data_ptr(), 8, step_rew.data_ptr(), None, stream))

    us = measure({"fork": fork, "rollout": rollout, "steps": steps, "call": lambda t: env.lookahead(plans)})
    med = {k: statistics.median(v) for k, v in us.items()}
    row = LA.row_bytes(env.cells_stride, n, env.prestige_t is not None)
    moved = row * (R + m)           # every shadow row written, every env row read once (its K readers meet in L2)
    out["shapes"].append({
        "m": m, "K": K, "T": T, "rows": R, "row_bytes": row,
        "low_median_high_us": {k: [min(v), statistics.median(v), max(v)] for k, v in us.items()},
        "fork_bytes": moved, "fork_TB_per_s": moved / (med["fork"] * 1e-6) / 1e12,
        "rollout_minus_fork_us": med["rollout"] - med["fork"], "steps_minus_fork_us": med["steps"] - med["fork"],
        "rollout_over_steps": (med["rollout"] - med["fork"]) / (med["steps"] - med["fork"]),
        "agent_steps_per_s": R * T * n / (med["call"] * 1e-6),
        "frozen_rows": int(out_done[:, -1].sum())})
    env.check_errors()
    del env, look, sh, plans, flat, rewards
    torch.cuda.empty_cache()
out["build"] = N.lib().mg_build_info().decode()
print(json.dumps(out))
