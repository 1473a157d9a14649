#!/usr/bin/env python
"""What the exploration maps cost on the bench workload (MarlGrid-3AgentCluttered15x15-v0): HIP events around `--calls` calls, the
legs alternating in ONE process (the GPU's clocks drift between processes), `--rounds` rounds each; lowest, median and highest
round per leg, in microseconds per call.

    (a) env.step() with explore=False                      the yardstick: this commit's default step
    (b) env.step() with explore=True                       the same step and the mg_explore_update launch behind it
    (c) the mg_explore_update launch alone                 on (b)'s env, mask NULL: every env, as step() launches it
    (d) mg_encode_views on the same env                    the launch it shares its phases A to D with

Both envs are built from the same seeds, auto_reset=True as bench.py builds its env.  The workload only ends by its time limit,
every env at once: before anything is timed the episodes are staggered (env b is reset by hand after step b % max_steps), so
that afterwards every step begins a new episode — and clears two planes per agent — in B / max_steps envs.  Prints one JSON line.

    python tools/bench_explore.py --batch 32768 --calls 200
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
from marlgrid_amd.envs import make  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32768)
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--rounds", type=int, default=5)
args = ap.parse_args()
NAME, B = "MarlGrid-3AgentCluttered15x15-v0", args.batch

off = make(NAME, batch_size=B, seed=1337, auto_reset=True, strict=False)
on = make(NAME, batch_size=B, seed=1337, auto_reset=True, strict=False, explore=True)
dev, n, M = on.device, on.num_agents, on.max_steps
gen = torch.Generator(dev).manual_seed(0)
acts = [torch.randint(0, 7, (B, n), device=dev, generator=gen) for _ in range(16)]
rows = torch.arange(B, device=dev)
views = torch.zeros((B, n, on.view_size, on.view_size, 3), dtype=torch.uint8, device=dev)
ex = on._explore


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for t in range(calls):
        fn(t)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls * 1e3      # us per call


def leg_c(t):
    N.check(on._lib.mg_explore_update(C.byref(on._cfg), C.byref(on._state), None, ex.seen_u8.data_ptr(), ex.visits.data_ptr(),
                                      ex.new_cells.data_ptr(), ex.visit_count.data_ptr(), on._stream()))


def leg_d(t):
    N.check(on._lib.mg_encode_views(C.byref(on._cfg), C.byref(on._state), views.data_ptr(), on._stream()))


LEGS = {"a": lambda t: off.step(acts[t % 16]), "b": lambda t: on.step(acts[t % 16]), "c": leg_c, "d": leg_d}

for env in (off, on):
    env.reset()
    for t in range(M):              # stagger the episodes
        env.step(acts[t % 16])
        env.reset(env_mask=(rows % M) == t)
for k in LEGS:                      # warm: every tensor made, every kernel loaded
    for t in range(8):
        LEGS[k](t)
torch.cuda.synchronize()
us = {k: [] for k in LEGS}
for _ in range(args.rounds):
    for k in LEGS:
        us[k].append(timed(LEGS[k], args.calls))
med = {k: statistics.median(v) for k, v in us.items()}
out = {"batch": B, "calls": args.calls, "rounds": args.rounds, "max_steps": M, "us_per_call": us,
       "low_median_high_us": {k: [min(v), med[k], max(v)] for k, v in us.items()},
       "b_minus_a_us": [b - a for b, a in zip(us["b"], us["a"])],
       "b_over_a": med["b"] / med["a"], "c_over_d": med["c"] / med["d"],
       "explore_no_slower_than_encode_views": max(us["c"]) <= min(us["d"]),
       "seen_fraction": float(on.seen.float().mean()), "explore_launches": ex.launches,
       "kernel": on.kernel_name, "kernel_off": off.kernel_name, "build": N.lib().mg_build_info().decode()}
off.check_errors()
on.check_errors()
print(json.dumps(out))
