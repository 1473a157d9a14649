#!/usr/bin/env python
"""What the memory maps cost on the bench workload (MarlGrid-3AgentCluttered15x15-v0): HIP events around `--calls` calls, the
legs alternating in ONE process (the GPU's clocks drift between processes), `--rounds` rounds each; lowest, median and highest
round per leg, in microseconds per call.

    (a) env.step() with explore=True                       the yardstick: the step and the mg_explore_update launch behind it
    (b) env.step() with memory=True                        the same step and the mg_memory_update launch in its place
    (c) the mg_memory_update launch alone                  on (b)'s env, mask NULL: every env, as step() launches it
    (d) the mg_explore_update launch alone                 on (a)'s env, likewise
    (e) mg_encode_views on (b)'s env                       the launch whose triples (c) stores

Both envs are built from the same seeds, auto_reset=True as bench.py builds its env.  The workload only ends by its time limit,
every env at once: before anything is timed the episodes are staggered (env b is reset by hand after step b % max_steps), so
that afterwards every step begins a new episode — and clears the planes of every agent — in B / max_steps envs.  Prints one JSON
line.

    python tools/bench_memory.py --batch 32768 --calls 200
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

exp = make(NAME, batch_size=B, seed=1337, auto_reset=True, strict=False, explore=True)
mem = make(NAME, batch_size=B, seed=1337, auto_reset=True, strict=False, memory=True)
dev, n, M = mem.device, mem.num_agents, mem.max_steps
gen = torch.Generator(dev).manual_seed(0)
acts = [torch.randint(0, 7, (B, n), device=dev, generator=gen) for _ in range(16)]
rows = torch.arange(B, device=dev)
views = torch.zeros((B, n, mem.view_size, mem.view_size, 3), dtype=torch.uint8, device=dev)


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for t in range(calls):
        fn(t)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls * 1e3      # us per call


def four(env):
    ex = env._explore
    return (ex.seen_u8.data_ptr(), ex.visits.data_ptr(), ex.new_cells.data_ptr(), ex.visit_count.data_ptr())


def leg_c(t):
    ex = mem._explore
    N.check(mem._lib.mg_memory_update(C.byref(mem._cfg), C.byref(mem._state), None, *four(mem), ex.memory.data_ptr(),
                                      ex.seen_step.data_ptr(), mem._stream()))


def leg_d(t):
    N.check(exp._lib.mg_explore_update(C.byref(exp._cfg), C.byref(exp._state), None, *four(exp), exp._stream()))


def leg_e(t):
    N.check(mem._lib.mg_encode_views(C.byref(mem._cfg), C.byref(mem._state), views.data_ptr(), mem._stream()))


LEGS = {"a": lambda t: exp.step(acts[t % 16]), "b": lambda t: mem.step(acts[t % 16]), "c": leg_c, "d": leg_d, "e": leg_e}

for env in (exp, mem):
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
known = mem.memory[..., 3] == 1
stale = (mem.step_count[:, None, None, None] - mem.seen_step)[known].float().mean()
out = {"batch": B, "calls": args.calls, "rounds": args.rounds, "max_steps": M, "us_per_call": us,
       "low_median_high_us": {k: [min(v), med[k], max(v)] for k, v in us.items()},
       "b_minus_a_us": [b - a for b, a in zip(us["b"], us["a"])], "c_minus_d_us": [c - d for c, d in zip(us["c"], us["d"])],
       "b_over_a": med["b"] / med["a"], "c_over_d": med["c"] / med["d"], "c_over_e": med["c"] / med["e"],
       "known_fraction": float(known.float().mean()), "mean_staleness_of_known_cells": float(stale),
       "invariants_hold": bool((known == mem.seen).all() and ((mem.seen_step >= 0) == mem.seen).all()),
       "launches": {"explore": exp._explore.launches, "memory": mem._explore.launches},
       "kernel": mem.kernel_name, "build": N.lib().mg_build_info().decode()}
exp.check_errors()
mem.check_errors()
print(json.dumps(out))
