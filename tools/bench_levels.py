#!/usr/bin/env python
"""What replayable levels cost per step on the bench workload: `step()` plus the level calls, HIP events around `--steps` steps,
the legs alternating in ONE process (the GPU's clocks drift between processes), `--legs` rounds each; medians and ranges.

    (a) no levels                         auto_reset="next_step", episode_info=True, nothing else
    (b) bank form                         a bank of 4 096 levels; every step, the envs that finished are pointed at another slot
                                          by a device tensor: set_levels(bank, ids, env_mask=done) — mg_level_apply per step
    (c) seeds form                        every step, the envs that finished get a fresh device-drawn seed:
                                          set_levels(seeds=..., env_mask=done) — mg_level_seed + mg_level_apply per step
    (a') (a) through another build of the library (`--other-lib path/to/libmarlgrid_hip.so`, e.g. the parent commit's)

The bench workload only ends by its time limit, every env at once: before anything is timed the episodes are staggered (env b is
reset by hand after step b % max_steps), so that afterwards every step ends B / (max_steps + 1) episodes.  Nothing on the host
per step: ids and seeds come from pre-drawn device tensors.  Prints one JSON line.

    python tools/bench_levels.py --batch 32768 --steps 200
    python tools/bench_levels.py --only b --legs 1        # one leg alone, for a kernel trace
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from marlgrid_amd import _native as N  # noqa: E402
from marlgrid_amd.envs import make  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32768)
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--legs", type=int, default=5)
ap.add_argument("--levels", type=int, default=4096)
ap.add_argument("--only", default="", help="comma-separated legs (a, b, c, a_other); default: all there are")
ap.add_argument("--other-lib", default=None)
args = ap.parse_args()
NAME = "MarlGrid-3AgentCluttered15x15-v0"
B = args.batch
legs = ["a", "b", "c"] + (["a_other"] if args.other_lib else [])
if args.only:
    legs = [k for k in legs if k in args.only.split(",")]

other = None
if args.other_lib:
    other = C.CDLL(os.path.abspath(args.other_lib))
    for f in N.SYMBOLS:         # the same prototypes (a build without the level calls has every other symbol)
        if hasattr(other, f):
            getattr(other, f).argtypes = getattr(N.lib(), f).argtypes
            getattr(other, f).restype = getattr(N.lib(), f).restype

envs, banks = {}, {}
for k in legs:
    env = envs[k] = make(NAME, batch_size=B, seed=1337, auto_reset="next_step", episode_info=True, strict=False)
    if k == "a_other":
        env._lib = other
    if k == "b":
        banks[k] = env.level_bank(torch.arange(args.levels, device=env.device) + 10 ** 6)
        env.set_levels(banks[k], torch.arange(B, device=env.device) % args.levels)
    if k == "c":
        env.set_levels(seeds=torch.arange(B, device=env.device) + 10 ** 7)
dev = next(iter(envs.values())).device
n = next(iter(envs.values())).num_agents
M = next(iter(envs.values())).max_steps
gen = torch.Generator(dev).manual_seed(0)
acts = [torch.randint(0, 7, (B, n), device=dev, generator=gen) for _ in range(16)]
ids = [torch.randint(0, args.levels, (B,), device=dev, generator=gen) for _ in range(16)]
seeds = [torch.randint(0, 2 ** 62, (B,), device=dev, generator=gen) for _ in range(16)]
rows = torch.arange(B, device=dev)


def step(k, t):
    env = envs[k]
    _, _, done, _ = env.step(acts[t % 16])
    if k == "b":
        env.set_levels(banks[k], ids[t % 16], env_mask=done)
    elif k == "c":
        env.set_levels(seeds=seeds[t % 16], env_mask=done)


for k in legs:                  # stagger the episodes; the level calls run from the start
    envs[k].reset()
    for t in range(M):
        step(k, t)
        envs[k].reset(env_mask=(rows % M) == t)
    for t in range(2 * M + 2):
        step(k, t)
torch.cuda.synchronize()
ms = {k: [] for k in legs}
for _ in range(args.legs):
    for k in legs:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for t in range(args.steps):
            step(k, t)
        b.record()
        b.synchronize()
        ms[k].append(a.elapsed_time(b) / args.steps)
out = {"batch": B, "steps": args.steps, "legs": args.legs, "levels": args.levels, "max_steps": M, "ms_per_step": ms,
       "median_ms": {k: statistics.median(v) for k, v in ms.items()}, "range_ms": {k: [min(v), max(v)] for k, v in ms.items()},
       "level_launches": {k: envs[k]._level_launches for k in legs},
       "episode_levels_distinct": {k: int(envs[k].episode_level.unique().numel()) for k in legs},
       "kernel": envs[legs[0]].kernel_name, "build": N.lib().mg_build_info().decode()}
for k in legs:
    envs[k].check_errors()
print(json.dumps(out))
