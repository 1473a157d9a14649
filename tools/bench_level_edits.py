#!/usr/bin/env python
"""What editable levels cost per step on the bench workload: `env.step()` (plus, for the bank legs, the level call in front of
it), HIP events around `--steps` steps, the legs alternating in ONE process (the GPU's clocks drift between processes),
`--legs` rounds each; medians and ranges.  bench.py's actions (uniform over the 7 ids).

    e0   level_edits=0, auto_reset=True            the default path: no table, no op
    e8   level_edits=8, auto_reset=True            every env holds 8 live edits (walls on random interior cells), applied at
                                                   every in-launch reset: 32 more bytes read per reset
    s    a seed-only bank, auto_reset="next_step"  every step, the envs that finished are pointed at another slot:
                                                   set_levels(bank, ids, env_mask=done) — mg_level_apply per step
    f    a full bank, the same                     ... mg_level_apply_rows per step: 8 + 4 K = 40 more bytes copied per env
                                                   that takes a slot
    (s and f both run level_edits=8 envs: the launch in front of the step is what differs)

Before anything is timed the episodes are staggered (env b is reset by hand after step b % max_steps), so that afterwards every
step ends B / (max_steps + 1) episodes.  Nothing on the host per step.  Prints one JSON line.

    python tools/bench_level_edits.py --batch 32768 --steps 200
"""
import argparse
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
ap.add_argument("--edits", type=int, default=8)
ap.add_argument("--only", default="", help="comma-separated legs (e0, e8, s, f); default: all")
args = ap.parse_args()
NAME = "MarlGrid-3AgentCluttered15x15-v0"
B, K, L = args.batch, args.edits, args.levels
legs = [k for k in ("e0", "e8", "s", "f") if not args.only or k in args.only.split(",")]

envs, banks = {}, {}
for k in legs:
    bank_leg = k in ("s", "f")
    env = envs[k] = make(NAME, batch_size=B, seed=1337, strict=False, level_edits=0 if k == "e0" else K,
                         auto_reset="next_step" if bank_leg else True, episode_info=bank_leg)
    gen = torch.Generator(env.device).manual_seed(1)
    if k != "e0":       # K live entries per env / per slot: walls on random interior cells
        def lists(rows):
            cell = torch.randint(1, env.width - 1, (rows, K, 2), device=env.device, generator=gen)
            return torch.cat([cell, torch.ones_like(cell)], dim=2)          # (x, y, kind 1 = Wall, on)
    if k == "e8":
        env.set_edits(lists(B))
    if bank_leg:
        banks[k] = env.level_bank(L, full=k == "f")
        seeds = torch.arange(L, device=env.device) + 10 ** 6
        if k == "f":
            banks[k].assign(None, seeds, edits=lists(L))
        else:
            banks[k].assign(None, seeds)
            env.set_edits(lists(B))
        env.set_levels(banks[k], torch.arange(B, device=env.device) % L)
first = envs[legs[0]]
dev, n, M = first.device, first.num_agents, first.max_steps
gen = torch.Generator().manual_seed(0)
acts = [torch.randint(0, 7, (B, n), generator=gen).to(dev) for _ in range(16)]
ids = [torch.randint(0, L, (B,), generator=gen).to(dev) for _ in range(16)]
rows = torch.arange(B, device=dev)


def step(k, t):
    env = envs[k]
    _, _, done, _ = env.step(acts[t % 16])
    if k in banks:
        env.set_levels(banks[k], ids[t % 16], env_mask=done)


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
out = {"batch": B, "steps": args.steps, "legs": args.legs, "levels": L, "level_edits": K, "max_steps": M, "ms_per_step": ms,
       "median_ms": {k: statistics.median(v) for k, v in ms.items()}, "range_ms": {k: [min(v), max(v)] for k, v in ms.items()},
       "extra_bytes_per_reset": {"e8": 4 * K, "f": N.GEN_DRAWS + 4 * K},
       "level_launches": {k: envs[k]._level_launches for k in legs},
       "kernel": {k: envs[k].kernel_name for k in legs}, "build": N.lib().mg_build_info().decode()}
for k in legs:
    envs[k].check_errors()
print(json.dumps(out))
