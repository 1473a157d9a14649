#!/usr/bin/env python
"""What solve_distance costs, next to goal_distance on the same envs: HIP events around `--calls` calls, the legs alternating in
ONE process (the GPU's clocks drift between processes), `--rounds` rounds each; lowest, median and highest round per leg, in
microseconds per call.

  MarlGrid-2AgentDoorKey8x8-v0 (one door, one key: 4 of the default 12 layers)
    (a) solve_distance() for every env, default caps       (b) the same with policy=True (one more copy kernel)
    (c) goal_distance(_path="lds")                         (d) goal_distance() — the register-resident kernel
    (e) env.step() alone, auto_reset="next_step"           (f) step() + solve_distance(env_mask=info["reset"]); reported as (f) - (e)
    (a1) solve_distance(max_doors=1, max_items=1): the caps these levels need — the same 4 layers searched, a third of the LDS
  MarlGrid-3AgentCluttered15x15-v0 (no door, no item: ONE layer — the LDS goal kernel's plane work plus the scan for
  interactables and an edge pass per level)
    (g) solve_distance()      (h) goal_distance(_path="lds")      (i) goal_distance()
    (g0) solve_distance(max_doors=0, max_items=0): the same one layer, LDS for one layer

goal_distance and its kernels are the parent commit's.  The DoorKey episodes are staggered before anything is timed, as
tools/bench_goal_distance.py does.  Prints one JSON line.

    python tools/bench_solve_distance.py --batch 32768 --calls 200
"""
import argparse
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
B = args.batch
DOORKEY, CLUTTERED = "MarlGrid-2AgentDoorKey8x8-v0", "MarlGrid-3AgentCluttered15x15-v0"


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for t in range(calls):
        fn(t)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls * 1e3      # us per call


def measure(legs, warm):
    for k in legs:                  # warm: every tensor made, every kernel loaded
        for t in range(warm.get(k, 4)):
            legs[k](t)
    torch.cuda.synchronize()
    us = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k in legs:
            us[k].append(timed(legs[k], args.calls))
    return us


def summary(us):
    return {k: [min(v), statistics.median(v), max(v)] for k, v in us.items()}


env = make(DOORKEY, batch_size=B, seed=1337, auto_reset="next_step", episode_info=True, strict=False)
dev, n, M = env.device, env.num_agents, env.max_steps
gen = torch.Generator(dev).manual_seed(0)
# (no toggle: a door shut on the other agent is the reference's AssertionError when that agent moves on)
acts = [torch.randint(0, 5, (B, n), device=dev, generator=gen) for _ in range(16)]
rows = torch.arange(B, device=dev)
env.reset()
for t in range(M):              # stagger the episodes
    env.step(acts[t % 16])
    env.reset(env_mask=(rows % M) == t)


def leg_f(t):
    info = env.step(acts[t % 16])[3]
    env.solve_distance(env_mask=info["reset"])


us = measure({"a": lambda t: env.solve_distance(), "b": lambda t: env.solve_distance(policy=True),
              "c": lambda t: env.goal_distance(_path="lds"), "d": lambda t: env.goal_distance(),
              "e": lambda t: env.step(acts[t % 16]), "f": leg_f,
              "a1": lambda t: env.solve_distance(max_doors=1, max_items=1)}, {"e": 2 * M + 2})
dist, static = env.solve_distance(), env.goal_distance()
med = {k: statistics.median(v) for k, v in us.items()}
out = {"batch": B, "calls": args.calls, "rounds": args.rounds,
       "doorkey": {"env": DOORKEY, "max_steps": M, "low_median_high_us": summary(us),
                   "solve_over_goal_lds": med["a"] / med["c"], "solve_over_goal_default": med["a"] / med["d"],
                   "solve_share_of_step": med["a"] / med["e"],
                   "f_minus_e_us": [f - e for f, e in zip(us["f"], us["e"])],
                   "f_minus_e_share_of_step": statistics.median(f - e for f, e in zip(us["f"], us["e"])) / med["e"],
                   "pairs_without_a_path": int((dist < 0).sum()), "pairs_goal_distance_calls_unsolvable": int((static < 0).sum()),
                   "exact_envs": int(env.solve_exact.sum()),
                   "lds_bytes": {"default": N.lib().mg_solve_distance_lds_bytes(env.width, env.height, 2, 2),
                                 "caps_1_1": N.lib().mg_solve_distance_lds_bytes(env.width, env.height, 1, 1)}}}
env.check_errors()
del env
torch.cuda.empty_cache()

env = make(CLUTTERED, batch_size=B, seed=1337, auto_reset=False, place_obs=False, strict=False)
env.reset()
us = measure({"g": lambda t: env.solve_distance(), "h": lambda t: env.goal_distance(_path="lds"), "i": lambda t: env.goal_distance(),
              "g0": lambda t: env.solve_distance(max_doors=0, max_items=0)}, {})
med = {k: statistics.median(v) for k, v in us.items()}
out["cluttered"] = {"env": CLUTTERED, "low_median_high_us": summary(us), "solve_over_goal_lds": med["g"] / med["h"],
                    "solve_over_goal_default": med["g"] / med["i"], "one_layer_lds_over_goal_lds": med["g0"] / med["h"],
                    "lds_bytes": {"default": N.lib().mg_solve_distance_lds_bytes(env.width, env.height, 2, 2),
                                  "caps_0_0": N.lib().mg_solve_distance_lds_bytes(env.width, env.height, 0, 0)},
                    "equal_to_goal_distance": bool(torch.equal(env.solve_distance(), env.goal_distance()))}
out["build"] = N.lib().mg_build_info().decode()
print(json.dumps(out))
