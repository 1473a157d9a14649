#!/usr/bin/env python
"""What goal_distance costs next to a step on the bench workload (MarlGrid-3AgentCluttered15x15-v0): HIP events around `--calls`
calls, the legs alternating in ONE process (the GPU's clocks drift between processes), `--rounds` rounds each; lowest, median and
highest round per leg, in microseconds per call and as a share of (a).

    (a) env.step() alone                                   auto_reset="next_step", episode_info=True: the yardstick
    (b) goal_distance() for every env, register-resident kernel
    (c) the same, LDS kernel
    (d) step() + goal_distance(env_mask=info["reset"])      what a replay loop adds per step; reported as (d) and as (d) - (a)
    (e) goal_distance(field=True) for every env

The bench workload only ends by its time limit, every env at once: before anything is timed the episodes are staggered (env b is
reset by hand after step b % max_steps), so that afterwards every step resets B / (max_steps + 1) envs.  Then one line each, no
claim attached: Custom-8AgentCluttered30x30 (tests/scenarios.py) at `--wide-batch` envs, and the 255 x 255 serpentine maze of
tests/goal_ref.py at B = 2 — the worst case, 32 509 levels.  Those two lines borrow the test infrastructure (product_envs for
the scenario, goal_ref for the maze, hostemu_goal.RawCase for a config made by hand), as tools/fuzz_sweep.py and
tools/long_soak.py do: `--skip-extra` runs without any of it.  Prints one JSON line.

    python tools/bench_goal_distance.py --batch 32768 --calls 200
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "native"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from marlgrid_amd import _native as N  # noqa: E402
from marlgrid_amd.envs import make  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32768)
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--wide-batch", type=int, default=16384)
ap.add_argument("--skip-extra", action="store_true", help="the five legs only")
args = ap.parse_args()
NAME, B = "MarlGrid-3AgentCluttered15x15-v0", args.batch

env = make(NAME, batch_size=B, seed=1337, auto_reset="next_step", episode_info=True, strict=False)
dev, n, M = env.device, env.num_agents, env.max_steps
gen = torch.Generator(dev).manual_seed(0)
acts = [torch.randint(0, 3, (B, n), device=dev, generator=gen) for _ in range(16)]
rows = torch.arange(B, device=dev)


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for t in range(calls):
        fn(t)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls * 1e3      # us per call


def leg_d(t):
    info = env.step(acts[t % 16])[3]
    env.goal_distance(env_mask=info["reset"])


LEGS = {"a": lambda t: env.step(acts[t % 16]),
        "b": lambda t: env.goal_distance(_path="reg"),
        "c": lambda t: env.goal_distance(_path="lds"),
        "d": leg_d,
        "e": lambda t: env.goal_distance(field=True)}

env.reset()
for t in range(M):              # stagger the episodes
    env.step(acts[t % 16])
    env.reset(env_mask=(rows % M) == t)
for k in LEGS:                  # warm: every tensor made, every kernel loaded
    for t in range(2 * M + 2 if k == "a" else 4):
        LEGS[k](t)
torch.cuda.synchronize()
us = {k: [] for k in LEGS}
for _ in range(args.rounds):
    for k in LEGS:
        us[k].append(timed(LEGS[k], args.calls))
dist = env.goal_distance()
out = {"batch": B, "calls": args.calls, "rounds": args.rounds, "max_steps": M, "us_per_call": us,
       "low_median_high_us": {k: [min(v), statistics.median(v), max(v)] for k, v in us.items()},
       "d_minus_a_us": [d - a for d, a in zip(us["d"], us["a"])],
       "share_of_a": {k: statistics.median(us[k]) / statistics.median(us["a"]) for k in "bce"},
       "d_minus_a_share_of_a": statistics.median(d - a for d, a in zip(us["d"], us["a"])) / statistics.median(us["a"]),
       "register_path_kept": max(us["b"]) < min(us["c"]),
       "pairs_without_a_distance": int((dist < 0).sum()), "goal_launches": env._goal.launches,
       "kernel": env.kernel_name, "build": N.lib().mg_build_info().decode()}
env.check_errors()

if not args.skip_extra:
    import goal_ref as G
    import hostemu_goal as HG
    import product_envs
    del env
    torch.cuda.empty_cache()
    Bw = args.wide_batch
    wide = product_envs.build("Custom-8AgentCluttered30x30", batch_size=Bw, seed=1337, place_obs=False, auto_reset=False, strict=False)
    wide.reset()
    for t in range(4):
        wide.goal_distance(field=True)
    out["wide_30x30"] = {"batch": Bw, "us_dist": [timed(lambda t: wide.goal_distance(), 50) for _ in range(3)],
                         "us_field": [timed(lambda t: wide.goal_distance(field=True), 50) for _ in range(3)]}
    del wide
    wall, goal = G.serpentine(255, 255)
    g = np.zeros((2, 255, 255), np.uint8)
    g[:, wall] = HG.RawCase.WALL
    g[:, goal[0], goal[1]] = HG.RawCase.GOAL
    case = HG.RawCase(g, [[(1, 1, 0, 5)], [(1, 1, 0, 5)]])
    grid, rec = torch.from_numpy(case.grid).to(dev), torch.from_numpy(case.rec.view(np.int64)).to(dev)
    obj = torch.from_numpy(np.frombuffer(bytes(case.obj), np.uint8).copy()).to(dev)
    case.cfg.obj = obj.data_ptr()
    case.state.grid, case.state.agents = grid.data_ptr(), rec.data_ptr()
    d = torch.full((2, 1), -7, dtype=torch.int32, device=dev)
    f = torch.full((2, 255, 255, 4), -7, dtype=torch.int32, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def maze(t, field=None):
        N.check(N.lib().mg_goal_distance(C.byref(case.cfg), C.byref(case.state), None, d.data_ptr(), field, stream))
    maze(0)
    out["maze_255x255"] = {"batch": 2, "us_dist": [timed(maze, 2) for _ in range(3)],
                           "us_field": [timed(lambda t: maze(t, f.data_ptr()), 2) for _ in range(3)], "dist": int(d[0, 0])}
print(json.dumps(out))
