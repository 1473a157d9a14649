#!/usr/bin/env python
"""obs_delta on / off, interleaved, at the bench shape (MarlGrid-3AgentCluttered15x15-v0, 32 768 envs, auto_reset): two envs
in one process — same seeds, same actions —, timed in turns of `--steps` steps each with device events, `--rounds` turns each.
Per policy: ms per step of every turn, the medians, the ratio, and each side's own max - min spread.  Policies: `uniform`
(bench.py's: uniform over the 7 action ids), `moving` (left / right / forward only: every agent changes its image every step —
the guard rail: obs_delta must not cost more than the spread there), `done` (nothing moves: the ceiling).

--fraction: also the share of bands the delta launch did NOT store, read off the buffers themselves: the set about to be
written is filled with 0xA5 behind the env's back, and the bands that still read 0xA5 after the step were skipped
(tests/test_hip_obs_delta.py's method), averaged over `--fraction-steps` steps after 20 steps of the policy.

    python tools/ab_obs_delta.py [--batch 32768] [--steps 200] [--rounds 5] [--policies uniform,moving,done] [--fraction]
Prints one JSON line per policy."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from marlgrid_amd.envs import make

NAME = "MarlGrid-3AgentCluttered15x15-v0"


def pool(policy, B, n, dev, count=64, seed=0):
    g = torch.Generator().manual_seed(seed)
    if policy == "uniform":
        return [torch.randint(0, 7, (B, n), generator=g).to(dev) for _ in range(count)]
    if policy == "moving":
        return [torch.randint(0, 3, (B, n), generator=g).to(dev) for _ in range(count)]      # left, right, forward
    if policy == "done":
        return [torch.full((B, n), 6, dtype=torch.int64).to(dev) for _ in range(count)]
    raise KeyError(policy)


def timed(env, acts, steps, t0):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for s in range(steps):
        env.step(acts[(t0 + s) % len(acts)])
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def skipped_fraction(env, acts, steps):
    """in turns of `obs_buffers` steps: measured steps (sentinel in, count what survives, invalidate THAT set — the sentinel is
    not an observation), then as many repairing steps (they store everything and record the signature the next
    measured step into the set compares with, `obs_buffers` steps later as in ordinary use)"""
    fr = []
    nb = env.obs_buffers
    for s in range(steps):
        if (s // nb) % 2:
            env.step(acts[s % len(acts)])
            continue
        i = (env._ring_i + 1) % nb if nb > 1 else 0
        env._ring[i]["obs"].fill_(0xA5)
        o = env.step(acts[s % len(acts)])[0]
        B, n, P = o.shape[:3]
        stale = (o.reshape(B, n, P // 8, 8 * P * 3) == 0xA5).all(dim=-1)
        fr.append(stale.float().mean().item())
        env.invalidate_obs(i)
    return fr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32768)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--policies", default="uniform,moving,done")
    ap.add_argument("--obs-buffers", type=int, default=2)
    ap.add_argument("--fraction", action="store_true")
    ap.add_argument("--fraction-steps", type=int, default=40)
    args = ap.parse_args()
    dev = "cuda:0"
    B = args.batch
    seeds = 1337 + np.arange(B)
    envs = {k: make(NAME, batch_size=B, device=dev, seeds=seeds, auto_reset=True, obs_delta=k, obs_buffers=args.obs_buffers)
            for k in (True, False)}
    n = envs[True].num_agents
    for policy in args.policies.split(","):
        acts = pool(policy, B, n, dev)
        for e in envs.values():
            e.reset()
            timed(e, acts, 20, 0)
        ms = {True: [], False: []}
        t0 = 20
        for r in range(args.rounds):
            for k in ((True, False) if r % 2 == 0 else (False, True)):
                ms[k].append(timed(envs[k], acts, args.steps, t0))
            t0 += args.steps
        same = bool(torch.equal(envs[True].obs, envs[False].obs))
        out = {"policy": policy, "batch": B, "steps": args.steps, "obs_buffers": args.obs_buffers,
               "delta_ms": [round(v, 5) for v in ms[True]], "plain_ms": [round(v, 5) for v in ms[False]],
               "delta_median": round(float(np.median(ms[True])), 5), "plain_median": round(float(np.median(ms[False])), 5),
               "delta_spread": round(max(ms[True]) - min(ms[True]), 5), "plain_spread": round(max(ms[False]) - min(ms[False]), 5),
               "speedup": round(float(np.median(ms[False]) / np.median(ms[True])), 4), "obs_equal_at_end": same,
               "delta_in_use": bool(envs[True]._delta_wanted())}
        if args.fraction:
            e = envs[True]
            e.reset()
            timed(e, acts, 20 + 2 * args.obs_buffers, 0)
            fr = skipped_fraction(e, acts, args.fraction_steps)
            # (the twin takes the same steps: the two envs' RNG streams stay the same for the next policy's comparison)
            envs[False].reset()
            timed(envs[False], acts, 20 + 2 * args.obs_buffers, 0)
            for s_ in range(args.fraction_steps):
                envs[False].step(acts[s_ % len(acts)])
            out["skipped_bands"] = round(float(np.mean(fr)), 4)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
