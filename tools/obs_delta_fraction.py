#!/usr/bin/env python
"""How much of an observation equals what its ring buffer already holds — on the CPU oracle, no GPU: OracleBatch of
MarlGrid-3AgentCluttered15x15-v0, `--envs` envs (seeds 1337 + i), `--steps` steps, auto_reset, the first `--drop` steps left out.
Per unit (a band: one tile row of one agent's image, 8 pixel rows; a whole agent image; 24 pixel rows of the env's output
stream — one four-trip block of the fixed-lane chunk raster; a single tile) the share that is byte-identical to the observation
k steps earlier, k = 2 (obs_buffers=2, the default) and k = 1.  Policies: uniform over the 7 action ids (bench.py's), or
`moving` (left / right / forward only).

    python tools/obs_delta_fraction.py [--envs 512] [--steps 230] [--drop 20] [--policy uniform]
Prints one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=512)
    ap.add_argument("--steps", type=int, default=230)
    ap.add_argument("--drop", type=int, default=20)
    ap.add_argument("--policy", choices=("uniform", "moving"), default="uniform")
    args = ap.parse_args()
    import scenarios
    from oracle import oracle as O
    name = "MarlGrid-3AgentCluttered15x15-v0"
    orc = O.OracleBatch(scenarios.registered(name), 1337 + np.arange(args.envs))
    orc.reset()
    rng = np.random.RandomState(0)
    hist = []
    units = ("band", "image", "rows24", "tile")
    same = {(u, k): [] for u in units for k in (1, 2)}
    for t in range(args.steps):
        a = rng.randint(0, 7 if args.policy == "uniform" else 3, size=(args.envs, orc.n))
        obs = np.array(orc.step(a, auto_reset=True)[0], copy=True)          # (B, n, P, P, 3)
        B, n, P = obs.shape[:3]
        V = P // 8
        for k in (1, 2):
            if len(hist) >= k and t >= args.drop:
                eq = obs == hist[-k]
                same[("band", k)].append(eq.reshape(B, n, V, -1).all(-1).mean())
                same[("image", k)].append(eq.reshape(B, n, -1).all(-1).mean())
                same[("rows24", k)].append(eq.reshape(B, n * P // 24, -1).all(-1).mean())
                same[("tile", k)].append(eq.reshape(B, n, V, 8, V, 24).all(axis=(3, 5)).mean())
        hist = (hist + [obs])[-2:]
    out = {"envs": args.envs, "steps": args.steps, "drop": args.drop, "policy": args.policy}
    for u in units:
        out[u] = {"vs_2_steps_earlier": round(float(np.mean(same[(u, 2)])), 4), "vs_1_step_earlier": round(float(np.mean(same[(u, 1)])), 4)}
    out["band_min_step_vs_2"] = round(float(np.min(same[("band", 2)])), 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
