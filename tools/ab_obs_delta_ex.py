#!/usr/bin/env python
"""obs_delta with episode outputs and / or encode_in_step (mg_step_render_delta_ex) against another checkout — the parent commit's —
running the same options: ONE env per process, so that a run is a fresh process with its own package and library, as
profiles/obs_delta/README.md compared the plain delta.  The caller interleaves the two trees' runs (five each).

Times `env.step()` alone at the bench shape (MarlGrid-3AgentCluttered15x15-v0, 32 768 envs, uniform actions over the 7 ids, device
events around legs of `--steps` steps after `--warmup`), prints one JSON line: every leg's ms per step, their median, the build
that answered, how many of the steps were delta launches.

    python tools/ab_obs_delta_ex.py --options next_step,episode_info --obs-delta true
    python tools/ab_obs_delta_ex.py --tree ../parent --options next_step,episode_info --obs-delta auto
    python tools/ab_obs_delta_ex.py --against ../parent [--runs 5] [--mixes "next_step,episode_info;encode_in_step;encode_in_step,next_step,episode_info"]
--options: a comma list of episode_info, next_step, encode_in_step (empty: the plain step).  --tree: the checkout whose marlgrid_amd
is imported (default: this one).  --against DIR: the whole series — per run and mix one child process of DIR's tree with
obs_delta="auto" (the parent: the same options without the delta), then one of this tree with obs_delta=True, `--runs` times; the
children's lines are echoed, then one summary line per mix (both sides' medians, min - max, their ratio, and whether every run of
this tree beat every run of the other)."""
import argparse
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--options", default="")
ap.add_argument("--obs-delta", default="true", choices=["true", "false", "auto"])
ap.add_argument("--batch", type=int, default=32768)
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--legs", type=int, default=5)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--obs-buffers", type=int, default=2)
ap.add_argument("--against", default=None)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--mixes", default="next_step,episode_info;encode_in_step;encode_in_step,next_step,episode_info")
args = ap.parse_args()


def series():
    import subprocess
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = {}
    for run in range(args.runs):
        for mix in args.mixes.split(";"):
            for tree, delta in ((args.against, "auto"), (here, "true")):
                line = subprocess.check_output([sys.executable, os.path.abspath(__file__), "--tree", tree, "--options", mix, "--obs-delta", delta,
                                                "--batch", str(args.batch), "--steps", str(args.steps), "--legs", str(args.legs),
                                                "--warmup", str(args.warmup), "--obs-buffers", str(args.obs_buffers)], timeout=300)
                line = line.decode().strip().splitlines()[-1]
                print(line, flush=True)
                res.setdefault(mix, {}).setdefault(delta, []).append(json.loads(line))
    for mix, r in res.items():
        a, b = [x["median_ms"] for x in r["auto"]], [x["median_ms"] for x in r["true"]]
        ma, mb = sorted(a)[len(a) // 2], sorted(b)[len(b) // 2]
        print(json.dumps({"summary": mix, "other_tree_ms": a, "this_tree_delta_ms": b, "other_median": ma, "delta_median": mb,
                          "speedup": round(ma / mb, 4), "every_run_beats_every_other_run": max(b) < min(a),
                          "delta_launches": [x["delta_launches"] for x in r["true"]], "other_build": r["auto"][0]["build"],
                          "this_build": r["true"][0]["build"]}), flush=True)


if args.against:
    series()
    sys.exit(0)
sys.path.insert(0, os.path.abspath(args.tree))

import numpy as np
import torch

from marlgrid_amd import _native as N
from marlgrid_amd.envs import make

NAME = "MarlGrid-3AgentCluttered15x15-v0"


def main():
    opts = [o for o in args.options.split(",") if o]
    assert set(opts) <= {"episode_info", "next_step", "encode_in_step"}, opts
    kw = dict(auto_reset="next_step" if "next_step" in opts else True, episode_info="episode_info" in opts,
              encode_in_step="encode_in_step" in opts)
    delta = {"true": True, "false": False, "auto": "auto"}[args.obs_delta]
    dev, B = "cuda:0", args.batch
    env = make(NAME, batch_size=B, device=dev, seeds=1337 + np.arange(B), obs_delta=delta, obs_buffers=args.obs_buffers, **kw)
    g = torch.Generator().manual_seed(0)
    acts = [torch.randint(0, 7, (B, env.num_agents), generator=g).to(dev) for _ in range(64)]
    env.reset()
    t = 0

    def leg(steps):
        nonlocal t
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            env.step(acts[t % len(acts)])
            t += 1
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / steps
    leg(args.warmup)
    ms = [leg(args.steps) for _ in range(args.legs)]
    env.check_errors()
    print(json.dumps({"tree": os.path.abspath(args.tree), "build": N.lib().mg_build_info().decode(), "options": opts,
                      "obs_delta": args.obs_delta, "batch": B, "steps": args.steps, "obs_buffers": args.obs_buffers,
                      "ms": [round(v, 5) for v in ms], "median_ms": round(float(np.median(ms)), 5),
                      "delta_launches": int(getattr(env, "_delta_launches", 0)), "steps_taken": t}), flush=True)


if __name__ == "__main__":
    main()
