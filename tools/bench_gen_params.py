#!/usr/bin/env python
"""Step time of the curriculum id (a PARAM op and a symbolic count in the reset program) beside the plain Cluttered id, same
batch, same seeds, same actions: HIP events around `--steps` steps after `--warmup`, auto_reset=True.  Prints one JSON line.

    python tools/bench_gen_params.py --batch 32768 --steps 200
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from marlgrid_amd.envs import make  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32768)
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--repeats", type=int, default=3)
args = ap.parse_args()
IDS = ("MarlGrid-3AgentCluttered15x15-v0", "MarlGrid-3AgentClutteredCurriculum15x15-v0")
out = {"batch": args.batch, "steps": args.steps, "ms_per_step": {}}
for env_id in IDS:
    env = make(env_id, batch_size=args.batch, seed=1337, auto_reset=True, strict=False)
    if "Curriculum" in env_id:          # the whole interval, mixed over the batch
        env.set_params(n_clutter=torch.arange(args.batch, device=env.device) % 51)
    env.reset()
    n = env.num_agents
    acts = [torch.randint(0, 7, (args.batch, n), device=env.device, generator=torch.Generator(env.device).manual_seed(i))
            for i in range(16)]
    for t in range(args.warmup):
        env.step(acts[t % 16])
    times = []
    for _ in range(args.repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for t in range(args.steps):
            env.step(acts[t % 16])
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / args.steps)
    out["ms_per_step"][env_id] = sorted(times)
    out.setdefault("kernel", {})[env_id] = env.kernel_name
    del env
print(json.dumps(out))
