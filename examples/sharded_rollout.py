#!/usr/bin/env python
"""Random-policy rollout of ONE batch sharded over several GPUs, driven by one process (needs an MI355X; with one GPU, name
it twice — the shards then share it).

    python examples/sharded_rollout.py --devices cuda:0,cuda:1 --batch 65536 --steps 200

Every shard's actions are made on the shard's own device and stream (`shards.on(k)`), and its step is issued from there, so
nothing crosses devices and the host never waits inside the loop: while shard 0's step kernel runs the host is already
issuing shard 1's.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from marlgrid_amd.envs import make, registered_envs  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--env", default="MarlGrid-3AgentCluttered15x15-v0", choices=registered_envs)
ap.add_argument("--devices", default="cuda:0,cuda:0")
ap.add_argument("--batch", type=int, default=8192)
ap.add_argument("--steps", type=int, default=200)
args = ap.parse_args()

shards = make(args.env, batch_size=args.batch, devices=args.devices.split(","), auto_reset=True, strict=False)
n, N = shards.num_agents, len(shards.envs)
obs = shards.reset()                                          # per shard: (B_k, n, P, P, 3) uint8 on devices[k], ordered on streams[k]
returns, episodes = [], []
for k in range(N):
    with shards.on(k):                                        # device k current, stream k current
        returns.append(torch.zeros(shards.envs[k].batch_size, n, device=shards.devices[k]))
        episodes.append(torch.zeros((), dtype=torch.int64, device=shards.devices[k]))
shards.synchronize()
t0 = time.perf_counter()
for t in range(args.steps):
    for k in range(N):
        with shards.on(k):
            actions = torch.randint(0, 3, (shards.envs[k].batch_size, n), device=shards.devices[k])     # left / right / forward
            obs[k], rew, done, _ = shards.step_shard(k, actions)
            returns[k] += rew
            episodes[k] += done.sum()
shards.synchronize()
dt = time.perf_counter() - t0
shards.check_errors()
total = sum(float(r.sum()) for r in returns)
finished = sum(int(e) for e in episodes)
print("%s on %s: %d envs (%s per shard) x %d steps in %.3f s = %.1f M agent-steps/s; %d episodes finished; mean return %.4f"
      % (args.env, [str(d) for d in shards.devices], args.batch, [e.batch_size for e in shards.envs], args.steps, dt,
         args.batch * n * args.steps / dt / 1e6, finished, total / max(finished, 1) / n))
