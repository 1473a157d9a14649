#!/usr/bin/env python
"""A curriculum over the clutter of a batched gridworld (needs an MI355X): every env reads its own number of wall blocks,
0 .. 50, from `env.params["n_clutter"]` when it resets.  An env whose episode TERMINATED (every agent reached the goal) gets
more blocks for its next episodes, one that was TRUNCATED by the time limit gets fewer — on the device, without a host
synchronisation and without building a second env.

    python examples/curriculum.py --batch 4096 --steps 2000
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from marlgrid_amd.envs import make  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=4096)
ap.add_argument("--steps", type=int, default=2000)
ap.add_argument("--up", type=int, default=5, help="blocks added after an episode that terminated")
ap.add_argument("--down", type=int, default=2, help="blocks taken away after an episode that was truncated")
args = ap.parse_args()

# auto_reset="next_step": the step after an episode's end is the env's reset — the value set in between is the one it reads
env = make("MarlGrid-3AgentClutteredCurriculum15x15-v0", batch_size=args.batch, auto_reset="next_step", episode_info=True,
           max_steps=100, strict=False)
n = env.num_agents
env.set_params(n_clutter=5)                                     # everyone starts easy (the id's default is 25)
obs = env.reset()
for t in range(args.steps):
    actions = torch.randint(0, 3, (args.batch, n), device=obs.device)     # left / right / forward
    obs, rew, done, info = env.step(actions)
    level = env.params["n_clutter"].to(torch.int64)             # (B,) — a view of the table the resets read
    level = level + args.up * info["terminated"] - args.down * info["truncated"]
    env.set_params(n_clutter=level)                             # a device tensor: clamped to 0 .. 50 in stream order
    if (t + 1) % 500 == 0:
        lv = env.params["n_clutter"].float()
        print("step %5d: n_clutter mean %.1f, min %d, max %d" % (t + 1, float(lv.mean()), int(lv.min()), int(lv.max())))
env.check_errors()
