#!/usr/bin/env python
"""Exploration maps at work (needs an MI355X): `MultiGridEnv(explore=True)` keeps, per agent, the cells it has seen this episode
and how often it stood on each cell — on the device, by one launch behind every step.  Two policies play the same levels of
`MarlGrid-2AgentDoorKey8x8-v0`: random play over left / right / forward, and a one-step greedy that looks at `env.visits` around
the agent — the cell ahead, and the cells it would face after a left or a right turn — and takes the action towards the cell it
has stood on least (an occupied cell counts as visited for ever; ties go to a random one of the tied actions).

Printed: the mean fraction of the level's free cells each agent had seen when its episode ended, for both; and for the last
step of the greedy run the two per-step scalars a count-based bonus is made of, `new_cells` and `1 / sqrt(visit_count)`.

    python examples/explore_bonus.py --batch 512 --max-steps 60
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from marlgrid_amd.envs import make  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=512)
ap.add_argument("--max-steps", type=int, default=60)
args = ap.parse_args()
B, T = args.batch, args.max_steps
DX, DY = (1, 0, -1, 0), (0, 1, 0, -1)     # the forward vector per heading


def play(policy):
    env = make("MarlGrid-2AgentDoorKey8x8-v0", batch_size=B, seed=1337, auto_reset=False, max_steps=T, strict=False, place_obs=False,
               explore=True)
    dev, n, W, H = env.device, env.num_agents, env.width, env.height
    gen = torch.Generator(dev).manual_seed(0)
    dx, dy = torch.tensor(DX, device=dev), torch.tensor(DY, device=dev)
    rows = torch.arange(B, device=dev).unsqueeze(1).expand(B, n)
    who = torch.arange(n, device=dev).unsqueeze(0).expand(B, n)
    env.reset()
    over = torch.zeros(B, dtype=torch.bool, device=dev)
    frac = torch.zeros((B, n), device=dev)
    for t in range(T):
        if policy == "random":
            actions = torch.randint(0, 3, (B, n), device=dev, generator=gen)
        else:
            pos, d = env.agent_pos, env.agent_dir
            grid = env.grid_state[:, :W * H].view(B, W, H)
            cost = []
            for turn in (-1, 1, 0):                 # left, right, forward: the action ids 0, 1, 2
                h = (d + turn) % 4
                cx, cy = (pos[..., 0] + dx[h]).clamp(0, W - 1), (pos[..., 1] + dy[h]).clamp(0, H - 1)
                v = env.visits[rows, who, cx, cy].float()
                cost.append(torch.where(grid[rows, cx, cy] != 0, torch.full_like(v, 1e9), v))
            cost = torch.stack(cost, dim=-1) + torch.rand((B, n, 3), device=dev, generator=gen) * 0.5     # (ties: at random)
            actions = cost.argmin(dim=-1)
        _, _, done, _ = env.step(actions)
        free = (env.grid_state[:, :W * H] == 0).view(B, 1, W, H)
        now = (env.seen & free).flatten(2).sum(2).float() / free.flatten(2).sum(2).clamp(min=1).float()
        frac = torch.where(over.unsqueeze(1), frac, now)
        over |= done
    env.check_errors()
    return float(frac.mean()), env


for policy in ("random", "greedy"):
    mean, env = play(policy)
    print("%-7s mean fraction of free cells seen at the episode's end: %.3f" % (policy, mean))
bonus = torch.where(env.visit_count > 0, env.visit_count.float().rsqrt(), torch.zeros_like(env.visit_count, dtype=torch.float32))
print("last step of the greedy run, env 0: new_cells %s, visit_count %s, 1 / sqrt(visit_count) %s"
      % (env.new_cells[0].tolist(), env.visit_count[0].tolist(), [round(v, 3) for v in bonus[0].tolist()]))
print("                   batch means: new_cells %.3f, 1 / sqrt(visit_count) %.3f" % (float(env.new_cells.float().mean()), float(bonus.mean())))
