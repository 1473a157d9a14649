#!/usr/bin/env python
"""Exact regret on DoorKey (needs an MI355X): examples/level_regret.py's scoring on levels whose goal lies behind a locked door.

`env.goal_distance()` is a static analysis — nothing toggled, nothing picked up — and calls about half of these agent-level
pairs unsolvable; the example prints how many.  `env.solve_distance()` walks through the key and the door: every pair has a
path, and `env.optimal_return(dist=...)` of its distances is what an optimal agent earns.  After each step,
`env.solve_distance(env_mask=info["reset"])` analyses the envs that were just reset onto a new level: one launch, a wave per
such env, nothing goes to the host.  The regret of an episode is the optimal return of its level at the reset minus what the
agents did earn; a level's score is the mean regret of the episodes played on it (here the levels are the seeds of a
`LevelBank`, replayed by rank of their score as in examples/level_replay.py).

The envs have one agent each (with two, one agent can shut the door on the other, which the reference answers with an
AssertionError when that one moves on).  With --expert the agent follows `solve_distance(policy=True)` instead of acting at
random: its regret is 0.

    python examples/doorkey_regret.py --batch 4096 --steps 1000
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from marlgrid_amd.envs import make  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=4096)
ap.add_argument("--steps", type=int, default=1000)
ap.add_argument("--levels", type=int, default=256)
ap.add_argument("--expert", action="store_true", help="follow solve_distance's policy instead of acting at random")
args = ap.parse_args()
B, L = args.batch, args.levels

env = make("MarlGrid-1AgentDoorKey8x8-v0", batch_size=B, auto_reset="next_step", episode_info=True, max_steps=60, strict=False)
dev, n = env.device, env.num_agents
gen = torch.Generator(dev).manual_seed(0)
bank = env.level_bank(torch.randint(0, 2 ** 62, (L,), device=dev, generator=gen))
total = torch.zeros(L, device=dev)                  # per slot: the regrets of the episodes played on it, summed
plays = torch.zeros(L, device=dev)
slot = torch.randint(0, L, (B,), device=dev, generator=gen)
env.set_levels(bank, slot)
obs = env.reset()

static = env.goal_distance()
dist = env.solve_distance()
print("%d agent-level pairs: goal_distance finds no path for %d of them, solve_distance for %d (longest path %d actions; %d of "
      "%d envs exact)" % (dist.numel(), int((static < 0).sum()), int((dist < 0).sum()), int(dist.max()), int(env.solve_exact.sum()), B))
best = env.optimal_return(dist=dist).sum(1).float()                     # (B,): what the team could earn on the running level
for t in range(args.steps):
    if args.expert:
        actions = env.solve_distance(policy=True)[1]
    else:
        actions = torch.randint(0, 6, (B, n), device=dev, generator=gen)
    obs, rew, done, info = env.step(actions)
    regret = best - info["episode_return"].sum(1).float()
    total.index_add_(0, slot, regret * done)
    plays.index_add_(0, slot, done.float())
    # the envs whose call was their reset have a new grid: analyse those, and only those
    fresh = info["reset"]
    dist = env.solve_distance(env_mask=fresh)
    best = torch.where(fresh, env.optimal_return(dist=dist).sum(1).float(), best)
    score = total / plays.clamp(min=1)
    rank = (-score).argsort().argsort().float() + 1
    nxt = torch.multinomial(1 / rank, B, replacement=True)
    slot = torch.where(done, nxt, slot)
    env.set_levels(bank, nxt, env_mask=done)                            # the others keep the level they are playing
    if (t + 1) % 250 == 0:
        ok = plays > 0
        print("step %5d: %d slots played, mean regret %.3f" % (t + 1, int(ok.sum()), float(score[ok].mean())))
env.check_errors()
