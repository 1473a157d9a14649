#!/usr/bin/env python
"""A minimal prioritised level replay loop (needs an MI355X).  A level is a seed: an env that resets onto slot i of the bank
plays `env.seed(bank.seeds[i]); env.reset()`, the same layout and the same draws whoever plays it and whenever.  The bank holds
512 levels with a score each — here how badly the team does on the level, minus the mean of its episode returns there, standing
in for a learner's regret estimate.  Every env that finishes an episode is sent to a slot sampled by score rank, high scores
first; now and then the lowest-scored slots are replaced by fresh seeds drawn on the device.  Nothing is read back per step:
scores, sampling and replacement are device tensors, `set_levels` and `assign` are launches in stream order.

    python examples/level_replay.py --batch 4096 --steps 2000
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
ap.add_argument("--levels", type=int, default=512)
ap.add_argument("--replace", type=int, default=16, help="slots given a fresh level every --every steps")
ap.add_argument("--every", type=int, default=100)
args = ap.parse_args()
B, L = args.batch, args.levels

# auto_reset="next_step": the step after an episode's end is the env's reset — it plays the level set in between
env = make("MarlGrid-3AgentCluttered15x15-v0", batch_size=B, auto_reset="next_step", episode_info=True, max_steps=50, strict=False)
dev, n = env.device, env.num_agents
fresh = torch.Generator(dev).manual_seed(0)
bank = env.level_bank(torch.randint(0, 2 ** 62, (L,), device=dev, generator=fresh))
total = torch.zeros(L, device=dev)                  # per slot: minus the team returns of the episodes played on it, summed
plays = torch.zeros(L, device=dev)
slot = torch.randint(0, L, (B,), device=dev)        # the slot each env is pointed at
env.set_levels(bank, slot)
obs = env.reset()
for t in range(args.steps):
    actions = torch.randint(0, 3, (B, n), device=dev)                  # left / right / forward
    obs, rew, done, info = env.step(actions)
    # the finished episodes' returns go to the slots they were played on (`slot`; info["level"] is the level's seed)
    total.index_add_(0, slot, -info["episode_return"].sum(1).float() * done)
    plays.index_add_(0, slot, done.float())
    score = total / plays.clamp(min=1)
    # rank-prioritised sampling (PLR): weight 1 / rank, the highest score first
    rank = (-score).argsort().argsort().float() + 1
    nxt = torch.multinomial(1 / rank, B, replacement=True)
    slot = torch.where(done, nxt, slot)
    env.set_levels(bank, nxt, env_mask=done)                            # the others keep the slot they are playing
    if (t + 1) % args.every == 0:
        # the lowest-scored slots that were played have nothing left to teach: fresh levels in their place
        stale = torch.where(plays > 0, score, torch.full_like(score, float("inf"))).topk(args.replace, largest=False).indices
        bank.assign(stale, torch.randint(0, 2 ** 62, (args.replace,), device=dev, generator=fresh))
        total[stale] = 0
        plays[stale] = 0
    if (t + 1) % 500 == 0:
        print("step %5d: %d slots played, mean score %.3f, %d distinct levels running"
              % (t + 1, int((plays > 0).sum()), float((total / plays.clamp(min=1))[plays > 0].mean()), int(env.episode_level.unique().numel())))
env.check_errors()
