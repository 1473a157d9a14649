#!/usr/bin/env python
"""An ACCEL-shaped loop (needs an MI355X): evolve levels by EDITING them.  A level is (seed, parameters, a short list of cell
edits); a full `LevelBank` holds all three per slot, and an env that resets onto a slot takes the slot's generator, parameter row
and edit list in one launch.  Every so often the best-scored slots are parents: a child is the parent's seed and rows with ONE
edit entry changed — a wall put on, or taken off, a random interior cell —, written into the worst-scored slots with
`bank.assign(dst, bank.seeds[src], params=..., edits=...)`.  Finished envs are pointed at slots sampled by score rank with
`env_mask=done`.  Nothing goes to the host per step: scores, sampling, the children and their edits are device tensors.

    python examples/level_editing.py --batch 4096 --steps 2000
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from marlgrid_amd.envs import make  # noqa: E402
from marlgrid_amd.objects import Wall  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=4096)
ap.add_argument("--steps", type=int, default=2000)
ap.add_argument("--levels", type=int, default=256)
ap.add_argument("--edits", type=int, default=8, help="edit entries per level (level_edits)")
ap.add_argument("--children", type=int, default=16, help="children written every --every steps")
ap.add_argument("--every", type=int, default=100)
args = ap.parse_args()
B, L, K, C = args.batch, args.levels, args.edits, args.children

env = make("MarlGrid-3AgentClutteredCurriculum15x15-v0", batch_size=B, auto_reset="next_step", episode_info=True, max_steps=50,
           strict=False, level_edits=K)
dev, n = env.device, env.num_agents
wall = env.edit_key(Wall())
gen = torch.Generator(dev).manual_seed(0)
bank = env.level_bank(L, full=True)
bank.assign(None, torch.randint(0, 2 ** 62, (L,), device=dev, generator=gen),
            params=dict(n_clutter=torch.randint(0, 31, (L,), device=dev, generator=gen)))
total = torch.zeros(L, device=dev)                  # per slot: minus the team returns of the episodes played on it, summed
plays = torch.zeros(L, device=dev)
slot = torch.randint(0, L, (B,), device=dev, generator=gen)
env.set_levels(bank, slot)
obs = env.reset()
col = bank.columns["n_clutter"]
for t in range(args.steps):
    actions = torch.randint(0, 3, (B, n), device=dev, generator=gen)   # left / right / forward
    obs, rew, done, info = env.step(actions)
    total.index_add_(0, slot, -info["episode_return"].sum(1).float() * done)
    plays.index_add_(0, slot, done.float())
    score = total / plays.clamp(min=1)
    rank = (-score).argsort().argsort().float() + 1
    nxt = torch.multinomial(1 / rank, B, replacement=True)
    slot = torch.where(done, nxt, slot)
    env.set_levels(bank, nxt, env_mask=done)                            # the others keep the level they are playing
    if (t + 1) % args.every == 0:
        played = plays > 0
        src = torch.where(played, score, torch.full_like(score, -float("inf"))).topk(C).indices          # parents: the hardest
        dst = torch.where(played, score, torch.full_like(score, float("inf"))).topk(C, largest=False).indices
        # child = the parent's rows with one entry changed: entry k becomes (x, y, wall or nothing, on) at a random interior cell
        child = bank.edits[src].clone()
        k = torch.randint(0, K, (C,), device=dev, generator=gen)
        cell = torch.randint(1, env.width - 1, (C, 2), device=dev, generator=gen)
        kind = torch.randint(0, 2, (C,), device=dev, generator=gen) * wall
        child[torch.arange(C, device=dev), k] = torch.stack([cell[:, 0], cell[:, 1], kind, torch.ones_like(kind)], 1).to(torch.uint8)
        bank.assign(dst, bank.seeds[src], params=dict(n_clutter=bank.params[src, col]), edits=child)
        total[dst] = 0
        plays[dst] = 0
    if (t + 1) % 500 == 0:
        on = (bank.edits[:, :, 3] != 0).sum(1).float()
        print("step %5d: %d slots played, mean score %.3f, %.2f edits per level, %d distinct seeds in the bank"
              % (t + 1, int((plays > 0).sum()), float((total / plays.clamp(min=1))[plays > 0].mean()), float(on.mean()),
                 int(bank.seeds.unique().numel())))
env.check_errors()
