#!/usr/bin/env python
"""examples/level_editing.py with EXACT regret (needs an MI355X): the same ACCEL-shaped loop — levels are (seed, parameters, a
short list of cell edits) in a full `LevelBank`, children are parents with one edit entry changed — but a level is scored by what
an optimal agent would have earned on it minus what the agents did earn, and a level that cannot be solved is not replayed.

After each step, `env.goal_distance(env_mask=info["reset"])` analyses the envs that were just reset onto a level: one launch, a
wave per such env, a breadth-first search over the env's own grid in HBM.  `env.optimal_return(dist)` turns the distances into the
return of a shortest path.  A slot whose level left any agent without a path to the goal (an edit can wall the goal off) gets
score -inf: it is never a parent and is the first to be overwritten.  Every other slot's score is the mean regret
`optimal_return - episode_return` of the episodes played on it.  Nothing goes to the host per step.

    python examples/level_regret.py --batch 4096 --steps 2000
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
total = torch.zeros(L, device=dev)                  # per slot: the regrets of the episodes played on it, summed
plays = torch.zeros(L, device=dev)
unsolvable = torch.zeros(L, dtype=torch.bool, device=dev)
slot = torch.randint(0, L, (B,), device=dev, generator=gen)
env.set_levels(bank, slot)
obs = env.reset()
dist = env.goal_distance()
best = env.optimal_return(dist).sum(1).float()                          # (B,): what the team could earn on the running level
unsolvable[slot[(dist < 0).any(1)]] = True
col = bank.columns["n_clutter"]
inf = float("inf")
for t in range(args.steps):
    actions = torch.randint(0, 3, (B, n), device=dev, generator=gen)   # left / right / forward
    obs, rew, done, info = env.step(actions)
    regret = best - info["episode_return"].sum(1).float()
    total.index_add_(0, slot, regret * done)
    plays.index_add_(0, slot, done.float())
    # the envs whose call was their reset have a new grid: analyse those, and only those
    fresh = info["reset"]
    dist = env.goal_distance(env_mask=fresh)
    best = torch.where(fresh, env.optimal_return(dist).sum(1).float(), best)
    unsolvable |= torch.zeros(L, device=dev).index_add_(0, slot, (fresh & (dist < 0).any(1)).float()) > 0
    score = torch.where(unsolvable, torch.full_like(total, -inf), total / plays.clamp(min=1))
    rank = (-score).argsort().argsort().float() + 1
    nxt = torch.multinomial(torch.where(unsolvable, torch.zeros_like(rank), 1 / rank) + 1e-12, B, replacement=True)
    slot = torch.where(done, nxt, slot)
    env.set_levels(bank, nxt, env_mask=done)                            # the others keep the level they are playing
    if (t + 1) % args.every == 0:
        played = (plays > 0) & ~unsolvable
        src = torch.where(played, score, torch.full_like(score, -inf)).topk(C).indices                  # parents: the highest regret
        # overwritten first: the unsolvable slots (-inf), then the lowest regret
        dst = torch.where(played | unsolvable, score, torch.full_like(score, inf)).topk(C, largest=False).indices
        child = bank.edits[src].clone()
        k = torch.randint(0, K, (C,), device=dev, generator=gen)
        cell = torch.randint(1, env.width - 1, (C, 2), device=dev, generator=gen)
        kind = torch.randint(0, 2, (C,), device=dev, generator=gen) * wall
        child[torch.arange(C, device=dev), k] = torch.stack([cell[:, 0], cell[:, 1], kind, torch.ones_like(kind)], 1).to(torch.uint8)
        bank.assign(dst, bank.seeds[src], params=dict(n_clutter=bank.params[src, col]), edits=child)
        total[dst] = 0
        plays[dst] = 0
        unsolvable[dst] = False
    if (t + 1) % 500 == 0:
        ok = (plays > 0) & ~unsolvable
        print("step %5d: %d slots played, %d unsolvable, mean regret %.3f"
              % (t + 1, int(ok.sum()), int(unsolvable.sum()), float((total / plays.clamp(min=1))[ok].mean())))
env.check_errors()
