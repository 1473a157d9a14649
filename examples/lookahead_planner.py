#!/usr/bin/env python
"""Random shooting with the true model (needs an MI355X): every step, `env.lookahead` rolls K random plans of T actions forward
for every env — on a shadow copy of the state, the env itself untouched —, and the env executes the first action of the plan
that earned the most.  Two launches per decision, nothing goes to the host.

Printed: the mean episode return of the planner, of random play, and of an agent that follows `solve_distance(policy=True)`
(the optimum) on the same levels.  DoorKey needs the key, the door and the goal in a row, so a horizon that does not reach the goal
sees no reward at all: the planner then acts like random play — raise --horizon or --plans.

    python examples/lookahead_planner.py --batch 1024 --plans 64 --horizon 24
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from marlgrid_amd.envs import make  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=1024)
ap.add_argument("--plans", type=int, default=64)
ap.add_argument("--horizon", type=int, default=24)
ap.add_argument("--max-steps", type=int, default=60)
args = ap.parse_args()
B, K, T = args.batch, args.plans, args.horizon


def play(policy):
    """one episode per env from the same seeds -> mean return"""
    env = make("MarlGrid-1AgentDoorKey8x8-v0", batch_size=B, seed=1337, auto_reset=False, max_steps=args.max_steps, strict=False,
               place_obs=False)
    dev, n = env.device, env.num_agents
    gen = torch.Generator(dev).manual_seed(0)
    env.reset()
    total = torch.zeros(B, device=dev)
    over = torch.zeros(B, dtype=torch.bool, device=dev)
    rows = torch.arange(B, device=dev)
    for t in range(args.max_steps):
        if policy == "random":
            actions = torch.randint(0, 6, (B, n), device=dev, generator=gen)
        elif policy == "expert":
            actions = env.solve_distance(policy=True)[1]
        else:
            plans = torch.randint(0, 6, (K, T, B, n), device=dev, generator=gen)
            rewards, _ = env.lookahead(plans)                       # (K, T, B, n): 0 after a plan's episode has ended
            best = rewards.sum(dim=(1, 3)).argmax(dim=0)            # (B,): the plan that earned the most (ties: the first)
            actions = plans[best, 0, rows]
        _, rew, done, _ = env.step(actions)
        total += torch.where(over, torch.zeros_like(total), rew.sum(1))
        over |= done
    env.check_errors()
    return float(total.mean())


for policy in ("random", "planner", "expert"):
    print("%-8s mean return %.3f" % (policy, play(policy)))
