#!/usr/bin/env python
"""Memory maps at work (needs an MI355X): `MultiGridEnv(memory=True)` keeps, per agent, what every cell showed when the agent
last saw it (`env.memory`: type, colour, state, known) and at which step that was (`env.seen_step`) — on the device, by the one
launch behind every step that also keeps the exploration maps.  Random play on `MarlGrid-2AgentDoorKey8x8-v0`; printed for env
0: agent 0's memory next to the true grid (one letter per object type, `?` never seen, lower case where the memory is older
than `--old` steps), and for the batch the mean staleness of known cells, `step_count - seen_step`.

    python examples/memory_map.py --batch 512 --steps 40
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from marlgrid_amd.envs import make  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=512)
ap.add_argument("--steps", type=int, default=40)
ap.add_argument("--old", type=int, default=10)
args = ap.parse_args()
B = args.batch

env = make("MarlGrid-2AgentDoorKey8x8-v0", batch_size=B, seed=1337, auto_reset=False, max_steps=args.steps + 1, strict=False,
           place_obs=False, memory=True, obs_format="encoded")
dev, n, W, H = env.device, env.num_agents, env.width, env.height
gen = torch.Generator(dev).manual_seed(0)
env.reset()
for t in range(args.steps):
    env.step(torch.randint(0, 7, (B, n), device=dev, generator=gen))
env.check_errors()

# the true grid: MultiGrid.encode of every cell (objects; agents on empty cells)
truth = env.grid.encode()[0].cpu()
mem, stamp, now = env.memory[0, 0].cpu(), env.seen_step[0, 0].cpu(), int(env.step_count[0])
names = {}


def letter(type_idx):
    if type_idx == 0:
        return "."
    if type_idx not in names:
        names[type_idx] = "ABCDEFGHIJKLMNOPQRSTUVWXYZ"[len(names) % 26]
    return names[type_idx]


print("env 0 after %d steps: agent 0's memory   | the grid" % now)
for y in range(H):
    row = ""
    for x in range(W):
        t, _, _, known = mem[x, y].tolist()
        c = letter(t) if known else "?"
        row += c.lower() if known and now - int(stamp[x, y]) > args.old else c
    print(row + "   | " + "".join(letter(int(truth[x, y, 0])) for x in range(W)))
print("letters: %s" % ", ".join("%s = type %d" % (v, k) for k, v in sorted(names.items())))
known = env.memory[..., 3] == 1
age = (env.step_count[:, None, None, None] - env.seen_step)[known].float()
print("batch of %d: %.1f %% of the cells known per agent, mean staleness of known cells %.2f steps, oldest %d"
      % (B, 100.0 * float(known.float().mean()), float(age.mean()), int(age.max())))
assert bool((known == env.seen).all()) and bool(((env.seen_step >= 0) == env.seen).all())
