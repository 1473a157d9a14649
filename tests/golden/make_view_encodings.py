#!/usr/bin/env python
"""Generate tests/golden/viewenc_<scenario>.npz by EXECUTING THE REAL REFERENCE (/root/reference, through
tests/golden/refshim).  Build container only.

    python tests/golden/make_view_encodings.py [scenario ...]

For the first S seeds of a committed traj_<scenario>.npz the recorded actions are replayed on the live reference (a
caller-side reset after `done`, as make_golden.py recorded them).  The replay first checks every step's grid.encode()
against the trajectory's own `encode` array — the same trajectory — and records, per agent k,

    g, vis = env.gen_obs_grid(agent_k); g.encode(vis_mask=vis)          (base.py:418-451, 196-214)

at the constructor state, the reset state and the steps listed in `steps`.  Arrays only; no reference source is stored:
  seeds [S], actions [S][T][n] (the replayed prefix), reset_after [S][T], steps [K],
  ctor_a<k> [S][V_k][V_k][3], reset_a<k> [S][V_k][V_k][3], step_a<k> [S][K][V_k][V_k][3]   (uint8, index [i][j])
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import refload  # noqa: E402
import refstate  # noqa: E402
import scenarios  # noqa: E402

VIEWENC = {  # scenario -> (seeds, steps replayed, every how many steps the views are recorded)
    "MarlGrid-3AgentCluttered15x15-v0": (4, 120, 2),
    "Test-4AgentEmpty5x5-crowded": (4, 150, 1),
    "Test-4AgentEmpty5x5-hide": (4, 150, 1),
    "Test-3AgentCluttered9x9-hide": (4, 120, 1),
    "Test-3AgentEmpty7x7-spawn-delay": (4, 120, 1),
    "Test-3AgentCluttered9x9-respawn": (4, 150, 2),
    "Test-2AgentEmpty7x7-see-through": (4, 60, 1),
    "Edge-5AgentEmpty9x9-tile5-offset3": (4, 60, 1),
    "Test-3AgentCluttered9x9-hetero-views": (4, 100, 1),
    "Limit-3AgentCluttered33x33-view31-tile4": (2, 40, 4),
    "Limit-24AgentEmpty20x20-view5": (2, 60, 2),
    "Limit-3Agent100Kinds24x24": (3, 80, 2),
    "Limit-3AgentCluttered200x200-hide": (2, 40, 2),
    "Goalcycle-demo-solo-v0": (4, 150, 1),
}


def views(env):
    out = []
    for a in env.agents:
        g, vis = env.gen_obs_grid(a)
        out.append(np.asarray(g.encode(vis_mask=vis), np.uint8))
    return out


def gen(name, out):
    spec = scenarios.registered(name)
    recipe = scenarios.ref_recipe(name)
    S, T, every = VIEWENC[name]
    tr = np.load(os.path.join(HERE, "traj_%s.npz" % name))
    seeds, actions = tr["seeds"][:S], tr["actions"][:S, :T]
    n = actions.shape[2]
    steps = np.arange(0, T, every)
    Vk = [a.get("view", spec)["view_size"] for a in spec["agents"]]
    ctor = [np.zeros((S, v, v, 3), np.uint8) for v in Vk]
    rst = [np.zeros((S, v, v, 3), np.uint8) for v in Vk]
    stp = [np.zeros((S, len(steps), v, v, 3), np.uint8) for v in Vk]
    reset_after = np.zeros((S, T), bool)
    for si, seed in enumerate(seeds):
        env = refstate.make_ref_env(spec, recipe, seed=int(seed))
        for k, v in enumerate(views(env)):
            ctor[k][si] = v
        env.reset()
        for k, v in enumerate(views(env)):
            rst[k][si] = v
        ki = 0
        for t in range(T):
            _, _, dn, _ = env.step(actions[si, t])
            # the same trajectory as traj_<name>.npz: its grid.encode() of every step
            assert np.array_equal(env.grid.encode(), tr["encode"][si, t]), (name, si, t)
            if ki < len(steps) and steps[ki] == t:
                for k, v in enumerate(views(env)):
                    stp[k][si, ki] = v
                ki += 1
            if dn:
                assert tr["reset_after"][si, t]
                env.reset()
                reset_after[si, t] = True
    d = dict(seeds=seeds, actions=actions, reset_after=reset_after, steps=steps)
    for k in range(n):
        d["ctor_a%d" % k], d["reset_a%d" % k], d["step_a%d" % k] = ctor[k], rst[k], stp[k]
    np.savez_compressed(out, **d)


def main():
    refload.load()
    for name in sys.argv[1:] or list(VIEWENC):
        out = os.path.join(HERE, "viewenc_%s.npz" % name)
        gen(name, out)
        print("viewenc", name, os.path.getsize(out), flush=True)


if __name__ == "__main__":
    main()
