"""What `_sync_tables()` leaves per view group — launch config, object table, atlas (gather copy included), hide table, spawn
reject table, kernel name, warnings — for a list of envs, as plain data: tests/golden/launch_tables.json is what the tree made of
the list BEFORE the derivation moved to marlgrid_amd/launch_tables.py (`python tests/launch_table_cases.py record [--tree DIR]`),
tests/test_launch_tables_host.py holds every later tree to it.  No device: the env is built dry and `_sync_tables()` then runs
whole with its uploads going to CPU tensors (the library answers kernel names and LDS sizes on the host)."""
import hashlib
import json
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "launch_tables.json")
POINTERS = ("hide_by_obj", "obj", "atlas", "spawn_reject")
SHAPES = ((8, 7, {}), (5, 7, {}), (11, 7, {}), (6, 5, dict(hide_item_types=["Wall"])), (8, 7, dict(color="prestige")), (7, 9, {}))
REJECT_CALLS = []


def _reject(pos):       # (a function of the position alone; every call is counted)
    REJECT_CALLS.append((int(pos[0]), int(pos[1])))
    return (pos[0] + pos[1]) % 3 == 0


def _empty(agents, grid_size=9, **kw):
    from marlgrid_amd.agents import GridAgentInterface
    from marlgrid_amd.envs import EmptyMultiGrid
    return EmptyMultiGrid(agents=[GridAgentInterface(**a) for a in agents], grid_size=grid_size, _dry=True, **kw)


def two_groups_reject():
    """two view groups (8- and 5-pixel tiles) and a reject_fn over a 4 x 5 spawn rectangle"""
    env = _empty([dict(view_tile_size=8), dict(view_tile_size=5, color="blue")])
    env.agent_spawn_kwargs = dict(reject_fn=_reject, top=(1, 1), size=(4, 5))      # (the scenario's `_gen_grid` ends with {})
    return env


def case_names():
    from marlgrid_amd import envs as E
    return (list(E.registered_envs) + list(E.extension_envs) + ["Fuzz-%d" % i for i in range(120)]
            + ["Test-2AgentReject9x9", "Limit-3Agent100Kinds24x24"] + ["shape-%d" % i for i in range(len(SHAPES))]
            + ["two-groups-reject", "three-agents-prestige", "grid-in-place-200", "tile5-no-gather-atlas", "tile5-encoded"])


def build(name):
    import product_envs
    if name.startswith("shape-"):
        ts, vs, kw = SHAPES[int(name[6:])]
        return _empty([dict(view_tile_size=ts, view_size=vs, **kw)])
    if name == "two-groups-reject":
        return two_groups_reject()
    if name == "three-agents-prestige":
        return _empty([dict(view_tile_size=8), dict(view_tile_size=8, color="blue", spawn_delay=2),
                       dict(view_tile_size=8, color="prestige", prestige_beta=0.9, prestige_scale=3)], max_steps=33, respawn=True)
    if name == "grid-in-place-200":
        return _empty([dict(view_tile_size=8)], grid_size=200)
    if name == "tile5-no-gather-atlas":
        return _empty([dict(view_tile_size=5)])
    if name == "tile5-encoded":
        return _empty([dict(view_tile_size=5)], obs_format="encoded")
    return product_envs.build(name, _dry=True)


def on_cpu(env):
    """a dry env whose `_sync_tables()` runs whole: the uploads become CPU tensors"""
    import torch
    env._dry, env.device = False, torch.device("cpu")
    return env


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def row(name):
    from marlgrid_amd import base
    env = on_cpu(build(name))
    base._GENERIC_WARNED.clear()        # (the warning is said once per configuration and process: every case starts unsaid)
    no_gather = name == "tile5-no-gather-atlas"
    if no_gather:
        os.environ["MG_NO_GATHER_ATLAS"] = "1"
    try:
        with warnings.catch_warnings(record=True) as said:
            warnings.simplefilter("always")
            env._sync_tables()
    finally:
        if no_gather:
            del os.environ["MG_NO_GATHER_ATLAS"]
    groups = []
    for g in env._groups:
        cfg = type(g.cfg).from_buffer_copy(g.cfg)
        for p in POINTERS:
            setattr(cfg, p, None)
        atlas = g.atlas_dev.numpy()
        groups.append(dict(cfg=_sha(np.frombuffer(bytes(cfg), np.uint8)), obj=_sha(g.obj_dev.numpy()), atlas=_sha(atlas),
                           atlas_bytes=int(atlas.size), atlas_gather_off=int(g.cfg.atlas_gather_off),
                           hide_by=None if g.hide_dev is None else g.hide_dev.numpy().view(np.uint32).tolist(),
                           has_reject=bool(g.cfg.spawn_reject), kernel_name=g.kernel_name))
    rej = None
    if groups[0]["has_reject"]:
        t = env._spawn_reject_dev.numpy()[:env.width * env.height].reshape(env.width, env.height)
        rej = [[int(x), int(y)] for x, y in np.argwhere(t)]
    return dict(groups=groups, spawn_reject=rej, warnings=[str(w.message) for w in said])


def record():
    return {name: row(name) for name in case_names()}


def time_fast_path(calls=200000, legs=5):
    """median ns of `_sync_tables()` when nothing changed — what every step pays —, on the bench configuration's env"""
    import time
    from marlgrid_amd.envs import make
    env = on_cpu(make("MarlGrid-3AgentCluttered15x15-v0", batch_size=32768, auto_reset=True, _dry=True))
    env._sync_tables()
    sync, out = env._sync_tables, []
    for _ in range(legs):
        t0 = time.perf_counter()
        for _ in range(calls):
            sync()
        out.append(round((time.perf_counter() - t0) / calls * 1e9, 1))
    return out


if __name__ == "__main__":
    tree = sys.argv[sys.argv.index("--tree") + 1] if "--tree" in sys.argv else os.path.dirname(HERE)
    sys.path.insert(0, tree)
    if sys.argv[1] == "record":
        rec = record()
        with open(GOLDEN, "w") as f:
            json.dump(rec, f, indent=0, sort_keys=True)
        print("%d cases, %d groups" % (len(rec), sum(len(r["groups"]) for r in rec.values())))
    elif sys.argv[1] == "time":
        print(json.dumps({"ns_per_sync_tables": time_fast_path()}))
