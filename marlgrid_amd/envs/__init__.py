"""Scenario classes and the ids the reference registers with gym (marlgrid/envs/__init__.py:20-121).

gym is not a dependency: ids live in a module-level table and `make(id, batch_size=..., device=...)`
stands in for `gym.make`.

`DoorKeyEnv` is upstream's envs/doorkey.py with gym-minigrid's `_rand_int` (upstream's own cannot be constructed: it never
defines the method, doorkey.py:26,34).  Its `_gen_grid` lays the room out from random draws — `MultiGridEnv._rand_int`
inside `_gen_grid` is recorded and drawn per env on the device at every reset.  A recorded `_gen_grid` may compute with a
draw (`draw +- int`) and use it as a coordinate or extent of put_obj / grid.set / the wall helpers, in place_obj's `top` /
`size` and as a bound of a later `_rand_int`.  To BRANCH on one (compare it, index or loop with it, choose an object by
it) `_gen_grid` asks for its value with `self._fork(draw)`, or draws with `self._rand_elem(...)` / `self._rand_bool()`: it is
then recorded once per path and every env runs the ops of its own path (`ColoredDoorKeyEnv`: a door and key of one of six
colours).  `self._param(name, lo, hi)` is used like a draw but read per env from `env.params[name]` (`env.set_params`) at every
reset: `ClutteredMultiGrid(n_clutter_max=K)` scatters `count=self._param("n_clutter", 0, K + 1)` blocks.  `_gen_grid` still
cannot put a draw or a parameter into `agent_spawn_kwargs` or have a `reject_fn` that depends on one.  Upstream registers
no DoorKey id; the ids in `extension_envs` are this package's own and are built by `make` like the registered ones, and so
are the one-agent DoorKey ids in `solo_envs` (`env.solve_distance(policy=True)` is followed by an agent that has its level
to itself).
"""
import functools
import random

from ..agents import GridAgentInterface
from ..base import MultiGridEnv
from .scenarios import (ClutteredGoalCycleEnv, ClutteredMultiGrid, ColoredDoorKeyEnv, DoorKeyEnv, EmptyMultiGrid,  # noqa: F401
                        VisibilityTestEnv)

_PALETTE = ("red", "blue", "purple", "orange", "olive", "pink")     # per-slot agent colours of a registered id
_registry = {}            # id -> factory(**constructor kwargs)
registered_envs = []      # ids, in registration order (upstream's list of the same name)
extension_envs = []       # ids upstream does not register (DoorKey): `make` builds them, `registered_envs` stays upstream's list
solo_envs = []            # ... and their one-agent forms (following `solve_distance`'s policy needs the level to oneself): `make` builds
_solo_registry = {}       # them too, from a table of their own — `_registry` and `extension_envs` are the ids whose recordings and
                          # launch tables are pinned one by one


def _construct(env_class, n_agents, geometry, agent_color, fixed, **extra):
    view_size, view_offset = geometry
    team = [GridAgentInterface(color=agent_color or _PALETTE[i], view_size=view_size, view_offset=view_offset,
                               view_tile_size=8)           # upstream hard-codes 8 here whatever it was given (:42)
            for i in range(n_agents)]
    return env_class(agents=team, **dict(fixed, **extra))


def register_marl_env(env_name, env_class, n_agents, grid_size, view_size, view_tile_size=8, view_offset=0,
                      agent_color=None, env_kwargs={}, listed_in=None):
    """Same signature as upstream (:20-55).  `view_tile_size` is accepted and — as upstream — ignored.  `listed_in` (not
    upstream's): the list of ids the new one joins, `registered_envs` unless given (`extension_envs` for this package's own)."""
    if n_agents > len(_PALETTE):
        raise AssertionError("a registered id has at most %d agents" % len(_PALETTE))
    _registry[env_name] = functools.partial(_construct, env_class, n_agents, (view_size, view_offset), agent_color,
                                            dict(env_kwargs, grid_size=grid_size))
    (registered_envs if listed_in is None else listed_in).append(env_name)


def make(env_name, pipeline=None, devices=None, **kwargs):
    """`gym.make` stand-in; kwargs (batch_size, device, seed, seeds, auto_reset, strict, ...) reach the env.

    pipeline=P (P >= 2): the batch as P independent envs of batch_size / P on P streams — a
    `marlgrid_amd.sharding.ShardPipeline` whose parts a sampler steps in turn (`pipe.step_part(k, actions)` under
    `pipe.on(k)`): the launches of independent shards overlap (+10 % at 32 768 envs, +17 % at 65 536 on one
    MI355X), and env g of the batch keeps its seed `seed + g`, so trajectories are those of the one big env.

    devices=[...] (torch devices, strs or ints; entries may repeat): the batch sharded over these devices in ONE process
    — a `marlgrid_amd.sharding.DeviceShards`: shard k is an env of `shard_range(batch_size, k, len(devices))` on
    devices[k] with its own stream, `step(actions)` issues every shard's launch from the calling thread, `gather()` joins
    what they return; env g keeps its seed `seed + g`.  Every other kwarg reaches every shard's env unchanged, except that
    a device named m > 1 times gives its shards `share=m` in `place_obs`.  Not together with `pipeline`, `seeds` or
    `device`."""
    try:
        factory = _registry[env_name] if env_name in _registry else _solo_registry[env_name]
    except KeyError:
        raise KeyError("unknown env id %r; registered: %s" % (env_name, ", ".join(registered_envs + extension_envs + solo_envs))) from None
    if devices is not None:
        from ..sharding import DeviceShards, merge_share
        if pipeline is not None:
            raise ValueError("make(devices=) and make(pipeline=) are two ways to split one batch: give one of them")
        if "seeds" in kwargs:
            raise ValueError("make(devices=): per-env seeds come from `seed` + the env's index in the whole batch")
        if kwargs.get("device") is not None:
            raise ValueError("make(devices=): the shards' devices are `devices`; `device` has no meaning next to it")
        kwargs.pop("device", None)
        batch_size, seed, streams = kwargs.pop("batch_size", 1), kwargs.pop("seed", 1337), kwargs.pop("streams", None)
        place_obs = kwargs.pop("place_obs", True)
        return DeviceShards(lambda batch_size, seeds, device, share=1: factory(
            batch_size=batch_size, seeds=seeds, device=device, place_obs=merge_share(place_obs, share), **kwargs),
            batch_size, devices, seed=seed, streams=streams)
    if pipeline is None or int(pipeline) <= 1:
        return factory(**kwargs)
    from ..sharding import ShardPipeline
    if "seeds" in kwargs:
        raise ValueError("make(pipeline=): per-env seeds come from `seed` + the env's index in the whole batch")
    batch_size, seed, device = kwargs.pop("batch_size"), kwargs.pop("seed", 1337), kwargs.pop("device", None)
    streams = kwargs.pop("streams", None)
    return ShardPipeline(lambda batch_size, seeds, device: factory(batch_size=batch_size, seeds=seeds, device=device, **kwargs),
                         batch_size, parts=int(pipeline), seed=seed, device=device, streams=streams)


def _scenario_classes():
    found, todo = {}, [MultiGridEnv]
    while todo:
        cls = todo.pop()
        found[cls.__name__] = cls
        todo.extend(cls.__subclasses__())
    return found


def env_from_config(env_config, randomize_seed=True):
    """Build the scenario class named by `env_config["env_class"]` from the rest of the dict (:58-67)."""
    spec = dict(env_config)
    env_class = _scenario_classes()[spec.pop("env_class")]
    if randomize_seed:
        spec["seed"] = spec.get("seed", 0) + random.randint(0, 1337 * 1337)
    return env_class(**spec)


# (id, class, agents, grid, view, view_offset, scenario kwargs) — upstream :70-121.  Its
# "1AgentCluttered15x15" really is an 11x11 room seen through a 5x5 view.
for _row in (
        ("MarlGrid-1AgentCluttered15x15-v0", ClutteredMultiGrid, 1, 11, 5, 0, dict(n_clutter=30)),
        ("MarlGrid-3AgentCluttered11x11-v0", ClutteredMultiGrid, 3, 11, 7, 0, dict(clutter_density=0.15)),
        ("MarlGrid-3AgentCluttered15x15-v0", ClutteredMultiGrid, 3, 15, 7, 0, dict(clutter_density=0.15)),
        ("MarlGrid-2AgentEmpty9x9-v0", EmptyMultiGrid, 2, 9, 7, 0, {}),
        ("MarlGrid-3AgentEmpty9x9-v0", EmptyMultiGrid, 3, 9, 7, 0, {}),
        ("MarlGrid-4AgentEmpty9x9-v0", EmptyMultiGrid, 4, 9, 7, 0, {}),
        ("Goalcycle-demo-solo-v0", ClutteredGoalCycleEnv, 1, 13, 7, 1, dict(clutter_density=0.1, n_bonus_tiles=3)),
):
    register_marl_env(_row[0], _row[1], n_agents=_row[2], grid_size=_row[3], view_size=_row[4], view_offset=_row[5],
                      env_kwargs=_row[6])
for _row in (("MarlGrid-2AgentDoorKey6x6-v0", 6), ("MarlGrid-2AgentDoorKey8x8-v0", 8)):
    register_marl_env(_row[0], DoorKeyEnv, n_agents=2, grid_size=_row[1], view_size=7, listed_in=extension_envs)
register_marl_env("MarlGrid-2AgentColoredDoorKey8x8-v0", ColoredDoorKeyEnv, n_agents=2, grid_size=8, view_size=7,
                  listed_in=extension_envs)
for _row in (("MarlGrid-1AgentDoorKey6x6-v0", 6), ("MarlGrid-1AgentDoorKey8x8-v0", 8)):
    _solo_registry[_row[0]] = functools.partial(_construct, DoorKeyEnv, 1, (7, 0), None, dict(grid_size=_row[1]))
    solo_envs.append(_row[0])
# a curriculum over the clutter: every env reads its number of wall blocks, 0 .. 50, from `env.params["n_clutter"]` when it resets
register_marl_env("MarlGrid-3AgentClutteredCurriculum15x15-v0", ClutteredMultiGrid, n_agents=3, grid_size=15, view_size=7,
                  env_kwargs=dict(n_clutter=25, n_clutter_max=50), listed_in=extension_envs)
del _row
