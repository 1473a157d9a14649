"""Sharding of the env batch: contiguous env slices, no collective on the data path (envs are fully independent: own
grid, agents and RNG — marlgrid/base.py:371-374).  Three ways to drive the slices:

  * one process per GPU (bench.py --gpus N): `shard_range` / `shard_seeds`; only the benchmark's wall-clock is reduced over
    ranks (MAX);
  * `ShardPipeline`: the batch of ONE GPU as independent envs on as many streams, for a double-buffered sampler;
  * `DeviceShards`: ONE process, one env per entry of a device list, every step issued from the calling thread.

Env g of the global batch is seeded `seed + g` whatever the sharding, so all three step the trajectories of the one big env,
and a checkpoint of one (`merge_state_dicts` / `split_state_dict`) loads into any other."""
import contextlib


def shard_range(global_batch, rank, world_size):
    """Contiguous slice [lo, hi) of the global env ids owned by `rank` (sizes differ by at most 1)."""
    if not (0 <= rank < world_size):
        raise ValueError("rank out of range")
    base, rem = divmod(int(global_batch), int(world_size))
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def shard_seeds(base_seed, global_batch, rank, world_size):
    """Per-env seeds of this rank's slice: env with global id g is seeded base_seed + g, whatever the
    sharding — which is what makes trajectories shard-invariant."""
    lo, hi = shard_range(global_batch, rank, world_size)
    return [int(base_seed) + g for g in range(lo, hi)]


def shard_ranges(global_batch, world_size):
    """[shard_range(global_batch, k, world_size) for every k]: a partition of [0, global_batch) in order.  Raises
    ValueError for an empty world or a batch with fewer envs than shards (a shard without envs is not an env)."""
    world_size = int(world_size)
    if world_size < 1:
        raise ValueError("at least one shard is needed")
    if int(global_batch) < world_size:
        raise ValueError("batch_size (%d) must be at least the number of shards (%d)" % (int(global_batch), world_size))
    return [shard_range(global_batch, k, world_size) for k in range(world_size)]


def merge_share(place_obs, share):
    """The `place_obs` of a shard whose device carries `share` shards of one DeviceShards: the placement search of each
    counts on 1 / share of the free memory (MgPlaceTuning.share).  True / "search" / "thorough" become the equivalent dict
    plus `share`; a dict keeps a `share` of its own; False stays False; with share <= 1 nothing changes."""
    share = int(share)
    if share <= 1 or place_obs is False or place_obs is None:
        return place_obs
    if place_obs is True or place_obs == "search":
        return {"share": share}
    if place_obs == "thorough":
        return {"thorough": True, "share": share}
    if isinstance(place_obs, dict):
        return dict({"share": share}, **place_obs)
    return place_obs          # (not a value MultiGridEnv accepts: its constructor says so)


def _engine_version():
    from .base import STATE_DICT_VERSION
    return STATE_DICT_VERSION


def merge_state_dicts(dicts):
    """`MultiGridEnv.state_dict()`s of consecutive slices of a batch -> the state_dict of the whole batch: every tensor
    concatenated along dim 0 in the order given, `version` checked (equal everywhere, and the one this engine reads).  The
    optional keys (`prestige_t`, `ep_return_t`, `params_t`, `edits_t`, `seen` with `visits`, `memory` with `seen_step`, and `episode_level_t` with `level_next_t`) are in every dict or in none: anything else raises KeyError.  Pure: no
    device is touched beyond what torch.cat does with the tensors it is given (all on one device)."""
    import torch
    dicts = list(dicts)
    if not dicts:
        raise ValueError("merge_state_dicts: nothing to merge")
    keys = set(dicts[0].keys())
    for i, d in enumerate(dicts):
        if set(d.keys()) != keys:
            raise KeyError("merge_state_dicts: shard %d has the keys %s, shard 0 has %s" % (i, sorted(d.keys()), sorted(keys)))
    if "version" not in keys:
        raise KeyError("merge_state_dicts: no 'version' (a checkpoint without it predates the look-ahead RNG form)")
    versions = [int(d["version"]) for d in dicts]
    if len(set(versions)) != 1 or versions[0] != _engine_version():
        raise ValueError("merge_state_dicts: checkpoint versions %s, this engine reads %d" % (sorted(set(versions)), _engine_version()))
    out = {k: torch.cat([d[k] for d in dicts], dim=0) for k in sorted(keys - {"version"})}
    out["version"] = dicts[0]["version"].clone()
    return out


def split_state_dict(sd, ranges):
    """The inverse: the state_dict of a whole batch -> one per (lo, hi) of `ranges` (views of the rows lo .. hi of every
    tensor, `version` copied).  `ranges` must partition [0, batch) in order; `version` must be the one this engine reads."""
    ranges = [(int(lo), int(hi)) for lo, hi in ranges]
    if "version" not in sd:
        raise KeyError("split_state_dict: no 'version' (a checkpoint without it predates the look-ahead RNG form)")
    if int(sd["version"]) != _engine_version():
        raise ValueError("split_state_dict: checkpoint version %d, this engine reads %d" % (int(sd["version"]), _engine_version()))
    at = 0
    for lo, hi in ranges:
        if lo != at or hi <= lo:
            raise ValueError("split_state_dict: ranges must partition the batch in order (got %s)" % (ranges,))
        at = hi
    for k, v in sd.items():
        if k != "version" and v.shape[0] != at:
            raise ValueError("split_state_dict: %s has %d rows, the ranges cover %d" % (k, v.shape[0], at))
    return [dict({k: v[lo:hi] for k, v in sd.items() if k != "version"}, version=sd["version"].clone()) for lo, hi in ranges]


def split_params(ranges, env_mask=None, env_ids=None, _who="set_params", **values):
    """`MultiGridEnv.set_params` arguments in GLOBAL env order -> one dict of keyword arguments per (lo, hi) of `ranges` (None
    for a shard that none of `env_ids` falls into): rows lo .. hi of `env_mask` and of every per-env value, `env_ids` of the
    shard rebased to it together with their values.  `env_ids` are read on the host (a device tensor is copied: a host
    sync); masks and values may stay on their device — they are only sliced.  `_who`: the caller's name in the messages."""
    import numpy as np
    from . import per_env as P
    ranges = [(int(lo), int(hi)) for lo, hi in ranges]
    B = ranges[-1][1]
    P.check_selectors(B, env_mask, env_ids, _who)
    ids = None if env_ids is None else P.host_ids(env_ids, B, _who, any_number=True)
    for name, v in values.items():
        P.check_value_shape(P.shape_of(v), B, None if ids is None else len(ids), "%s(%s=)" % (_who, name))
    out = []
    for lo, hi in ranges:
        kw = {}
        if env_mask is not None:
            kw["env_mask"] = env_mask[lo:hi]
        sel = None
        if ids is not None:
            sel = np.nonzero((ids >= lo) & (ids < hi))[0]
            if not sel.size:
                out.append(None)
                continue
            kw["env_ids"] = ids[sel] - lo
        for name, v in values.items():
            if P.shape_of(v) == ():
                kw[name] = v
            elif ids is not None and P.shape_of(v) == (len(ids),):
                v = v if hasattr(v, "shape") else np.asarray(v)
                kw[name] = v[sel] if isinstance(v, np.ndarray) else v[sel.tolist()]
            else:
                kw[name] = (v if hasattr(v, "shape") else np.asarray(v))[lo:hi]
        out.append(kw)
    return out


def _host_ids(env_ids, B, who):
    """global env ids on the host, range-checked (a device tensor is copied: a host sync)"""
    from . import per_env as P
    return P.host_ids(env_ids, B, who, any_number=True)


def split_levels(ranges, ids=None, seeds=None, env_mask=None, env_ids=None):
    """`MultiGridEnv.set_levels` arguments in GLOBAL env order -> one dict of keyword arguments per (lo, hi) of `ranges` (None for
    a shard that none of `env_ids` falls into), as `split_params` splits a parameter: exactly one of `ids` (bank slots) and
    `seeds`, an int or one value per env.  The bank is not part of it (a shard reads a replica on its own device)."""
    if (ids is None) == (seeds is None):
        raise ValueError("set_levels: either (bank, ids) or seeds=")
    return split_params(ranges, env_mask, env_ids, "set_levels", **({"ids": ids} if ids is not None else {"seeds": seeds}))


def split_edits(ranges, edits, env_mask=None, env_ids=None):
    """`MultiGridEnv.set_edits` arguments in GLOBAL env order -> one dict of keyword arguments per (lo, hi) of `ranges` (None for
    a shard that none of `env_ids` falls into), `split_params`' pattern: a (K', 4) list goes to every shard as it is, one list
    per env — (B, K', 4), or (k, K', 4) with `env_ids` — is sliced or picked by rows."""
    import numpy as np
    from . import per_env as P
    ranges = [(int(lo), int(hi)) for lo, hi in ranges]
    B = ranges[-1][1]
    P.check_selectors(B, env_mask, env_ids, "set_edits")
    ids = None if env_ids is None else P.host_ids(env_ids, B, "set_edits", any_number=True)
    edits = edits if hasattr(edits, "shape") else np.asarray(edits)
    per_env = len(edits.shape) == 3
    if per_env and edits.shape[0] not in ((B,) if ids is None else (B, len(ids))):
        raise ValueError("set_edits(edits=): one list per selected env, (%d, K', 4); got %s"
                         % (B if ids is None else len(ids), tuple(edits.shape)))
    out = []
    for lo, hi in ranges:
        kw = {}
        if env_mask is not None:
            kw["env_mask"] = env_mask[lo:hi]
        sel = None
        if ids is not None:
            sel = np.nonzero((ids >= lo) & (ids < hi))[0]
            if not sel.size:
                out.append(None)
                continue
            kw["env_ids"] = ids[sel] - lo
        if not per_env:
            kw["edits"] = edits
        elif ids is not None and edits.shape[0] == len(ids):
            kw["edits"] = edits[sel] if isinstance(edits, np.ndarray) else edits[sel.tolist()]
        elif ids is not None:
            rows = ids[sel]
            kw["edits"] = edits[rows] if isinstance(edits, np.ndarray) else edits[rows.tolist()]
        else:
            kw["edits"] = edits[lo:hi]
        out.append(kw)
    return out


def max_over_ranks(value, device=None):
    """MAX-reduce a python float over the default process group (returns it unchanged when
    torch.distributed is not initialised)."""
    import torch
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return float(value)
    t = torch.tensor([float(value)], dtype=torch.float64, device=device)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def sum_over_ranks(value, device=None):
    import torch
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return float(value)
    t = torch.tensor([float(value)], dtype=torch.float64, device=device)
    dist.all_reduce(t, op=dist.ReduceOp.SUM)
    return float(t.item())


class _Shards(object):
    """What ShardPipeline and DeviceShards share: `envs`, one stream per env (`streams`), the global rows of each
    (`ranges`), and everything that is the same loop over them.  A subclass says how shard k's context is entered (`on`)."""

    envs = ()
    streams = ()
    ranges = ()

    # what a training loop asks an env for
    @property
    def num_agents(self):
        return self.envs[0].num_agents

    @property
    def agents(self):
        """shard 0's agent interfaces (every shard has its own, bound to its own env: agent.pos etc. are per shard)"""
        return self.envs[0].agents

    @property
    def action_space(self):
        return self.envs[0].action_space

    @property
    def observation_space(self):
        return self.envs[0].observation_space

    def _each(self, fn):
        out = []
        for k, env in enumerate(self.envs):
            with self.on(k):
                out.append(fn(k, env))
        return out

    def close(self):
        self.synchronize()
        self.envs = []

    def synchronize(self):
        for s in self.streams:
            s.synchronize()

    def check_errors(self):
        """every shard's check_errors(), each under its own stream (an env waits for every stream it launched on, so
        this also holds for shards that were stepped one by one from elsewhere)"""
        self._each(lambda k, env: env.check_errors())

    def state_dict(self):
        """ONE checkpoint of the whole batch, in global env order, on the CPU: exactly the keys and shapes the one big env's
        `state_dict()` has at this batch size (`merge_state_dicts` of the shards').  It loads into that env, and into any
        other split of the batch — `load_state_dict` of a ShardPipeline or a DeviceShards with other shards.  Host sync."""
        return merge_state_dicts(self._each(lambda k, env: {key: v.cpu() for key, v in env.state_dict().items()}))

    def set_params(self, env_mask=None, env_ids=None, **values):
        """`MultiGridEnv.set_params` for the whole batch: `env_mask`, `env_ids` and per-env values in GLOBAL env order, split
        by `ranges` (`split_params`); every shard's part is written on its own stream"""
        parts = split_params(self.ranges, env_mask=env_mask, env_ids=env_ids, **values)
        self._each(lambda k, env: None if parts[k] is None else env.set_params(**parts[k]))

    def level_bank(self, seeds_or_capacity, full=False):
        """`MultiGridEnv.level_bank` of shard 0 (every shard declares the same parameters and `level_edits`): the bank that
        `set_levels(bank, ids)` takes; the shards read replicas of it on their own devices"""
        return self.envs[0].level_bank(seeds_or_capacity, full=full)

    def set_edits(self, edits, env_mask=None, env_ids=None):
        """`MultiGridEnv.set_edits` for the whole batch (envs built with `level_edits=K`): the lists, `env_mask` and `env_ids`
        in GLOBAL env order, split by `ranges` (`split_edits`); every shard's part is written on its own stream"""
        parts = split_edits(self.ranges, edits, env_mask=env_mask, env_ids=env_ids)
        self._each(lambda k, env: None if parts[k] is None else env.set_edits(**parts[k]))

    @property
    def edits_t(self):
        """per shard: its env's `edits_t`"""
        return [env.edits_t for env in self.envs]

    def edit_key(self, obj):
        """`MultiGridEnv.edit_key` in every shard (the shards register kinds in one order: one id)"""
        return self._each(lambda k, env: env.edit_key(obj))[0]

    def set_levels(self, bank=None, ids=None, seeds=None, env_mask=None, env_ids=None):
        """`MultiGridEnv.set_levels` for the whole batch: `ids` / `seeds`, `env_mask` and `env_ids` in GLOBAL env order, split by
        `ranges` (`split_levels`).  With a bank, every shard reads a replica of it on its own device — one per distinct device,
        seeded there from `bank.seeds` — that `bank.assign` keeps up to date."""
        if (bank is None) == (seeds is None) or (bank is not None and ids is None) or (seeds is not None and ids is not None):
            raise ValueError("set_levels: either (bank, ids) or seeds=")
        parts = split_levels(self.ranges, ids=ids, seeds=seeds, env_mask=env_mask, env_ids=env_ids)
        reps = [None] * len(self.envs)
        if bank is not None and not self.envs[0]._dry:
            for k, env in enumerate(self.envs):
                reps[k] = bank.replica(env.device, [s for s, e in zip(self.streams, self.envs) if e.device == env.device])

        def one(k, env):
            env._levels.enable()        # (every shard, selected or not: a checkpoint has the level keys in every shard or in none)
            if parts[k] is not None:
                env.set_levels(bank=reps[k] if bank is not None and reps[k] is not None else bank, **parts[k])
        self._each(one)

    @property
    def episode_level(self):
        """per shard: its env's `episode_level`"""
        return [env.episode_level for env in self.envs]

    def goal_distance(self, env_mask=None, env_ids=None, field=False):
        """`MultiGridEnv.goal_distance` for the whole batch: `env_mask` / `env_ids` in GLOBAL env order, split by `ranges`; every
        shard launches on its own stream.  Per shard: its env's (rows, n) tensor, or with `field=True` its (dist, field) pair
        (a shard none of `env_ids` falls into selects nothing and returns its tensors as they are)."""
        import numpy as np
        parts = split_params(self.ranges, env_mask=env_mask, env_ids=env_ids, _who="goal_distance")
        none = {"env_ids": np.zeros(0, np.int64)}
        return self._each(lambda k, env: env.goal_distance(field=field, **(none if parts[k] is None else parts[k])))

    def solve_distance(self, env_mask=None, env_ids=None, max_doors=2, max_items=2, policy=False):
        """`MultiGridEnv.solve_distance` for the whole batch: `env_mask` / `env_ids` in GLOBAL env order, split by `ranges`; every
        shard launches on its own stream.  Per shard: its env's (rows, n) tensor, or with `policy=True` its (dist, action) pair
        (a shard none of `env_ids` falls into selects nothing and returns its tensors as they are)."""
        import numpy as np
        parts = split_params(self.ranges, env_mask=env_mask, env_ids=env_ids, _who="solve_distance")
        none = {"env_ids": np.zeros(0, np.int64)}
        return self._each(lambda k, env: env.solve_distance(max_doors=max_doors, max_items=max_items, policy=policy,
                                                            **(none if parts[k] is None else parts[k])))

    def lookahead(self, actions, env_ids=None):
        """`MultiGridEnv.lookahead` for the whole batch: `actions` (K, T, m, n) or (T, m, n) and `env_ids` in GLOBAL env order,
        split by `ranges` — the env axis of `actions` with them —; every shard launches on its own stream.  Per shard: its env's
        (rewards, done) pair for the envs of the selection that are its own, in the selection's order (a shard none of
        `env_ids` falls into returns empty tensors)."""
        import numpy as np
        import torch
        if not torch.is_tensor(actions):
            actions = torch.as_tensor(np.asarray(actions))
        if actions.dim() == 3:
            actions = actions.unsqueeze(0)
        B = self.ranges[-1][1]
        ids = None if env_ids is None else _host_ids(env_ids, B, "lookahead")
        if actions.dim() != 4 or actions.shape[2] != (B if ids is None else len(ids)):
            raise ValueError("lookahead: actions must have shape (K, T, %d, n), got %s"
                             % (B if ids is None else len(ids), tuple(actions.shape)))

        def one(k, env):
            lo, hi = self.ranges[k]
            if ids is None:
                return env.lookahead(actions[:, :, lo:hi])
            sel = np.nonzero((ids >= lo) & (ids < hi))[0]
            return env.lookahead(actions[:, :, sel.tolist()], env_ids=ids[sel] - lo)
        return self._each(one)

    @property
    def lookahead_errors(self):
        """per shard: its env's `lookahead_errors`"""
        return [env.lookahead_errors for env in self.envs]

    def fork(self, src_ids, dst_ids):
        """`MultiGridEnv.fork` with ids in GLOBAL env order (read on the host).  A copy stays within one shard: a pair of ids that
        crosses shards raises NotImplementedError, before anything is copied."""
        import numpy as np
        B = self.ranges[-1][1]
        src, dst = _host_ids(src_ids, B, "fork(src_ids=)"), _host_ids(dst_ids, B, "fork(dst_ids=)")
        if src.size != dst.size:
            raise ValueError("fork: %d src_ids for %d dst_ids" % (src.size, dst.size))
        if len(set(dst.tolist())) != dst.size:
            raise ValueError("fork: a dst env is named twice (%s)" % dst.tolist())
        los = np.asarray([lo for lo, _ in self.ranges])
        ks, kd = np.searchsorted(los, src, side="right") - 1, np.searchsorted(los, dst, side="right") - 1
        if (ks != kd).any():
            i = int(np.nonzero(ks != kd)[0][0])
            raise NotImplementedError("fork: env %d is on shard %d and env %d on shard %d; a copy stays within one shard"
                                      % (src[i], ks[i], dst[i], kd[i]))
        self._each(lambda k, env: env.fork(src[ks == k] - los[k], dst[kd == k] - los[k]) if (ks == k).any() else None)

    # explore=True: per shard, its env's exploration tensors (None without the option)
    seen = property(lambda self: [env.seen for env in self.envs])
    visits = property(lambda self: [env.visits for env in self.envs])
    new_cells = property(lambda self: [env.new_cells for env in self.envs])
    visit_count = property(lambda self: [env.visit_count for env in self.envs])
    # memory=True: the two memory tensors likewise
    memory = property(lambda self: [env.memory for env in self.envs])
    seen_step = property(lambda self: [env.seen_step for env in self.envs])

    @property
    def solve_exact(self):
        """per shard: its env's `solve_exact`"""
        return [env.solve_exact for env in self.envs]

    @property
    def params(self):
        """per shard: its env's `params` (name -> the shard's (rows,) uint8 column)"""
        return [env.params for env in self.envs]

    def load_state_dict(self, sd):
        """a checkpoint of the whole batch (from one env, a pipeline or device shards, however it was split), rows
        `ranges[k]` into shard k (`split_state_dict`)"""
        parts = split_state_dict(sd, self.ranges)
        self._each(lambda k, env: env.load_state_dict(parts[k]))


class ShardPipeline(_Shards):
    """The batch of ONE GPU as `parts` independent envs, each stepped on its own stream.

    Why: a launch of the step kernel has a store-free head (staging, the env step, the first views: ~27 us during
    which HBM idles) and a ragged tail (waves exit between 80 and 165 us of a 165 us launch).  Two launches that do
    not depend on each other overlap there — the later one's workgroups start on the CUs the earlier one's leave —
    and the envs of a batch ARE independent (base.py:371-374: one RNG per env, nothing shared).  Measured on MI355X
    (profiles/r03/two_halves*.txt): 2 x 16 384 envs on two streams step 6-8 % faster than one env of 32 768,
    2 x 32 768 17 % faster than one of 65 536 (0.289 against 0.347 ms per step: 682 M agent-steps/s on one GPU); the
    same parts on ONE stream are 13 % slower than the one env, and parts that are joined after every step gain
    nothing — the overlap is between step i of one part and step i + 1 of the other, so it is there for callers that
    drive the parts independently (the usual double-buffered sampler: the policy looks at part A's observations
    while part B steps), not for a caller that needs all observations of a step before it issues the next.

    Env g of the global batch keeps its seed (seed + g, marlgrid_amd.sharding.shard_seeds), so trajectories are
    bit-identical to those of the one big env.  Everything a part returns is ordered on ITS stream
    (`pipe.streams[k]`): consume it there, or `pipe.streams[k].synchronize()` / `pipe.synchronize()` first.
    """

    def __init__(self, make_env, batch_size, parts=2, seed=1337, device=None, streams=None):
        """make_env(batch_size=..., seeds=..., device=...) -> MultiGridEnv.  `streams`: one per part (default: new
        ones.  HIP multiplexes streams onto a few hardware queues — GPU_MAX_HW_QUEUES, 4 by default —, and two streams
        that share a queue do not overlap: a process that builds several pipelines should hand the same streams to
        all of them)."""
        import torch
        if parts < 1 or batch_size % parts:
            raise ValueError("batch_size must be a multiple of parts")
        self.device = torch.device(device if device is not None else "cuda")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.batch_size, self.parts = int(batch_size), int(parts)
        self.part_size = self.batch_size // self.parts
        self.ranges = [(k * self.part_size, (k + 1) * self.part_size) for k in range(self.parts)]
        self.streams = list(streams) if streams is not None else [torch.cuda.Stream(device=self.device) for _ in range(self.parts)]
        if len(self.streams) != self.parts:
            raise ValueError("one stream per part")
        # Part k is BUILT on the stream it will be stepped on: a constructor ends with launches nobody waits for (the
        # first observation; the seeding and reset of a non-strict env), and torch's side streams do not wait for the
        # stream that happened to be current — on its own stream the part's first reset() / step_part() simply queues
        # behind them.
        self.envs = []
        for k in range(self.parts):
            with torch.cuda.stream(self.streams[k]):
                self.envs.append(make_env(batch_size=self.part_size, seeds=shard_seeds(seed, self.batch_size, k, self.parts),
                                          device=self.device))

    def on(self, k):
        """`with pipe.on(k): ...` — part k's stream as torch's current stream: the policy's kernels for part k and
        everything else that consumes its observations belong here, so that they queue behind part k's step and
        overlap the OTHER part's (the double-buffered sampler:

            obs = pipe.reset()
            while ...:
                for k in range(pipe.parts):
                    with pipe.on(k):
                        act = agents.action_step(obs[k])
                        nxt, rew, done, _ = pipe.step_part(k, act)
                        agents.save_step(obs[k], act, nxt, rew, done)
                        obs[k] = nxt
        )"""
        import torch
        return torch.cuda.stream(self.streams[k])

    def reset_part(self, k, **kw):
        with self.on(k):
            return self.envs[k].reset(**kw)

    def part(self, k, tensor):
        """rows of part k in a (batch_size, ...) tensor"""
        return tensor[k * self.part_size:(k + 1) * self.part_size]

    def reset(self):
        """per part: its observations (ordered on streams[k])"""
        return self._each(lambda k, env: env.reset())

    def step(self, actions):
        """actions: (batch_size, n_agents), resident and ready (the parts' streams do not wait for the stream that
        produced it), or a list with one tensor per part.  Returns per part (obs, rewards, done, info) — info: the part's
        episode_info dict, or {} —, each ordered on
        streams[k]."""
        per_part = isinstance(actions, (list, tuple))
        return self._each(lambda k, env: env.step(actions[k] if per_part else self.part(k, actions)))

    def step_part(self, k, actions):
        """one part alone (the double-buffered sampler's call)"""
        import torch
        with torch.cuda.stream(self.streams[k]):
            return self.envs[k].step(actions)


class DeviceShards(_Shards):
    """ONE process steps an env batch sharded over a list of GPUs: shard k is a MultiGridEnv of the global envs
    `ranges[k]` (`shard_range(batch_size, k, N)`: contiguous, sizes differ by at most one) on `devices[k]`, stepped on
    `streams[k]`.  Envs are independent and env g is seeded `seed + g` whatever the sharding, so the shards step exactly
    the trajectories of the one big env (and of `bench.py --gpus N`'s one process per GPU).

    `devices`: a non-empty sequence of torch.device / str / int; entries MAY REPEAT — two shards per GPU (each then plans
    its observation placement for its part of the device's memory: `place_obs` gets `share=m`, `merge_share`), or the way a
    one-GPU machine runs this class at all.

    Ordering contract.  `step()` / `reset()` issue the N shards' launches from the calling thread, one after the other,
    without a host synchronisation, and return a list with one entry per shard: what that shard's env returned, device
    tensors of devices[k] ORDERED ON streams[k].  Consume an entry under `with shards.on(k):` (device k current, stream k
    current — a policy's kernels for shard k then queue behind its step and run beside the other shards'), or pass the
    list to `gather()`, whose result is ordered on the caller's current stream, or `synchronize()` first.  Actions given as
    ONE device tensor need no readiness from the caller (unlike ShardPipeline.step): see `step`.

    Per-env errors (the reference's exceptions) are re-raised with the type the shard's env raises, and a message that
    names the shard and its global env range."""

    def __init__(self, make_env, batch_size, devices, seed=1337, streams=None):
        """make_env(batch_size=..., seeds=..., device=...) -> MultiGridEnv; for a shard whose device appears m > 1 times in
        `devices` it is called with `share=m` as well (what `make(devices=)` and `MultiGridEnv.sharded` merge into
        `place_obs`).  `streams`: one per shard, on its device (default: new ones; HIP multiplexes the streams of a device
        onto a few hardware queues — GPU_MAX_HW_QUEUES, 4 by default —: a process that builds several of these on the same
        devices should hand the same streams to all of them)."""
        import torch
        devices = list(devices) if devices is not None else []
        if not devices:
            raise ValueError("DeviceShards: `devices` must name at least one device")
        self.batch_size = int(batch_size)
        self.ranges = shard_ranges(self.batch_size, len(devices))
        self.devices = [self._device(d) for d in devices]
        for d in self.devices:
            if d.type != "cuda":
                raise ValueError("DeviceShards: HIP devices only (got %r)" % (d,))
        if streams is not None and len(streams) != len(self.devices):
            raise ValueError("one stream per shard")
        self.streams = list(streams) if streams is not None else [torch.cuda.Stream(device=d) for d in self.devices]
        for k, s in enumerate(self.streams):
            if s.device != self.devices[k]:
                raise ValueError("streams[%d] is a stream of %s, shard %d lives on %s" % (k, s.device, k, self.devices[k]))
        n = len(self.devices)
        # Shard k is BUILT with its device current and on its own stream (ShardPipeline.__init__ says why: a constructor ends
        # with launches nobody waits for; the shard's first reset() / step queues behind them there).
        self.envs = []
        for k, d in enumerate(self.devices):
            share = sum(1 for o in self.devices if o == d)
            extra = {"share": share} if share > 1 else {}
            with self.on(k):
                self.envs.append(self._call(k, lambda: make_env(batch_size=self.ranges[k][1] - self.ranges[k][0],
                                                                seeds=shard_seeds(seed, self.batch_size, k, n), device=d, **extra)))

    @staticmethod
    def _device(d):
        import torch
        if isinstance(d, int):
            return torch.device("cuda", d)
        d = torch.device(d)
        if d.type == "cuda" and d.index is None:
            d = torch.device("cuda", torch.cuda.current_device())
        return d

    # ---- shard k's context ------------------------------------------------------------------------------------------
    @contextlib.contextmanager
    def on(self, k):
        """`with shards.on(k): ...` — shard k's DEVICE as the current device and its STREAM as torch's current stream: where
        shard k's results are consumed and its actions are made (examples/sharded_rollout.py; the double-buffered loop of
        ShardPipeline.on works here unchanged, with `step_shard`)."""
        import torch
        with torch.cuda.device(self.devices[k]), torch.cuda.stream(self.streams[k]):
            yield self

    def _where(self, k):
        return "shard %d on %s (global envs [%d, %d); an env number in the message counts from %d)" % (
            (k, self.devices[k]) + self.ranges[k] + (self.ranges[k][0],))

    def _call(self, k, fn):
        """fn() for shard k; a per-env error of the engine — the exception types of _native.ERR_EXC — is re-raised as the same
        type with the shard and its global range in front"""
        from ._native import ERR_EXC
        try:
            return fn()
        except tuple(set(ERR_EXC.values())) as e:
            try:
                named = type(e)("%s: %s" % (self._where(k), e))
            except Exception:       # (a subclass with another constructor: as it is)
                raise e
            raise named from e

    def _each(self, fn):
        out = []
        for k, env in enumerate(self.envs):
            with self.on(k):
                out.append(self._call(k, lambda: fn(k, env)))
        return out

    def shard(self, k, tensor):
        """rows of shard k in a (batch_size, ...) tensor"""
        lo, hi = self.ranges[k]
        return tensor[lo:hi]

    # ---- the gym surface ----------------------------------------------------------------------------------------------
    def reset(self):
        """per shard: its observations (ordered on streams[k])"""
        return self._each(lambda k, env: env.reset())

    def reset_shard(self, k, **kw):
        with self.on(k):
            return self._call(k, lambda: self.envs[k].reset(**kw))

    def step_shard(self, k, actions):
        """one shard alone: `actions` (its rows only) as MultiGridEnv.step takes them — made under `on(k)`, or ready"""
        with self.on(k):
            return self._call(k, lambda: self.envs[k].step(actions))

    def step(self, actions):
        """All N shards' step launches, issued from this thread with no host synchronisation.  Returns per shard
        (obs, rewards, done, info), each ordered on streams[k].  `actions`:

          * a list / tuple with one entry per shard (its rows, as MultiGridEnv.step takes them: resident on devices[k] and
            ordered on streams[k] — made under `on(k)` —, or host arrays);
          * a (batch_size, n_agents) array on the host (numpy or a CPU tensor): each shard uploads its rows;
          * a (batch_size, n_agents) tensor on ANY HIP device, and the caller does NOT have to synchronise: one event is
            recorded on the producer device's current stream — whatever was queued there before this call, the kernel
            that writes the actions included, is what the shards wait for —, every shard's stream waits for that event, and
            each shard's rows are then copied to its device on its own stream (non_blocking; no copy where the shard lives on
            the producer's device).  (ShardPipeline.step asks the caller for readiness instead.)"""
        import torch
        if isinstance(actions, (list, tuple)):
            if len(actions) != len(self.envs):
                raise ValueError("a list of actions has one entry per shard (a host array of the whole batch: numpy or a tensor)")
            return self._each(lambda k, env: env.step(actions[k]))
        if not torch.is_tensor(actions):
            import numpy as np
            actions = torch.as_tensor(np.asarray(actions))
        if actions.dim() != 2 or actions.shape[0] != self.batch_size:
            raise AssertionError("actions must have shape (batch_size, n_agents), or be a list with one entry per shard")
        if actions.device.type != "cuda":
            return self._each(lambda k, env: env.step(self.shard(k, actions)))
        ready = torch.cuda.Event()
        ready.record(torch.cuda.current_stream(actions.device))

        def one(k, env):
            s = self.streams[k]
            s.wait_event(ready)
            rows = self.shard(k, actions)
            rows.record_stream(s)             # (the producer may free `actions` while shard k's copy / launch is still queued)
            return env.step(rows.to(self.devices[k], non_blocking=True))
        return self._each(one)

    # ---- joining the shards -------------------------------------------------------------------------------------------
    def gather(self, per_shard, device=None):
        """What the shards returned -> the same for the whole batch, in global env order, on ONE device (default: shard 0's).
        `per_shard`: a list with one entry per shard — tensors whose dim 0 is the shard's envs, dicts of them (the
        episode_info dicts; {} stays {}), or tuples / lists of those (so `obs, rew, done, info = shards.gather(shards.step(a))`
        works).  Every piece's copy is ordered behind its shard's stream: the target device's current stream waits for one
        event per shard, the copies are queued there (non_blocking), and the shards' streams then wait for the copies before
        they overwrite what was read — the result is ordered on the caller's current stream of `device`, no host
        synchronisation.  device="cpu": the copies are synchronous."""
        import torch
        if len(per_shard) != len(self.envs):
            raise ValueError("gather: one entry per shard")
        dst = self.devices[0] if device is None else torch.device(device) if not isinstance(device, int) else torch.device("cuda", device)
        if dst.type == "cuda" and dst.index is None:
            dst = torch.device("cuda", torch.cuda.current_device())
        if dst.type != "cuda":
            self.synchronize()
            return self._join(list(per_shard), dst)
        with torch.cuda.device(dst):
            target = torch.cuda.current_stream(dst)
            for s in self.streams:
                if s != target:
                    target.wait_event(s.record_event())
            out = self._join(list(per_shard), dst)
            done = target.record_event()
            for s in self.streams:
                if s != target:
                    s.wait_event(done)
        return out

    def _join(self, pieces, dst):
        import torch
        first = pieces[0]
        if torch.is_tensor(first):
            out = torch.empty((self.batch_size,) + tuple(first.shape[1:]), dtype=first.dtype, device=dst)
            for (lo, hi), p in zip(self.ranges, pieces):
                if p.shape[0] != hi - lo:
                    raise ValueError("gather: a piece with %d rows for a shard of %d envs" % (p.shape[0], hi - lo))
                out[lo:hi].copy_(p, non_blocking=dst.type == "cuda")      # (into pageable host memory: a blocking copy)
            return out
        if isinstance(first, dict):
            return {key: self._join([p[key] for p in pieces], dst) for key in first}
        if isinstance(first, (list, tuple)):
            return type(first)(self._join([p[i] for p in pieces], dst) for i in range(len(first)))
        raise TypeError("gather: tensors, dicts of tensors, or tuples / lists of them (got %r)" % type(first).__name__)

    # ---- the rest ---------------------------------------------------------------------------------------------------------
    def check_errors(self):
        """every shard's check_errors() under its own device and stream (host sync: an env waits for every stream it
        launched on).  The first shard with an env in error raises that env's exception — the type MultiGridEnv raises —
        with the shard and its global env range in the message."""
        self._each(lambda k, env: env.check_errors())

    @property
    def kernel_names(self):
        """per shard: the instantiation of the observation kernel its step launches (shards of different sizes may take
        different ones: the launcher picks workgroups by the batch)"""
        return [env.kernel_name for env in self.envs]

    @property
    def obs_placement(self):
        """per shard: its env's `obs_placement` (one record per view group; None where the buffer is a plain allocation)"""
        return [env.obs_placement for env in self.envs]
