"""Host only (`_dry`): the contract of `MultiGridEnv(level_edits=K)` — what the recorder appends, what `set_edits` takes and
refuses (`state_dict()` carries tensors: its round trip is tests/test_hip_level_edits.py's).  What the op DOES is tests/test_gen_edits_diff_host.py's."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "native"))

import test_gen_recording_pinned as PIN  # noqa: E402
from marlgrid_amd import _native as N  # noqa: E402
from marlgrid_amd import envs as E  # noqa: E402
from marlgrid_amd.gen_recorder import RecordedOp, pack_program  # noqa: E402
from marlgrid_amd.objects import Goal, Key, Wall  # noqa: E402

CLUTTERED = "MarlGrid-3AgentCluttered15x15-v0"
DOORKEY = "MarlGrid-2AgentColoredDoorKey8x8-v0"


def _ids_of(cls):
    return [n for n in sorted(E._registry) if isinstance(E.make(n, batch_size=1, _dry=True), cls)]


def _ops(env):
    env._ensure_recorded()
    return env._dry_trace[1]


def test_k0_leaves_every_registered_recording_as_pinned():
    with open(PIN.TABLE) as f:
        want = json.load(f)
    names = sorted(E.registered_envs + E.extension_envs)
    assert len(names) >= 11
    for name in names:
        env = E.make(name, batch_size=2, level_edits=0, _dry=True)
        assert env.level_edits == 0 and env.edits_t is None
        assert PIN.record(env) == want["registry:" + name], name


@pytest.mark.parametrize("cls", ["ClutteredMultiGrid", "ColoredDoorKeyEnv", "EmptyMultiGrid"])
def test_k_appends_exactly_one_op_last(cls):
    """also for a scenario that forks (ColoredDoorKeyEnv: guarded branches) and for one without a placement (EmptyMultiGrid)"""
    name = _ids_of(getattr(E, cls))[0]
    plain_env = E.make(name, batch_size=2, _dry=True)
    plain = _ops(plain_env)
    env = E.make(name, batch_size=2, level_edits=5, _dry=True)
    ops = _ops(env)
    assert [tuple(op) for op in ops[:-1]] == [tuple(op) for op in plain]
    last = ops[-1]
    assert last == RecordedOp.edits(5) and last.is_edits and last.guard is None and last.count == 5
    assert last.max_tries == N.GEN_EDITS == -3
    assert sum(1 for op in ops if op.is_edits) == 1
    assert not (last.is_draw or last.is_param or last.sets_register or last.is_fill or last.is_placement)
    if cls == "ColoredDoorKeyEnv":
        assert any(op.guard is not None for op in plain)
    if cls == "EmptyMultiGrid":
        assert plain == []
    packed, _ = pack_program(ops, env.width, env.height, env.cells_stride, len(env.obj_reg.objs))
    assert (packed[len(ops) - 1].max_tries, packed[len(ops) - 1].count, packed[len(ops) - 1].obj) == (-3, 5, 0)
    # the spec the oracle reads is the plain scenario's: an edit list is no part of `_gen_grid`
    assert env.scenario_spec()["gen_reset"] == plain_env.scenario_spec()["gen_reset"]
    assert env.edits_t.shape == (2, 5, 4) and env.edits_t.dtype == np.uint8 and not env.edits_t.any()


def test_level_edits_range_and_kwarg_paths():
    for bad in (-1, 65, 2.5, True, "4"):
        with pytest.raises(ValueError, match="level_edits"):
            E.make(CLUTTERED, batch_size=2, level_edits=bad, _dry=True)
    assert E.make(CLUTTERED, batch_size=2, level_edits=64, _dry=True).edits_t.shape == (2, 64, 4)
    with pytest.raises(ValueError, match="level_edits"):
        E.make(CLUTTERED, batch_size=2, _dry=True).set_edits([(1, 1, 1, 1)])


def test_set_edits_shapes_and_selection():
    B, K = 6, 4
    env = E.make(CLUTTERED, batch_size=B, level_edits=K, _dry=True)
    wall, goal = env.edit_key(Wall()), env.edit_key(Goal(color="green", reward=1))
    assert (env.edit_key(None), wall, goal) == (0, 1, 2)
    env.set_edits([(3, 4, wall, 1), (5, 6, goal, 7)])                    # (K', 4) for every env; `on` is stored as 0 / 1
    assert (env.edits_t[:, 0] == (3, 4, wall, 1)).all() and (env.edits_t[:, 1] == (5, 6, goal, 1)).all()
    assert not env.edits_t[:, 2:].any()                                  # the slots from K' on are off
    env.set_edits([(1, 1, 0, 1)], env_mask=np.arange(B) % 2 == 0)
    assert (env.edits_t[0::2, 0] == (1, 1, 0, 1)).all() and not env.edits_t[0::2, 1:].any()
    assert (env.edits_t[1::2, 1] == (5, 6, goal, 1)).all()
    per = np.zeros((2, 3, 4), np.int64)
    per[0, 0], per[1, 2] = (2, 2, wall, 1), (9, 9, wall, 1)
    env.set_edits(per, env_ids=[5, 1])                                   # (k, K', 4) with env_ids
    assert (env.edits_t[5, 0] == (2, 2, wall, 1)).all() and (env.edits_t[1, 2] == (9, 9, wall, 1)).all()
    assert not env.edits_t[5, 1:].any() and not env.edits_t[1, :2].any()
    whole = np.zeros((B, K, 4), np.uint8)
    whole[:, 0] = [(b + 1, 1, wall, 1) for b in range(B)]
    env.set_edits(whole)                                                 # (B, K, 4)
    assert np.array_equal(env.edits_t, whole)
    env.set_edits(whole[::-1].copy(), env_ids=[0])                       # a (B, ...) value with env_ids is gathered by them
    assert (env.edits_t[0, 0] == (B, 1, wall, 1)).all()
    env.set_edits([])
    assert not env.edits_t.any()
    key = env.edit_key(Key("blue"))                                      # a kind seen for the first time is registered
    assert key == 3 and len(env.obj_reg.objs) == 4
    env.set_edits([(2, 2, key, 1)])


def test_set_edits_refuses_bad_host_values():
    env = E.make(CLUTTERED, batch_size=4, level_edits=2, _dry=True)
    W, H, n = env.width, env.height, len(env.obj_reg.objs)
    for bad, what in (([(W, 1, 1, 1)], "x"), ([(1, H, 1, 1)], "y"), ([(1, 1, n, 1)], "kind"), ([(-1, 1, 1, 1)], "non-negative"),
                      ([(1, 1, 1, 1)] * 3, "level_edits=2"), ([(1, 1, 1)], "entries"), (np.zeros((3, 1, 4), np.int64), "per selected"),
                      ([(1.5, 1, 1, 1)], "integer")):
        before = env.edits_t.copy()
        with pytest.raises(ValueError, match=what):
            env.set_edits(bad)
        assert np.array_equal(env.edits_t, before)
    with pytest.raises(ValueError):
        env.set_edits([(1, 1, 1, 1)], env_mask=np.ones(4, bool), env_ids=[0])
    with pytest.raises(ValueError):
        env.set_edits([(1, 1, 1, 1)], env_ids=[4])


def test_split_edits_is_the_global_order():
    from marlgrid_amd import sharding
    B, K = 7, 3
    ranges = [(0, 3), (3, 7)]
    whole = np.arange(B * K * 4).reshape(B, K, 4) % 3
    parts = sharding.split_edits(ranges, whole)
    assert np.array_equal(parts[0]["edits"], whole[:3]) and np.array_equal(parts[1]["edits"], whole[3:])
    one = [(1, 2, 1, 1)]
    parts = sharding.split_edits(ranges, one, env_mask=np.arange(B) < 4)
    assert parts[0]["env_mask"].tolist() == [True] * 3 and parts[1]["env_mask"].tolist() == [True, False, False, False]
    assert np.array_equal(parts[0]["edits"], one) and np.array_equal(parts[1]["edits"], one)
    ids = np.array([6, 0, 4])
    parts = sharding.split_edits(ranges, whole[ids], env_ids=ids)
    assert parts[0]["env_ids"].tolist() == [0] and np.array_equal(parts[0]["edits"], whole[[0]])
    assert parts[1]["env_ids"].tolist() == [3, 1] and np.array_equal(parts[1]["edits"], whole[[6, 4]])
    assert sharding.split_edits(ranges, one, env_ids=[5])[0] is None
    with pytest.raises(ValueError):
        sharding.split_edits(ranges, whole[:2])
    # applied shard by shard, the parts are the one env's table
    one_env = E.make(CLUTTERED, batch_size=B, level_edits=K, _dry=True)
    one_env.set_edits(whole[ids], env_ids=ids)
    shards = [E.make(CLUTTERED, batch_size=hi - lo, level_edits=K, _dry=True) for lo, hi in ranges]
    for env, kw in zip(shards, parts):
        env.set_edits(**kw)
    assert np.array_equal(np.concatenate([e.edits_t for e in shards]), one_env.edits_t)
