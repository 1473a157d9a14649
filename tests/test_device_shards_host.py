"""Host side of DeviceShards (marlgrid_amd/sharding.py), no GPU: which envs and seeds a shard gets, the argument errors
(raised before a device is touched), the checkpoint merge / split as pure functions on fabricated tensors, and the rule
that merges `share` into `place_obs`."""
import pytest
import torch

from marlgrid_amd import sharding as S
from marlgrid_amd.base import STATE_DICT_VERSION, MultiGridEnv
from marlgrid_amd.envs import make

NAME = "MarlGrid-3AgentCluttered15x15-v0"


@pytest.mark.parametrize("B,N,sizes", [(10, 3, [4, 3, 3]), (4099, 8, [513] * 3 + [512] * 5), (8, 8, [1] * 8), (7, 1, [7])])
def test_ranges_and_seeds(B, N, sizes):
    ranges = S.shard_ranges(B, N)
    assert [hi - lo for lo, hi in ranges] == sizes
    assert ranges[0][0] == 0 and ranges[-1][1] == B
    assert all(ranges[k][1] == ranges[k + 1][0] for k in range(N - 1))          # union [0, B), no overlap, in order
    assert ranges == [S.shard_range(B, k, N) for k in range(N)]
    seen = []
    for k, (lo, hi) in enumerate(ranges):
        seeds = S.shard_seeds(1337, B, k, N)
        assert seeds == [1337 + g for g in range(lo, hi)]                        # seed + global id
        seen += seeds
    assert seen == [1337 + g for g in range(B)]


def test_argument_errors_before_any_device_is_touched():
    never = lambda **kw: pytest.fail("make_env must not be called")
    with pytest.raises(ValueError):
        S.DeviceShards(never, 8, [])
    with pytest.raises(ValueError):
        S.DeviceShards(never, 8, None)
    with pytest.raises(ValueError):
        S.DeviceShards(never, 2, ["cuda:0"] * 3)
    with pytest.raises(ValueError):
        S.shard_ranges(2, 3)
    with pytest.raises(ValueError):
        make(NAME, batch_size=8, devices=[])
    with pytest.raises(ValueError):
        make(NAME, batch_size=2, devices=["cuda:0"] * 3)
    with pytest.raises(ValueError):
        make(NAME, batch_size=8, devices=["cuda:0"] * 2, pipeline=2)
    with pytest.raises(ValueError):
        make(NAME, batch_size=8, devices=["cuda:0"] * 2, seeds=list(range(8)))
    with pytest.raises(ValueError):
        make(NAME, batch_size=8, devices=["cuda:0"] * 2, device="cuda:0")
    with pytest.raises(ValueError):
        MultiGridEnv.sharded([], ["cuda:0"] * 2, batch_size=8, seeds=list(range(8)))
    with pytest.raises(ValueError):
        MultiGridEnv.sharded([], [], batch_size=8)
    with pytest.raises(KeyError):
        make("no-such-env", batch_size=8, devices=["cuda:0"])


def _fake_state(B, n=3, prestige=False, ep=False, version=STATE_DICT_VERSION, seed=0):
    """tensors with MultiGridEnv.state_dict()'s keys, dtypes and per-env shapes (base.py: _STATE_KEYS), random content"""
    g = torch.Generator().manual_seed(seed)
    r = lambda shape, dtype, hi=2 ** 31 - 1: torch.randint(0, hi, shape, generator=g, dtype=torch.int64).to(dtype)
    sd = {"grid_state": r((B, 240), torch.uint8, 255), "agent_state": r((B, n), torch.int64), "mt_state": r((B, 624), torch.int32),
          "mt_pos": r((B,), torch.int32, 624), "mt_head": r((B, 16), torch.int32), "step_count_t": r((B,), torch.int32, 100),
          "done_t": r((B,), torch.uint8, 2), "error_t": r((B,), torch.int32, 2)}
    if prestige:
        sd["prestige_t"] = torch.rand((B, n), generator=g, dtype=torch.float64)
    if ep:
        sd["ep_return_t"] = torch.rand((B, n), generator=g, dtype=torch.float64)
    sd["version"] = torch.tensor(version)
    return sd


def _same(a, b):
    assert set(a) == set(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("prestige,ep", [(False, False), (True, False), (False, True), (True, True)])
def test_merge_split_round_trip_and_resharding(prestige, ep):
    B = 4099
    sd = _fake_state(B, prestige=prestige, ep=ep)
    r8, r2, r3 = S.shard_ranges(B, 8), S.shard_ranges(B, 2), S.shard_ranges(10, 3)
    parts8 = S.split_state_dict(sd, r8)
    assert [p["grid_state"].shape[0] for p in parts8] == [513] * 3 + [512] * 5                   # uneven ranges
    for p, (lo, hi) in zip(parts8, r8):
        assert set(p) == set(sd) and int(p["version"]) == STATE_DICT_VERSION
        assert all(torch.equal(p[k], sd[k][lo:hi]) for k in sd if k != "version")
    merged = S.merge_state_dicts(parts8)
    _same(merged, sd)                                                                            # split, merge: the identity
    _same(S.merge_state_dicts(S.split_state_dict(merged, r2)), sd)                                # an 8-way split loads 2-way
    _same(S.merge_state_dicts([sd]), sd)
    # merge, split: the identity as well (three separately made shards of 4, 3, 3 envs)
    shards = [_fake_state(hi - lo, prestige=prestige, ep=ep, seed=7 + k) for k, (lo, hi) in enumerate(r3)]
    for p, q in zip(S.split_state_dict(S.merge_state_dicts(shards), r3), shards):
        _same(p, q)


def test_merge_split_refuse_what_does_not_fit():
    a, b = _fake_state(4, seed=1), _fake_state(3, seed=2)
    with pytest.raises(KeyError):                 # optional keys: in every shard or in none
        S.merge_state_dicts([_fake_state(4, ep=True), b])
    with pytest.raises(KeyError):
        S.merge_state_dicts([a, _fake_state(3, prestige=True)])
    with pytest.raises(KeyError):
        S.merge_state_dicts([{k: v for k, v in a.items() if k != "version"}, {k: v for k, v in b.items() if k != "version"}])
    with pytest.raises(ValueError):               # version: the same everywhere, and this engine's
        S.merge_state_dicts([a, _fake_state(3, version=STATE_DICT_VERSION - 1)])
    with pytest.raises(ValueError):
        S.merge_state_dicts([_fake_state(4, version=STATE_DICT_VERSION + 1), _fake_state(3, version=STATE_DICT_VERSION + 1)])
    with pytest.raises(ValueError):
        S.merge_state_dicts([])
    with pytest.raises(ValueError):
        S.split_state_dict(_fake_state(7, version=STATE_DICT_VERSION - 1), S.shard_ranges(7, 2))
    with pytest.raises(KeyError):
        S.split_state_dict({k: v for k, v in a.items() if k != "version"}, S.shard_ranges(4, 2))
    with pytest.raises(ValueError):               # ranges that do not cover the batch / are not a partition in order
        S.split_state_dict(a, S.shard_ranges(5, 2))
    with pytest.raises(ValueError):
        S.split_state_dict(a, [(0, 2), (3, 4)])
    with pytest.raises(ValueError):
        S.split_state_dict(a, [(2, 4), (0, 2)])


def test_share_merges_into_every_form_of_place_obs():
    assert S.merge_share(True, 4) == {"share": 4}
    assert S.merge_share("search", 4) == {"share": 4}
    assert S.merge_share("thorough", 2) == {"thorough": True, "share": 2}
    assert S.merge_share({"seconds": 0.5}, 8) == {"seconds": 0.5, "share": 8}
    assert S.merge_share({"seconds": 0.5, "share": 3}, 8) == {"seconds": 0.5, "share": 3}        # its own share stays
    assert S.merge_share(False, 8) is False
    given = {"budget": 1 << 30}
    assert S.merge_share(given, 2) is not given and given == {"budget": 1 << 30}                 # the caller's dict is not edited
    for form in (True, "search", "thorough", False, given):                                      # one shard per device: untouched
        assert S.merge_share(form, 1) is form
    # "the equivalent dict": a host-only env configured with it ends up where the plain form leads
    from marlgrid_amd.agents import GridAgentInterface
    from marlgrid_amd.envs import EmptyMultiGrid
    for form in (True, "search", "thorough"):
        plain = EmptyMultiGrid(agents=[GridAgentInterface(view_tile_size=8)], grid_size=5, place_obs=form, _dry=True)
        shared = EmptyMultiGrid(agents=[GridAgentInterface(view_tile_size=8)], grid_size=5, place_obs=S.merge_share(form, 2), _dry=True)
        assert shared.place_obs == plain.place_obs and shared._place_kw.get("share") == 2
        assert bool(shared._place_kw.get("thorough")) == (form == "thorough")


def test_pipeline_keeps_its_ranges_and_gets_the_checkpoint_methods():
    assert S.ShardPipeline.state_dict is S.DeviceShards.state_dict and S.ShardPipeline.load_state_dict is S.DeviceShards.load_state_dict
    with pytest.raises(ValueError):               # (unchanged: an uneven pipeline is refused)
        S.ShardPipeline(lambda **kw: None, 7, parts=2)
