"""GPU (-m gpu): marlgrid_amd.sharding.DeviceShards through its public entry points — make(id, devices=[...]) and
MultiGridEnv.sharded(...) — in ONE process.  Repeated "cuda:0" entries are how a one-GPU machine runs the class: every shard
has its own env, stream, seeds and slice of the batch, exactly as on distinct devices; only the last test needs two GPUs.

What is proven: the shards step the trajectories of the one big env (all envs, every step, byte for byte — and against the
CPU oracle directly), every option reaches every shard, the three forms of `actions` and the per-shard loop agree, checkpoints
move between 8 shards, 2 shards, a pipeline and one env, and a per-env error surfaces with its type, its shard and its range.

Every DeviceShards / ShardPipeline of this file is built on the same 8 streams (`_streams`): with torch's default stream the
process opens 9."""
import numpy as np
import pytest

import canon
import product_envs
import scenarios
from marlgrid_amd import seeding
from oracle import oracle as O

pytestmark = pytest.mark.gpu

NAME = "MarlGrid-3AgentCluttered15x15-v0"
REW_TOL = 1e-6                      # the project's tolerance (tests/test_hip_parity.py)
INFO_KEYS = ("terminated", "truncated", "reset", "episode_return", "episode_length")
_STREAMS = {}


def _streams(k, device="cuda:0"):
    import torch
    if device not in _STREAMS:
        _STREAMS[device] = [torch.cuda.Stream(device=device) for _ in range(8)]
    return _STREAMS[device][:k]


def _devices(k):
    return ["cuda:0"] * k


def _sharded(B, k, name=NAME, **kw):
    from marlgrid_amd.envs import make
    return make(name, batch_size=B, devices=_devices(k), streams=_streams(k), **kw)


def _same_state(got, want):
    import torch
    assert set(got) == set(want), (sorted(got), sorted(want))
    for key in want:
        g, w = got[key].cpu(), want[key].cpu()
        assert g.dtype == w.dtype and g.shape == w.shape and torch.equal(g, w), key


def _invariance(B, devices, streams, steps):
    """make(devices=) against make(): obs, rewards and done of ALL envs identical on every step, the merged state at the end"""
    import torch
    from marlgrid_amd.envs import make
    from marlgrid_amd.sharding import DeviceShards, shard_ranges
    ds = make(NAME, batch_size=B, devices=devices, streams=streams, auto_reset=True)
    one = make(NAME, batch_size=B, auto_reset=True)
    assert isinstance(ds, DeviceShards) and ds.batch_size == B and len(ds.envs) == len(devices)
    assert ds.ranges == shard_ranges(B, len(devices)) and [e.batch_size for e in ds.envs] == [hi - lo for lo, hi in ds.ranges]
    assert [str(d) for d in ds.devices] == list(devices) and all(e.device == d for e, d in zip(ds.envs, ds.devices))
    for k, (lo, hi) in enumerate(ds.ranges):
        assert ds.envs[k].seeds == one.seeds[lo:hi]
    print("\nB=%d on %s: shard sizes %s, kernels %s (one env: %s)" % (B, devices, [e.batch_size for e in ds.envs],
                                                                    sorted(set(ds.kernel_names)), one.kernel_name))
    assert torch.equal(ds.gather(ds.reset()), one.reset())
    g = torch.Generator().manual_seed(B + len(devices))
    n_done = 0
    for t in range(steps):
        a = torch.randint(0, 7, (B, 3), generator=g).to("cuda:0", non_blocking=True)      # (no synchronise: step() orders it)
        o, r, d, info = ds.gather(ds.step(a))
        o2, r2, d2, _ = one.step(a)
        assert info == {}
        assert o.shape == o2.shape and o.dtype == o2.dtype and torch.equal(o, o2), "obs step %d" % t
        assert r.dtype == r2.dtype and torch.equal(r, r2), "rewards step %d" % t
        assert d.dtype == d2.dtype and torch.equal(d, d2), "done step %d" % t
        n_done += int(d2.sum())
    ds.check_errors(), one.check_errors()
    _same_state(ds.state_dict(), one.state_dict())
    assert all(v.device.type == "cpu" for v in ds.state_dict().values())
    ds.close()
    return n_done


# ---- 1. shard invariance through the public API ----------------------------------------------------------------------------
def test_uneven_shards_equal_the_one_env():
    """B = 4 099 on 8 shards (three of 513, five of 512 envs), 150 steps: across the time limit at step 100"""
    assert _invariance(4099, _devices(8), _streams(8), 150) >= 4099


@pytest.mark.parametrize("k", [8, 2])
def test_bench_batch_equals_the_one_env(k):
    """B = 32 768 on 8 and on 2 shards, 110 steps: across the mass reset at step 100.  (Both observation rings and the gathered
    copy fit beside each other — 5 x 925 MB —: every step is compared whole, nothing block-wise.)"""
    assert _invariance(32768, _devices(k), _streams(k), 110) >= 32768


# ---- 2. against the oracle directly ------------------------------------------------------------------------------------------
def test_shards_vs_oracle():
    """B = 1 027 on 3 shards, 300 steps, as tests/test_hip_parity.py::test_batch_vs_oracle compares one env: rewards to 1e-6,
    done every step, whole observations every 50th step (and the first), canonical state and RNG of every env at the end;
    finished episodes are reset per shard (reset_shard with the shard's rows of the mask)"""
    import torch
    B, k, T = 1027, 3, 300
    ds = _sharded(B, k, seed=5000)
    orc = O.OracleBatch(scenarios.registered(NAME), 5000 + np.arange(B))
    assert [hi - lo for lo, hi in ds.ranges] == [343, 342, 342]
    assert np.array_equal(ds.gather(ds.reset()).cpu().numpy(), orc.reset())
    rng = np.random.RandomState(11)
    episodes = 0
    for t in range(T):
        a = rng.randint(0, 7, size=(B, 3))
        o, r, dn, _ = ds.gather(ds.step(a))
        o2, r2, dn2, _ = orc.step(a, render=(t % 50 == 0 or t == T - 1))
        assert np.abs(r.cpu().numpy().astype(np.float64) - r2).max() <= REW_TOL, t
        assert np.array_equal(dn.cpu().numpy(), dn2), t
        if o2 is not None:
            assert np.array_equal(o.cpu().numpy(), o2), "obs step %d" % t
        if dn2.any():
            episodes += int(dn2.sum())
            for s, (lo, hi) in enumerate(ds.ranges):
                if dn2[lo:hi].any():
                    ds.reset_shard(s, env_mask=dn2[lo:hi])
            for b in np.nonzero(dn2)[0]:
                orc.envs[b].reset()
    assert episodes >= 2 * B
    ds.check_errors()
    for s, (lo, hi) in enumerate(ds.ranges):
        env = ds.envs[s]
        st = product_envs.canonical(env)
        enc = env.grid.encode().cpu().numpy()
        for b in range(lo, hi):
            canon.assert_same(st[b - lo], canon.oracle_canonical(orc.envs[b]), "env %d (shard %d)" % (b, s))
            assert np.array_equal(enc[b - lo], orc.envs[b].encode()), b
            assert seeding.same_stream(env.numpy_rng_state(b - lo), orc.envs[b].mt_state()), b


# ---- 3. options reach every shard -----------------------------------------------------------------------------------------------
def _pair(B, k, **kw):
    from marlgrid_amd.envs import make
    return _sharded(B, k, seed=77, **kw), make(NAME, batch_size=B, seed=77, **kw)


def test_option_encoded_views():
    import torch
    B, k = 515, 3
    ds, one = _pair(B, k, obs_format="encoded", auto_reset=True, max_steps=30)
    assert all(e.obs_format == "encoded" for e in ds.envs) and ds.kernel_names == [one.kernel_name] * k
    o = ds.gather(ds.reset())
    assert o.shape == (B, 3, 7, 7, 3) and torch.equal(o, one.reset())
    g = torch.Generator().manual_seed(3)
    for t in range(70):
        a = torch.randint(0, 7, (B, 3), generator=g)
        o, r, d, _ = ds.gather(ds.step(a))
        o2, r2, d2, _ = one.step(a)
        assert torch.equal(o, o2) and torch.equal(r, r2) and torch.equal(d, d2), t
    ds.check_errors()


def test_option_next_step_reset_with_episode_info():
    """the info dicts gathered equal the one env's, and so do the observations of the steps that end an episode (in next-step
    mode: the TERMINAL observations) and of the reset calls that follow"""
    import torch
    B, k = 515, 3
    ds, one = _pair(B, k, auto_reset="next_step", episode_info=True, max_steps=30)
    assert all(e.auto_reset_mode == "next_step" and e.episode_info and e._use_ep for e in ds.envs)
    assert torch.equal(ds.gather(ds.reset()), one.reset())
    g = torch.Generator().manual_seed(4)
    terminal = resets = 0
    for t in range(100):
        a = torch.randint(0, 7, (B, 3), generator=g).to("cuda:0")
        o, r, d, info = ds.gather(ds.step(a))
        o2, r2, d2, info2 = one.step(a)
        assert set(info) == set(INFO_KEYS) == set(info2)
        for key in INFO_KEYS:
            assert info[key].dtype == info2[key].dtype and torch.equal(info[key], info2[key]), (t, key)
        assert torch.equal(o, o2) and torch.equal(r, r2) and torch.equal(d, d2), t
        assert torch.equal(o[d2], o2[d2])                    # the terminal observations, explicitly
        terminal += int(d2.sum())
        resets += int(info2["reset"].sum())
    assert terminal >= 3 * B and resets >= 2 * B
    _same_state(ds.state_dict(), one.state_dict())            # ep_return_t included
    assert "ep_return_t" in ds.state_dict()
    ds.check_errors()


def test_option_encode_in_step():
    import torch
    B, k = 515, 3
    ds, one = _pair(B, k, encode_in_step=True, auto_reset=True, max_steps=30)
    ds.reset(), one.reset()
    g = torch.Generator().manual_seed(5)
    for t in range(50):
        a = torch.randint(0, 7, (B, 3), generator=g)
        parts = ds.step(a)
        o2 = one.step(a)[0]
        assert torch.equal(ds.gather([p[0] for p in parts]), o2), t
        for s in range(k):                                      # grid_encoding per shard: the one env's rows (compared on the
            # current stream, which gather() has just ordered behind every shard's and on which the one env stepped)
            assert torch.equal(ds.envs[s].grid_encoding, ds.shard(s, one.grid_encoding)), (t, s)
    assert torch.equal(ds.gather([e.grid_encoding for e in ds.envs]), one.grid.encode())
    ds.check_errors()


def test_other_options_and_sharded_classmethod():
    """fused_step=False, obs_buffers, strict=False and per-agent views (the per-agent list of observations) through
    MultiGridEnv.sharded, with shard 0 built on the agents themselves and the others on shallow copies"""
    import torch
    from marlgrid_amd.agents import GridAgentInterface
    from marlgrid_amd.envs import ClutteredMultiGrid
    B, k = 130, 3
    team = lambda: [GridAgentInterface(color="red", view_size=7, view_tile_size=8), GridAgentInterface(color="blue", view_size=5, view_tile_size=8)]
    kw = dict(grid_size=9, n_clutter=4, batch_size=B, seed=9, auto_reset=True, fused_step=False, obs_buffers=3, strict=False, max_steps=25)
    mine = team()
    ds = ClutteredMultiGrid.sharded(mine, _devices(k), streams=_streams(k), **kw)
    one = ClutteredMultiGrid(agents=team(), **kw)
    assert ds.envs[0].agents[0] is mine[0] and ds.envs[1].agents[0] is not mine[0] and ds.agents is ds.envs[0].agents
    assert ds.num_agents == 2 and all(e._hetero and not e.fused_step and e.obs_buffers == 3 and e.strict is False for e in ds.envs)
    ro, ro2 = ds.gather(ds.reset()), one.reset()
    assert isinstance(ro, list) and all(torch.equal(x, y) for x, y in zip(ro, ro2))
    g = torch.Generator().manual_seed(6)
    for t in range(60):
        a = torch.randint(0, 7, (B, 2), generator=g)
        o, r, d, _ = ds.gather(ds.step(a))
        o2, r2, d2, _ = one.step(a)
        assert len(o) == 2 and o[0].shape == (B, 56, 56, 3) and o[1].shape == (B, 40, 40, 3)
        assert all(torch.equal(x, y) for x, y in zip(o, o2)) and torch.equal(r, r2) and torch.equal(d, d2), t
    ds.check_errors()


# ---- 4. the forms of `actions` ------------------------------------------------------------------------------------------------------
def test_three_forms_of_actions_and_the_per_shard_loop():
    """a host array, a cuda:0 tensor nobody synchronised, a list with one tensor per shard made under on(k), and step_shard under
    on(k) in the double-buffered loop: the same results, those of the one env"""
    import torch
    from marlgrid_amd.envs import make
    B, k, T = 1001, 3, 60
    kw = dict(seed=21, auto_reset=True, max_steps=40)
    host, dev, lst, loop = (_sharded(B, k, **kw) for _ in range(4))
    one = make(NAME, batch_size=B, **kw)
    obs = [x.reset() for x in (host, dev, lst, loop)]
    want = one.reset()
    assert all(torch.equal(x.gather(o), want) for x, o in zip((host, dev, lst, loop), obs))
    rng = np.random.RandomState(8)
    scratch = torch.zeros((B, 3), dtype=torch.int64, device="cuda:0")
    for t in range(T):
        a = rng.randint(0, 7, size=(B, 3))
        want = one.step(torch.from_numpy(a))
        got = [host.gather(host.step(a))]                                           # numpy, whole batch
        # a device tensor whose producer is still queued when step() is called: written by a kernel on the current stream
        scratch.zero_()
        on_dev = scratch + torch.from_numpy(a).to("cuda:0", non_blocking=True)
        got.append(dev.gather(dev.step(on_dev)))
        per = []
        for s in range(k):
            with lst.on(s):                                                          # made on the shard's own stream
                per.append(torch.from_numpy(a[lst.ranges[s][0]:lst.ranges[s][1]]).to(lst.devices[s]))
        got.append(lst.gather(lst.step(per)))
        parts = []
        for s in range(k):                                                           # the double-buffered sampler's loop
            with loop.on(s):
                assert torch.cuda.current_stream() == loop.streams[s] and torch.cuda.current_device() == loop.devices[s].index
                act = torch.from_numpy(loop.shard(s, a)).to(loop.devices[s])
                parts.append(loop.step_shard(s, act))
        got.append(loop.gather(parts))
        for i, (o, r, d, _) in enumerate(got):
            assert torch.equal(o, want[0]) and torch.equal(r, want[1]) and torch.equal(d, want[2]), (t, i)
    with pytest.raises(ValueError):
        host.step([a, a])                      # a list has one entry per shard
    with pytest.raises(AssertionError):
        host.step(a[:-1])
    # gather to another place: the host
    o = host.gather(host.step(a), device="cpu")[0]
    assert o.device.type == "cpu" and torch.equal(o, one.step(torch.from_numpy(a))[0].cpu())
    for x in (host, dev, lst, loop):
        x.check_errors()


# ---- 5. checkpoints reshard -------------------------------------------------------------------------------------------------------
def test_checkpoint_from_8_shards_loads_into_one_env_2_shards_and_a_pipeline():
    import torch
    from marlgrid_amd.envs import make
    B = 1030                                   # 8 shards of 129 / 128 envs; 2 shards and 2 parts of 515
    kw = dict(auto_reset=True)
    ds8 = _sharded(B, 8, seed=1337, **kw)
    ds8.reset()
    g = torch.Generator().manual_seed(12)
    for t in range(60):
        ds8.step(torch.randint(0, 7, (B, 3), generator=g))
    sd = ds8.state_dict()
    assert all(v.device.type == "cpu" for v in sd.values())
    one = make(NAME, batch_size=B, seed=1, **kw)              # (other seeds: what they step afterwards is the checkpoint's)
    ds2 = _sharded(B, 2, seed=2, **kw)
    pipe = make(NAME, batch_size=B, seed=3, pipeline=2, streams=_streams(2), **kw)
    assert set(sd) == set(one.state_dict()) and all(sd[key].shape == v.shape for key, v in one.state_dict().items())
    for target in (one, ds2, pipe):
        target.load_state_dict(sd)
    _same_state(ds2.state_dict(), sd), _same_state(pipe.state_dict(), sd), _same_state(one.state_dict(), sd)
    n_done = 0
    for t in range(50):                                        # across the time limit at step 100
        a = torch.randint(0, 7, (B, 3), generator=g).to("cuda:0")
        torch.cuda.current_stream().synchronize()              # (ShardPipeline.step asks for ready actions)
        want = one.step(a)
        got = [ds8.gather(ds8.step(a)), ds2.gather(ds2.step(a))]
        parts = pipe.step(a)
        pipe.synchronize()
        got.append(tuple(torch.cat([p[i] for p in parts]) for i in range(3)))
        for i, res in enumerate(got):
            assert torch.equal(res[0], want[0]) and torch.equal(res[1], want[1]) and torch.equal(res[2], want[2]), (t, i)
        n_done += int(want[2].sum())
    assert n_done >= B
    _same_state(ds8.state_dict(), one.state_dict()), _same_state(pipe.state_dict(), one.state_dict())
    for target in (one, ds2, pipe, ds8):
        target.check_errors()


# ---- 6. errors ------------------------------------------------------------------------------------------------------------------------
def _no_walls_class():
    """the scenario of tests/test_hip_parity.py::test_error_paths_raise_like_the_reference: a room without its walls — an agent
    that walks to the edge looks at a cell outside the grid (MultiGrid.get asserts, base.py:154-156)"""
    from marlgrid_amd.base import MultiGrid, MultiGridEnv
    from marlgrid_amd.objects import Wall

    class NoWalls(MultiGridEnv):
        def _gen_grid(self, width, height):
            self.grid = MultiGrid((width, height))
            self.grid.horz_wall(0, 0, width, obj_type=Wall)       # top row only
    return NoWalls


def _walk_only_in_shard(ds, s, g):
    """actions under which only shard s's agents walk: the others turn left on the spot — where `_park` put them, in the
    middle of the room, every cell they can face is inside the grid"""
    import torch
    a = torch.zeros((ds.batch_size, 1), dtype=torch.int64)
    lo, hi = ds.ranges[s]
    a[lo:hi] = torch.randint(0, 3, (hi - lo, 1), generator=g)
    return a


def _park(ds, shards):
    """(an agent that FACES a cell outside the grid is the error, whatever its action: the agents of the shards that must stay
    clean are moved off the edge)"""
    for s in shards:
        with ds.on(s):
            ds.envs[s].set_agent(0, x=1, y=1)


@pytest.mark.parametrize("strict", [True, False])
def test_error_in_shard_2_raises_like_the_env_and_names_the_shard(strict):
    import torch
    from marlgrid_amd.agents import GridAgentInterface
    NoWalls = _no_walls_class()
    kw = dict(grid_size=4, batch_size=26, max_steps=1000, strict=strict)
    ds = NoWalls.sharded([GridAgentInterface(view_tile_size=8)], _devices(3), streams=_streams(3), **kw)
    assert ds.ranges == [(0, 9), (9, 18), (18, 26)]
    ds.reset()
    _park(ds, (0, 1))
    g = torch.Generator().manual_seed(0)
    if strict:
        with pytest.raises(AssertionError) as err:
            for _ in range(200):
                ds.step(_walk_only_in_shard(ds, 2, g))         # raised by a later step(): the error flag is polled
            ds.check_errors()
    else:
        for _ in range(200):
            ds.step(_walk_only_in_shard(ds, 2, g))             # nothing raises on the way
        with pytest.raises(AssertionError) as err:
            ds.check_errors()
    msg = str(err.value)
    print("\nstrict=%r: %s" % (strict, msg))
    assert type(err.value) is AssertionError                   # the type the env itself raises (test_error_paths_...)
    assert "shard 2" in msg and "[18, 26)" in msg and "an agent left a cell it is not in" in msg
    # the same scenario as ONE env raises the same type
    one = NoWalls(agents=[GridAgentInterface(view_tile_size=8)], **dict(kw, strict=False))
    one.reset()
    for _ in range(200):
        one.step(torch.randint(0, 3, (26, 1), generator=g))
    with pytest.raises(AssertionError):
        one.check_errors()
    # shards 0 and 1 had no error: their own checks pass
    for s in (0, 1):
        with ds.on(s):
            ds.envs[s].check_errors()


# ---- 7. placement ---------------------------------------------------------------------------------------------------------------------
def test_repeated_device_gives_every_shard_its_share():
    """k shards on one device: each shard's placement search counts on 1 / k of the free memory.  Whether the fast class was
    found is printed, not asserted (DESIGN.md section 3.4 calls it a lottery)."""
    ds = _sharded(32768, 2, auto_reset=True)                   # 2 x 462 MB buffers: above the 256 MiB threshold, placed
    for s, rec in enumerate(ds.obs_placement):
        assert len(rec) == 1 and rec[0] is not None and rec[0]["share"] == 2, (s, rec)
        print("\nshard %d of 2: found=%r kept=%r ms, %d candidates, stopped: %s" % (s, rec[0].get("found"), rec[0].get("kept"),
                                                                                 rec[0].get("candidates", 0), rec[0].get("stopped")))
    ds.close()
    del ds
    # ... merged into a caller's dict (small buffers placed because the caller lowers the threshold), and a caller's own share kept
    ds = _sharded(3000, 3, place_obs={"min_bytes": 1 << 20, "seconds": 0.3})
    assert [rec[0]["share"] for rec in ds.obs_placement] == [3, 3, 3]
    ds.close()
    ds = _sharded(3000, 3, place_obs={"min_bytes": 1 << 20, "seconds": 0.3, "share": 5})
    assert [rec[0]["share"] for rec in ds.obs_placement] == [5, 5, 5]
    ds.close()
    ds = _sharded(3000, 3, place_obs=False)
    assert ds.obs_placement == [[], [], []]
    ds.close()
    ds = _sharded(3000, 1, place_obs={"min_bytes": 1 << 20, "seconds": 0.3})       # one shard on its device: nothing merged
    assert ds.obs_placement[0][0]["share"] == 1
    ds.close()


# ---- 8. distinct devices --------------------------------------------------------------------------------------------------------------
def test_two_distinct_devices_equal_the_one_env():
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one HIP device visible: distinct devices need two")
    assert _invariance(4099, ["cuda:0", "cuda:1"], [_streams(1, "cuda:0")[0], _streams(1, "cuda:1")[0]], 150) >= 4099
