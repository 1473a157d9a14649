"""GPU (-m gpu): MultiGridEnv(specialize=...) — the observation kernel compiled at construction time for a (view, tile) pair the
library's table of instantiations lacks (mg_render_specialize: hipRTC), launched instead of the table's fully run-time kernel.
Every shape against a twin built without `specialize` (byte-identical, every step) and, for the plain step, against the CPU
oracle; the variants with the encode and with the episode outputs; view groups; shards; what is not specialised.

One cache directory for the module: an instantiation is compiled once (~5 s), whatever number of envs ask for it.  The tests
run where libhiprtc loads — on the MI355X machine it must: a missing libhiprtc fails them, it does not skip them."""
import warnings

import numpy as np
import pytest

import scenarios
from oracle import oracle as O

pytestmark = pytest.mark.gpu
REW_TOL = 1e-6          # per step: tests/test_core_hostemu.py
GENERIC = "fully run-time instantiation"


@pytest.fixture(scope="module")
def cache(tmp_path_factory):
    return str(tmp_path_factory.mktemp("marlgrid_spec_cache"))


def team(n, view, tile, colors=None):
    from marlgrid_amd.agents import GridAgentInterface
    colors = colors or scenarios.REG_COLORS[:n]
    return [GridAgentInterface(color=c, view_size=view, view_tile_size=tile) for c in colors]


def cluttered(agents, B, seeds, **kw):
    """cluttered 15 x 15 (12 blocks), as scenarios.cluttered_spec(n, 15, view, n_clutter=12, tile_size=tile) describes it"""
    from marlgrid_amd.envs import ClutteredMultiGrid
    return ClutteredMultiGrid(agents=agents, grid_size=15, n_clutter=12, batch_size=B, seeds=seeds, place_obs=False, **kw)


def build_pair(view, tile, B, cache, n=3, seed0=7000, **kw):
    """(specialised env, twin without `specialize`, warnings of each) on the same seeds"""
    from marlgrid_amd import base
    seeds = seed0 + np.arange(B)
    base._GENERIC_WARNED.clear()      # (the warning is said once per configuration and process: every pair starts unsaid)
    with warnings.catch_warnings(record=True) as w_env:
        warnings.simplefilter("always")
        env = cluttered(team(n, view, tile), B, seeds, specialize=True, specialize_cache=cache, **kw)
    with warnings.catch_warnings(record=True) as w_twin:
        warnings.simplefilter("always")
        twin = cluttered(team(n, view, tile), B, seeds, **kw)
    said = lambda ws: [str(w.message) for w in ws if GENERIC in str(w.message)]
    return env, twin, said(w_env), said(w_twin)


def same(a, b, what):
    import torch
    assert a.shape == b.shape and torch.equal(a, b), what


def run_vs_oracle_and_twin(view, tile, B, T, cache, name, max_steps=20, twin_warns=True):
    import torch
    env, twin, said_env, said_twin = build_pair(view, tile, B, cache, auto_reset=True, max_steps=max_steps)
    assert env.kernel_name == name and twin.kernel_name.startswith("mg::render_kernel<0, ")
    # (the warning is for the FULLY run-time instantiation: view 11 at 8-pixel tiles has its tile size compiled in on the table)
    assert bool(said_twin) == twin.kernel_name.startswith("mg::render_kernel<0, 0, ") == twin_warns and not said_env
    info = env.specialization
    assert len(info) == 1 and info[0]["kernel_name"] == name and info[0]["scratch_bytes"] == 0 and info[0]["want"] == 0
    orc = O.OracleBatch(scenarios.cluttered_spec(3, 15, view, n_clutter=12, tile_size=tile, max_steps=max_steps), 7000 + np.arange(B))
    o0 = env.reset()
    same(o0, twin.reset(), "reset")
    assert np.array_equal(o0.cpu().numpy(), orc.reset())
    rng = np.random.RandomState(3)
    ends = 0
    for t in range(T):
        a = rng.randint(0, 7, size=(B, 3))
        at = torch.from_numpy(a)
        o, r, d, _ = env.step(at)
        o2, r2, d2, _ = twin.step(at)
        same(o, o2, "obs step %d" % t), same(r, r2, "rewards step %d" % t), same(d, d2, "done step %d" % t)
        o3, r3, d3, _ = orc.step(a, auto_reset=True)
        assert np.array_equal(o.cpu().numpy(), o3), "obs vs oracle, step %d" % t
        assert np.abs(r.cpu().numpy().astype(np.float64) - r3).max() <= REW_TOL
        assert np.array_equal(d.cpu().numpy(), d3)
        ends += int(d3.sum())
    assert ends >= B * (T // max_steps)      # every env ran into its time limit: the fused reset is part of what was compared
    env.check_errors()
    return env


# A. the three shapes VERDICT r06 names, 67 envs: odd batches of 8 per wave, a ragged last workgroup
@pytest.mark.parametrize("view,tile,name", [(13, 4, "mg::render_kernel<13, 0, 4, 0, 0>"),
                                            (17, 5, "mg::render_kernel<17, 5, 4, 0, 2>"),
                                            (10, 6, "mg::render_kernel<10, 6, 4, 0, 2>")])
def test_off_table_shapes_vs_oracle_and_twin(view, tile, name, cache):
    run_vs_oracle_and_twin(view, tile, 67, 60, cache, name)


# B. one env: one wave of one workgroup with a batch of one
def test_one_env_batch(cache):
    run_vs_oracle_and_twin(11, 8, 1, 30, cache, "mg::render_kernel<11, 8, 4, 0, 0>", twin_warns=False)


# C. from 4096 envs on the workgroup is the larger one (8 waves: view 10 > 9)
def test_large_batch_takes_the_8_wave_workgroup(cache):
    import torch
    B = 4099
    env, twin, _, _ = build_pair(10, 6, B, cache, auto_reset=True, max_steps=20)
    assert env.kernel_name == "mg::render_kernel<10, 6, 8, 0, 2>"
    same(env.reset(), twin.reset(), "reset")
    rng = np.random.RandomState(4)
    for t in range(12):
        at = torch.from_numpy(rng.randint(0, 7, size=(B, 3)))
        o, r, d, _ = env.step(at)
        o2, r2, d2, _ = twin.step(at)
        same(o, o2, "obs step %d" % t), same(r, r2, "rewards step %d" % t), same(d, d2, "done step %d" % t)
    env.check_errors()


# D. the encode variant: the table has <6, 8, ., 0, 0> but no + 16 of it — a specialised env writes grid.encode() from the step's launch
def test_encode_variant(cache):
    import torch
    B = 67
    env, twin, _, _ = build_pair(6, 8, B, cache, auto_reset=True, max_steps=20, encode_in_step=True)
    assert env.kernel_name == twin.kernel_name == "mg::render_kernel<6, 8, 4, 0, 0>"      # the plain step: the table's own
    same(env.reset(), twin.reset(), "reset")
    second_launches = []
    encode_into = env._encode_into
    # (mg_encode into the step's own buffer is the second launch; grid.encode() below goes through the same method into a tensor of its own)
    env._encode_into = lambda out, vm=None: (second_launches.append(out is env.grid_encoding), encode_into(out, vm))[1]
    rng = np.random.RandomState(5)
    for t in range(30):
        at = torch.from_numpy(rng.randint(0, 7, size=(B, 3)))
        o, r, d, _ = env.step(at)
        o2, r2, d2, _ = twin.step(at)
        same(o, o2, "obs step %d" % t), same(r, r2, "rewards step %d" % t), same(d, d2, "done step %d" % t)
        same(env.grid_encoding, twin.grid_encoding, "encoding vs twin, step %d" % t)
        same(env.grid_encoding, env.grid.encode(), "encoding vs grid.encode(), step %d" % t)
    info = [i for i in env.specialization if i["want"] == 1]
    assert len(info) == 1 and info[0]["kernel_name"] == "mg::render_kernel<6, 8, 4, 16, 0>" and ", 16," in info[0]["kernel_name"]
    assert second_launches and not any(second_launches) and env._enc_fused       # mg_encode never followed a step; the table's fused encode was never asked
    assert twin._enc_fused is False                     # ... which the twin's step needed every time
    env.check_errors()


# E. the episode variant
def test_episode_variant(cache):
    import torch
    B = 67
    env, twin, _, _ = build_pair(9, 7, B, cache, auto_reset="next_step", episode_info=True, max_steps=15)
    assert env.kernel_name == "mg::render_kernel<9, 7, 4, 0, 2>"
    same(env.reset(), twin.reset(), "reset")
    rng = np.random.RandomState(6)
    resets = 0
    for t in range(60):
        at = torch.from_numpy(rng.randint(0, 7, size=(B, 3)))
        o, r, d, info = env.step(at)
        o2, r2, d2, info2 = twin.step(at)
        same(o, o2, "obs step %d" % t), same(r, r2, "rewards step %d" % t), same(d, d2, "done step %d" % t)
        assert set(info) == set(info2) == {"terminated", "truncated", "episode_return", "episode_length", "reset"}
        for k in info:
            same(info[k], info2[k], "info[%s] step %d" % (k, t))
        resets += int(info["reset"].sum())
    assert resets >= 3 * B
    names = {i["want"]: i["kernel_name"] for i in env.specialization}
    assert names == {0: "mg::render_kernel<9, 7, 4, 0, 2>", 2: "mg::render_kernel<9, 7, 4, 32, 2>"}
    assert env._ep_fused and twin._ep_fused is False
    env.check_errors()


def hetero_pair(views, B, cache):
    from marlgrid_amd.agents import GridAgentInterface
    seeds = 7100 + np.arange(B)
    mk = lambda: [GridAgentInterface(color=c, view_size=v, view_tile_size=t) for c, (v, t) in zip(scenarios.REG_COLORS, views)]
    env = cluttered(mk(), B, seeds, auto_reset=True, max_steps=20, specialize="auto", specialize_cache=cache)
    twin = cluttered(mk(), B, seeds, auto_reset=True, max_steps=20)
    return env, twin


# F. view groups: one raster launch per group, one handle per group that has something to gain.  The first case is the
# issue's — (7, 8) is the table's headline shape and (11, 5) one of its gather entries: nothing is compiled, the lists are the
# twin's —; the other two have a group (both groups) off the table.
@pytest.mark.parametrize("views,names", [
    (((7, 8), (11, 5)), ["mg::render_kernel<7, 8, 4, 0, 0>", "mg::render_kernel<11, 5, 4, 0, 2>"]),
    (((7, 8), (11, 6)), ["mg::render_kernel<7, 8, 4, 0, 0>", "mg::render_kernel<11, 6, 4, 0, 2>"]),
    (((13, 4), (10, 6)), ["mg::render_kernel<13, 0, 4, 0, 0>", "mg::render_kernel<10, 6, 4, 0, 2>"])])
def test_view_groups(views, names, cache):
    import torch
    B = 35
    env, twin = hetero_pair(views, B, cache)
    assert [g.kernel_name for g in env._groups] == names
    off_table = [k for k, g in enumerate(twin._groups) if g.kernel_name != names[k]]
    info = env.specialization
    assert [i["group"] for i in info] == off_table and all(i["want"] == 0 for i in info)      # one handle per such group
    assert [i["kernel_name"] for i in info] == [names[k] for k in off_table]
    o, o2 = env.reset(), twin.reset()
    assert isinstance(o, list) and len(o) == len(o2) == 2
    rng = np.random.RandomState(7)
    for t in range(25):
        at = torch.from_numpy(rng.randint(0, 7, size=(B, 2)))
        o, r, d, _ = env.step(at)
        o2, r2, d2, _ = twin.step(at)
        for k in range(2):
            same(o[k], o2[k], "agent %d step %d" % (k, t))
        same(r, r2, "rewards step %d" % t), same(d, d2, "done step %d" % t)
    env.check_errors()


# G. what is not specialised: True says so, "auto" runs as before
def test_prestige_is_not_specialised(cache):
    import torch
    from marlgrid_amd import base
    B, seeds = 35, 7200 + np.arange(35)
    colors = ["prestige", "blue", "purple"]
    with pytest.raises(NotImplementedError, match="prestige"):
        cluttered(team(3, 13, 4, colors), B, seeds, specialize=True, specialize_cache=cache)
    base._GENERIC_WARNED.clear()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        env = cluttered(team(3, 13, 4, colors), B, seeds, specialize="auto", specialize_cache=cache)
    twin = cluttered(team(3, 13, 4, colors), B, seeds)
    assert [m for m in w if GENERIC in str(m.message)] and env.specialization == []
    assert env.kernel_name == twin.kernel_name and env.kernel_name.endswith(", 9, 0>")
    same(env.reset(), twin.reset(), "reset")
    rng = np.random.RandomState(8)
    for t in range(10):
        at = torch.from_numpy(rng.randint(0, 7, size=(B, 3)))
        o, r, d, _ = env.step(at)
        o2, r2, d2, _ = twin.step(at)
        same(o, o2, "obs step %d" % t), same(r, r2, "rewards step %d" % t), same(d, d2, "done step %d" % t)
    with pytest.raises(ValueError):
        cluttered(team(3, 13, 4), B, seeds, specialize="yes")


# H. shards of one process: compiled once, loaded per shard
def test_shards_share_one_compile(cache, tmp_path):
    import torch
    from marlgrid_amd import envs as E
    name = "Test-3AgentCluttered15x15-view11"
    if name not in E._registry:      # (registered ids draw 8-pixel tiles: view 11 there is off the table)
        E.register_marl_env(name, E.ClutteredMultiGrid, n_agents=3, grid_size=15, view_size=11, env_kwargs=dict(n_clutter=12))
    B = 70
    fresh = str(tmp_path / "cache")      # (nobody compiled into this one: the second shard's hit is this process's memory or this directory)
    ds = E.make(name, devices=[0, 0], batch_size=B, seed=7300, place_obs=False, auto_reset=True, max_steps=20, specialize=True,
                specialize_cache=fresh)
    one = E.make(name, batch_size=B, seed=7300, place_obs=False, auto_reset=True, max_steps=20)
    assert ds.kernel_names == ["mg::render_kernel<11, 8, 4, 0, 0>"] * 2 and one.kernel_name == "mg::render_kernel<0, 8, 4, 0, 0>"
    infos = [env.specialization for env in ds.envs]
    assert [len(i) for i in infos] == [1, 1]
    assert infos[1][0]["cache_hit"] != 0 and infos[1][0]["compile_seconds"] == 0
    assert infos[0][0]["code_bytes"] == infos[1][0]["code_bytes"] > 0
    same(ds.gather(ds.reset()), one.reset(), "reset")
    rng = np.random.RandomState(9)
    for t in range(25):
        a = rng.randint(0, 7, size=(B, 3))
        o, r, d, _ = ds.gather(ds.step(a))
        o2, r2, d2, _ = one.step(torch.from_numpy(a))
        same(o, o2, "obs step %d" % t), same(r, r2, "rewards step %d" % t), same(d, d2, "done step %d" % t)
    for env in ds.envs:
        env.check_errors()


def test_handles_are_released_and_rebuilt_with_the_tables(cache):
    """a new object kind rebuilds atlas and object table: the group's handle is released and asked for again (the LDS layout it
    was compiled for may have changed); a released env's handles are gone"""
    import torch
    from marlgrid_amd.objects import Key
    B = 35
    env, twin, _, _ = build_pair(13, 4, B, cache, seed0=7400)
    same(env.reset(), twin.reset(), "reset")
    h0 = env._groups[0].spec[0].value
    for e in (env, twin):
        e.put_obj(Key(color="blue"), 3, 3)
    same(env.gen_obs(), twin.gen_obs(), "after a new object kind")
    assert env._groups[0].spec[0] and env.kernel_name == "mg::render_kernel<13, 0, 4, 0, 0>"
    rng = np.random.RandomState(10)
    for t in range(5):
        at = torch.from_numpy(rng.randint(0, 7, size=(B, 3)))
        same(env.step(at)[0], twin.step(at)[0], "obs step %d" % t)
    assert h0 is not None
    env._release_spec()
    assert env._groups[0].spec == {} and env.specialization == []
    same(env.gen_obs(), twin.gen_obs(), "after a release")                              # asked for again by the next launch: a hit
    assert env.specialization[0]["cache_hit"] != 0 and env.specialization[0]["compile_seconds"] == 0
