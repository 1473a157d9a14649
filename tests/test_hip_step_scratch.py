"""GPU (-m gpu): the kernels that carve the env step's LDS scratch with mg_step_layout.h's functions — step_kernel<64>,
step_kernel<256> and the step phase of encode_views_kernel — against the CPU oracle, at the shapes where a wrong column
would show: odd numbers of envs per workgroup, tail workgroups, more than 16 agents (the `ord` column), the smallest
batch that takes 256-lane workgroups and the smallest agent count that no longer does.  Every run is max_steps + 20
steps with auto_reset, so every env resets inside the launch at least once (the 131 073-env runs: 30 steps).

Envs per workgroup of the fused step + views launch (launch_encode_views: at most 256 / n whole envs, halved until the
workgroup's views fit 48 KiB): 3 agents at view 7 -> 42, 3 agents at view 5 -> 85 (the record area an odd number of
8-byte words), 24 agents at view 5 -> 10.
"""
import numpy as np
import pytest

import canon
import product_envs
import scenarios
from marlgrid_amd import seeding
from oracle import oracle as O
from test_hip_encoded_views import _check as _check_views

pytestmark = pytest.mark.gpu
REW_TOL = 1e-6


def _final_state(env, orc, ids, what):
    """canonical state and the RNG in numpy's form of envs `ids` against oracle envs 0 .. len(ids) - 1"""
    env.check_errors()
    st = product_envs.canonical_arrays(env.scenario_spec(), env.grid.grid[ids].cpu().numpy(), env.agent_state[ids].cpu().numpy(),
                                       env.step_count[ids].cpu().numpy())
    for j, b in enumerate(ids):
        canon.assert_same(st[j], canon.oracle_canonical(orc.envs[j]), "%s env %d" % (what, b))
        assert seeding.same_stream(env.numpy_rng_state(int(b)), orc.envs[j].mt_state()), (what, b)


# (scenario, B): the issue's two shapes, and the one that really puts 85 envs into a workgroup of the encoded path
SMALL = [("Test-3AgentSpawnRect9x9", 86), ("Limit-24AgentEmpty20x20-view5", 12), ("Test-3AgentEmpty7x7-spawn-delay", 86)]


@pytest.mark.parametrize("path", ["mg_step", "mg_step_encode_views"])
@pytest.mark.parametrize("name,B", SMALL, ids=[c[0] for c in SMALL])
def test_step_paths_vs_oracle(name, B, path):
    """mg_step (fused_step=False: the step, then the raster) and mg_step_encode_views (obs_format="encoded": the step and
    the views in one launch): rewards and done every step; canonical state, RNG and observations after the last"""
    import torch
    spec = scenarios.registered(name)
    seeds = 7300 + np.arange(B)
    kw = dict(fused_step=False) if path == "mg_step" else dict(obs_format="encoded")
    env = product_envs.build(name, batch_size=B, seeds=seeds, auto_reset=True, **kw)
    n, steps = env.num_agents, spec["max_steps"] + 20
    orc = O.OracleBatch(spec, seeds)
    env.reset()
    orc.reset()
    rng = np.random.RandomState(5)
    resets = np.zeros(B, bool)
    for t in range(steps):
        a = rng.randint(0, 7, size=(B, n))
        last = t == steps - 1
        obs, r, d, _ = env.step(torch.from_numpy(a))
        o2, r2, d2, _ = orc.step(a, render=last and path == "mg_step", auto_reset=True)
        assert np.abs(r.cpu().numpy().astype(np.float64) - r2).max() <= REW_TOL, t
        assert np.array_equal(d.cpu().numpy(), d2), t
        resets |= d2.astype(bool)
    assert resets.all()
    if path == "mg_step":
        assert np.array_equal(obs.cpu().numpy(), o2)
    else:
        _check_views(obs, orc.envs, n, "last step")
    _final_state(env, orc, np.arange(B), name)


WIDE = [("MarlGrid-3AgentEmpty9x9-v0", 256, 257), ("Edge-14AgentEmpty8x8-view3", 64, 65)]


@pytest.mark.parametrize("name,head,tail", WIDE, ids=[c[0] for c in WIDE])
def test_step_at_131073_envs_vs_oracle(name, head, tail):
    """B = 131 073, the smallest batch past mg_step's 256-lane threshold: with 3 agents step_kernel<256> (512 full workgroups
    and a tail workgroup of one env), with 14 agents — one more than the rule admits — step_kernel<64>.  mg_step + the views
    launch (obs_format="encoded", fused_step=False: the observations stay small), 30 steps.  The oracle steps ALL envs
    (nothing rendered): done of every env every step, and at the end every env's step count, with no error anywhere.  The
    first `head` and the last `tail` envs besides: rewards every step, canonical state, RNG and views at the end.
    (The oracle of all envs is what the case costs: about 3 s on 16 CPUs, 9 s on 8 — building 131 073 oracle envs, 30
    OpenMP steps, reading their step counts back.)"""
    import torch
    B, steps = 131073, 30
    spec = scenarios.registered(name)
    ids = np.concatenate([np.arange(head), np.arange(B - tail, B)])
    env = product_envs.build(name, batch_size=B, seeds=1337 + np.arange(B), auto_reset=True, obs_format="encoded", fused_step=False)
    n = env.num_agents
    orc = O.OracleBatch(spec, 1337 + np.arange(B))
    env.reset()
    for e in orc.envs:
        e.L.mgo_reset(e.h, 1)           # (OracleEnv.reset without its rendered observation)
    g = torch.Generator().manual_seed(3)
    for t in range(steps):
        a = torch.randint(0, 7, (B, n), generator=g)
        obs, r, d, _ = env.step(a)
        _, r2, d2, _ = orc.step(a.numpy(), render=False, auto_reset=True)
        assert np.array_equal(d.cpu().numpy(), d2), t
        assert np.abs(r[ids].cpu().numpy().astype(np.float64) - r2[ids]).max() <= REW_TOL, t
    assert not bool((env.error_t != 0).any())
    assert np.array_equal(env.step_count.cpu().numpy(), [e.state()["step_count"] for e in orc.envs])
    obs = [o[ids] for o in obs] if isinstance(obs, list) else obs[ids]
    sub = O.OracleBatch.__new__(O.OracleBatch)
    sub.envs = [orc.envs[b] for b in ids]
    _check_views(obs, sub.envs, n, "last step")
    _final_state(env, sub, ids, name)


def test_frame_of_the_largest_view_golden():
    """env.render() with the highlight at view 31 (mg_frame's view map and its in-memory shadow cast): one frame of the
    reference's MultiGridEnv.render(mode='rgb_array', tile_size=8, show_agent_views=False), whole
    (tests/golden/frame_view31.npz)"""
    import os
    import torch
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frame_view31.npz"))
    env = product_envs.build(str(g["name"]), batch_size=1, seeds=[int(g["seed"])])
    env.reset()
    for a in g["actions"]:
        env.step(torch.from_numpy(a[None].astype(np.int64)))
    img = env.render(tile_size=int(g["tile_size"]), show_agent_views=False).cpu().numpy()
    assert img.shape == g["full"].shape and np.array_equal(img, g["full"])
    assert (g["full"] != env.render(tile_size=int(g["tile_size"]), show_agent_views=False, highlight=False).cpu().numpy()).any()
