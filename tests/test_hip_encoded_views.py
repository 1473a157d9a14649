"""GPU (-m gpu): obs_format="encoded" — every agent's gen_obs_grid(agent) -> grid.encode(vis_mask) (base.py:418-451,
196-214) written by the step's launch, against the CPU oracle's composition of the same two functions (mgo_view's
post-hide_item_types top codes and visibility, mapped to (type, colour, state) triples as mgo_encode maps them)."""
import numpy as np
import pytest

import product_envs
import scenarios
from oracle import oracle as O

pytestmark = pytest.mark.gpu
REW_TOL = 1e-6


def _owner(e, k):
    """the oracle env that sees with agent k's geometry (OracleEnvViews: one env per geometry)"""
    return e.envs[e.owner[k]] if isinstance(e, O.OracleEnvViews) else e


def oracle_views(e):
    """[n] arrays (V_k, V_k, 3): agent k's gen_obs_grid -> encode on oracle env `e`"""
    base = _owner(e, 0)
    cfg, n = base.cfg, base.n
    tab = np.zeros((1000 + 32, 3), np.uint8)   # top code -> triple (mgo_encode: objects below 1000, agents from 1000)
    for o in range(1, cfg.n_obj):
        tab[o] = (cfg.obj[o].type_idx, cfg.obj[o].color_idx, cfg.obj[o].state)
    dirs = base.state()["dir"]
    for x in range(n):
        tab[1000 + x] = (cfg.agent_type_idx, cfg.agent_color_idx[x], dirs[x])
    out = []
    for k in range(n):
        vis, cells = _owner(e, k).view(k)
        out.append(np.where(vis[..., None], tab[cells], 0).astype(np.uint8))
    return out


def _per_agent(obs, n):
    """the product's return value as a list of n (B, V, V, 3) arrays (tensor, per-agent list, or rich dicts)"""
    if isinstance(obs, list):
        return [(o["pov"] if isinstance(o, dict) else o).cpu().numpy() for o in obs]
    a = obs.cpu().numpy()
    return [a[:, k] for k in range(n)]


def _check(obs, orcs, n, what):
    got = _per_agent(obs, n)
    want = [oracle_views(o) for o in orcs]
    for k in range(n):
        w = np.stack([v[k] for v in want])
        assert got[k].shape == w.shape, (what, k, got[k].shape, w.shape)
        bad = np.argwhere((got[k] != w).any(axis=(1, 2, 3)))
        assert bad.size == 0, (what, k, "envs", bad[:8].ravel().tolist())


# (scenario, batch, steps): stacks, hide_item_types, spawn_delay, respawn, see-through, view offsets, agents with their
# own views, views 3 ... 31, 24 agents, many kinds, a grid read in place, rich agents
CASES = [
    ("MarlGrid-3AgentCluttered15x15-v0", 48, 60),
    ("Test-4AgentEmpty5x5-crowded", 48, 60),
    ("Test-4AgentEmpty5x5-hide", 48, 60),
    ("Test-3AgentCluttered9x9-hide", 48, 60),
    ("Test-3AgentEmpty7x7-spawn-delay", 48, 60),
    ("Test-3AgentCluttered9x9-respawn", 48, 60),
    ("Test-2AgentEmpty7x7-see-through", 48, 60),
    ("Edge-5AgentEmpty9x9-tile5-offset3", 48, 60),
    ("Test-3AgentCluttered9x9-hetero-views", 48, 60),
    ("Test-3AgentEmpty7x7-rich", 32, 50),
    ("Edge-12AgentCluttered9x9-view3", 32, 40),
    ("Edge-3AgentCluttered11x11-view4-tile5", 32, 40),
    ("Edge-3AgentCluttered11x11-view5-tile5", 32, 40),
    ("Edge-3AgentCluttered11x11-view6-tile5", 32, 40),
    ("Edge-3AgentCluttered11x11-view8-tile5", 32, 40),
    ("Edge-3AgentCluttered11x11-view9-tile5", 32, 40),
    ("Edge-3AgentCluttered15x15-view11-tile5", 32, 40),
    ("Edge-3AgentCluttered15x15-view15-tile5", 32, 40),
    ("Limit-2AgentEmpty19x19-view17-tile8", 16, 40),
    ("Limit-3AgentCluttered33x33-view31-tile4", 16, 40),
    ("Limit-24AgentEmpty20x20-view5", 16, 40),
    ("Limit-3Agent100Kinds24x24", 16, 40),
    ("Limit-3AgentCluttered200x200-hide", 8, 30),
    ("Limit-2AgentEmpty255x255-view9-ts5", 4, 30),
    ("Goalcycle-demo-solo-v0", 16, 40),
]


@pytest.mark.parametrize("name,B,steps", CASES, ids=[c[0] for c in CASES])
def test_encoded_views_vs_oracle(name, B, steps):
    import torch
    spec = scenarios.registered(name)
    seeds = 4100 + np.arange(B)
    env = product_envs.build(name, batch_size=B, seeds=seeds, auto_reset=True, obs_format="encoded")
    n = env.num_agents
    orcs = [O.make_env(spec, seed=int(s)) for s in seeds]
    _check(env.gen_obs(), orcs, n, "constructor")
    obs = env.reset()
    for o in orcs:
        o.reset()
    _check(obs, orcs, n, "reset")
    rng = np.random.RandomState(11)
    for t in range(steps):
        a = rng.randint(0, 5 if "Kinds" in name else 7, size=(B, n))     # (no toggle among 100 kinds: Box.toggle raises)
        obs, r, d, _ = env.step(torch.from_numpy(a))
        outs = [o.step(a[b]) for b, o in enumerate(orcs)]
        for b, o in enumerate(orcs):
            if outs[b][2]:
                o.reset()                       # auto-reset inside the launch: the views are the new episode's
        _check(obs, orcs, n, t)
        assert np.abs(r.cpu().numpy().astype(np.float64) - np.stack([w[1] for w in outs])).max() <= REW_TOL
        assert np.array_equal(d.cpu().numpy(), np.array([w[2] for w in outs]))
    env.check_errors()


@pytest.mark.parametrize("B,every", [(1, 1), (4097, 10), (32768, 33)])
def test_encoded_views_batch_vs_oracle(B, every):
    """one env, a batch whose last workgroup is partial, and one whole 32 768-env shard, 100 steps with auto_reset (resets
    inside the launch): the oracle steps the whole batch; every env's views are compared (at the reset and every
    `every`-th step)"""
    import torch
    name = "MarlGrid-3AgentCluttered15x15-v0"
    seeds = 9000 + np.arange(B)
    env = product_envs.build(name, batch_size=B, seeds=seeds, auto_reset=True, obs_format="encoded")
    orc = O.OracleBatch(scenarios.registered(name), seeds)
    obs = env.reset()
    orc.reset()
    _check(obs, orc.envs, 3, "reset")
    rng = np.random.RandomState(2)
    for t in range(1, 101):
        a = rng.randint(0, 7, size=(B, 3))
        obs, r, d, _ = env.step(torch.from_numpy(a))
        _, r2, d2, _ = orc.step(a, render=False, auto_reset=True)
        assert np.abs(r.cpu().numpy() - r2).max() <= REW_TOL, t
        assert np.array_equal(d.cpu().numpy(), d2), t
        if t % every == 0 or t == 100:
            _check(obs, orc.envs, 3, t)


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("name", __import__("viewenc").fixtures())
def test_reference_fixtures_replayed_on_the_product(name, fused):
    """tests/golden/viewenc_*.npz — the live reference's gen_obs_grid -> encode along committed trajectories — replayed on the
    product byte for byte: the constructor, the reset and every recorded step (a caller-side reset after done, as recorded);
    fused: the step and the views in one launch (mg_step_encode_views), else mg_step + mg_encode_views"""
    import torch
    import viewenc
    d = viewenc.load(name)
    seeds, acts = d["seeds"], d["actions"]
    S, T, n = acts.shape
    steps = list(d["steps"])
    env = product_envs.build(name, batch_size=S, seeds=seeds, obs_format="encoded", fused_step=fused)

    def check(obs, key, ki=None):
        for k, v in enumerate(_per_agent(obs, n)):
            want = d["%s_a%d" % (key, k)] if ki is None else d["%s_a%d" % (key, k)][:, ki]
            assert np.array_equal(v, want), (key, ki, k)
    check(env.gen_obs(), "ctor")
    check(env.reset(), "reset")
    for t in range(T):
        obs, _, done, _ = env.step(torch.from_numpy(acts[:, t].astype(np.int64)))
        if t in steps:
            check(obs, "step", steps.index(t))
        dn = done.cpu().numpy()
        assert np.array_equal(dn, d["reset_after"][:, t]), t
        if dn.any():
            env.reset(env_mask=done)
    env.check_errors()


def _state(env):
    env.check_errors()
    return [t.cpu().numpy().copy() for t in (env.grid_state, env.agent_state, env.mt_state, env.mt_pos, env.mt_head,
                                              env.step_count_t)]


def _run(name, B, steps, **kw):
    import torch
    env = product_envs.build(name, batch_size=B, seeds=300 + np.arange(B), auto_reset=True, **kw)
    first = env.reset()
    first = first.cpu().numpy().copy() if hasattr(first, "cpu") else None
    rng = np.random.RandomState(8)
    rows = []
    for t in range(steps):
        o, r, d, _ = env.step(torch.from_numpy(rng.randint(0, 7, size=(B, env.num_agents))))
        rows.append((o.cpu().numpy().copy() if hasattr(o, "cpu") else None, r.cpu().numpy().copy(), d.cpu().numpy().copy()))
    return env, first, rows


@pytest.mark.parametrize("name", ["MarlGrid-3AgentCluttered15x15-v0", "Test-4AgentEmpty5x5-hide"])
def test_fused_and_two_launch_paths_agree(name):
    e1, f1, a = _run(name, 257, 40, obs_format="encoded", fused_step=True)
    e2, f2, b = _run(name, 257, 40, obs_format="encoded", fused_step=False)
    assert np.array_equal(f1, f2)
    for t, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and np.array_equal(x[2], y[2]), t
    for u, v in zip(_state(e1), _state(e2)):
        assert np.array_equal(u, v)


@pytest.mark.parametrize("fused", [True, False])
def test_image_and_encoded_runs_step_identically(fused):
    """the step itself does not change with the observation format: rewards, done, canonical state and RNG"""
    name = "MarlGrid-3AgentCluttered15x15-v0"
    e1, _, a = _run(name, 300, 60, obs_format="image", fused_step=fused, place_obs=False)
    e2, _, b = _run(name, 300, 60, obs_format="encoded", fused_step=fused)
    for t, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x[1], y[1]) and np.array_equal(x[2], y[2]), t
    for u, v in zip(_state(e1), _state(e2)):
        assert np.array_equal(u, v)
    assert a[-1][0].shape == (300, 3, 56, 56, 3) and b[-1][0].shape == (300, 3, 7, 7, 3)


@pytest.mark.parametrize("name", ["MarlGrid-3AgentCluttered15x15-v0", "Test-3AgentCluttered9x9-hetero-views"])
def test_render_and_gen_obs_grid_unchanged(name):
    e1, _, _ = _run(name, 16, 20, obs_format="image", place_obs=False)
    e2, _, _ = _run(name, 16, 20, obs_format="encoded")
    assert np.array_equal(e1.render(env_ids=[0, 3, 15]).cpu().numpy(), e2.render(env_ids=[0, 3, 15]).cpu().numpy())
    for k in range(e1.num_agents):
        c1, v1 = e1.gen_obs_grid(k)
        c2, v2 = e2.gen_obs_grid(k)
        assert np.array_equal(c1.cpu().numpy(), c2.cpu().numpy()) and np.array_equal(v1.cpu().numpy(), v2.cpu().numpy())
    # the views themselves still come back encoded afterwards
    for k, v in enumerate(_per_agent(e2.gen_obs(), e2.num_agents)):
        assert v.shape[1:] == (e2.agents[k].view_size, e2.agents[k].view_size, 3)


def test_encode_in_step_and_obs_buffers_with_encoded_views():
    import torch
    env = product_envs.build("MarlGrid-3AgentCluttered15x15-v0", batch_size=64, seeds=np.arange(64), obs_format="encoded",
                             encode_in_step=True, obs_buffers=3)
    assert env.obs_placement == []
    rng = np.random.RandomState(1)
    seen = []
    for t in range(5):
        o, _, _, _ = env.step(torch.from_numpy(rng.randint(0, 7, size=(64, 3))))
        assert torch.equal(env.grid_encoding, env._encode())
        seen.append(o.data_ptr())
    assert len(set(seen[:3])) == 3 and seen[3] == seen[0]      # the ring of 3 buffer sets


def test_pipeline_with_encoded_views():
    """make(..., pipeline=2) passes obs_format to both parts: their views are those of the one big env"""
    import torch
    from marlgrid_amd.envs import make
    name, B = "MarlGrid-3AgentCluttered15x15-v0", 128
    pipe = make(name, pipeline=2, batch_size=B, seed=55, obs_format="encoded")
    one = make(name, batch_size=B, seeds=55 + np.arange(B), obs_format="encoded")
    o1 = one.reset()
    parts = pipe.reset()
    pipe.synchronize()
    assert np.array_equal(torch.cat([p.cpu() for p in parts]).numpy(), o1.cpu().numpy())
    rng = np.random.RandomState(4)
    for t in range(10):
        a = torch.from_numpy(rng.randint(0, 7, size=(B, 3)))
        o1, _, _, _ = one.step(a)
        outs = pipe.step(a)
        pipe.synchronize()
        assert np.array_equal(torch.cat([x[0].cpu() for x in outs]).numpy(), o1.cpu().numpy()), t
