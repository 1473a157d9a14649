"""GPU (-m gpu): obs_delta — the step launch that does not store the observation bands whose tiles are the ones its output
buffer was drawn from (mg_step_render_delta) — against the same env stepped without it.  The twin (obs_delta=False) is the
plain launch the whole-shard tests hold against the oracle; everything here is torch.equal, byte for byte.

1. twin envs over 230 steps (two whole-batch resets at max_steps = 100), batches 1 / 67 / 4 099 (one env; ragged runs and
   partial staged batches on 4-wave workgroups; 16-wave workgroups), obs_buffers 1 / 2 / 3, four action streams;
2. bands ARE skipped (a sentinel behind the env's back survives where nothing changed) and invalidate_obs() ends that;
3. every other writer of a ring buffer invalidates;
4. shapes without the instantiation fall back under "auto", and the C call says MG_E_UNSUPPORTED for them;
5. one- and two-agent envs (the only shapes whose stream does not end on a four-trip block: the raster's single trips);
6. a step captured into a graph and replayed sees reset() and invalidate_obs() as an eager step does."""
import ctypes as C

import numpy as np
import pytest
import torch

from marlgrid_amd import _native as N
from marlgrid_amd.envs import make

pytestmark = pytest.mark.gpu

NAME = "MarlGrid-3AgentCluttered15x15-v0"
LEFT, RIGHT, FORWARD, DONE = 0, 1, 2, 6
STEPS = 230


def twins(B, name=NAME, **kw):
    seeds = 1337 + np.arange(B)
    a = make(name, batch_size=B, device="cuda:0", seeds=seeds, auto_reset=True, obs_delta=True, **kw)
    b = make(name, batch_size=B, device="cuda:0", seeds=seeds, auto_reset=True, obs_delta=False, **kw)
    assert torch.equal(a.reset(), b.reset())
    return a, b


def actions(kind, B, n, steps, seed=0):
    """(steps, B, n) int64 on the device"""
    g = torch.Generator().manual_seed(seed)
    if kind == "uniform":
        a = torch.randint(0, 7, (steps, B, n), generator=g)
    elif kind == "done":                   # nothing changes between steps
        a = torch.full((steps, B, n), DONE)
    elif kind == "leftright":              # the image of two steps ago, not that of one step ago: the ring trap
        a = torch.empty((steps, B, n), dtype=torch.int64)
        a[0::2] = LEFT
        a[1::2] = RIGHT
    elif kind == "moving":                 # every agent turns or walks, every step
        a = torch.tensor([LEFT, RIGHT, FORWARD])[torch.randint(0, 3, (steps, B, n), generator=g)]
    else:
        raise KeyError(kind)
    return a.to("cuda:0")


def step_both(a, b, act, where=""):
    oa, ra, da, _ = a.step(act)
    ob, rb, db, _ = b.step(act)
    assert torch.equal(oa, ob), "obs differ " + where
    assert torch.equal(ra, rb), "rewards differ " + where
    assert torch.equal(da, db), "done differs " + where
    return oa, ob


def used_delta(env):
    """the env's steps were mg_step_render_delta launches (whether they skipped anything: the sentinel tests)"""
    return env._delta_wanted() and env._delta_launches > 0


@pytest.mark.parametrize("kind", ["uniform", "done", "leftright", "moving"])
@pytest.mark.parametrize("obs_buffers", [1, 2, 3])
@pytest.mark.parametrize("B", [1, 67, 4099])
def test_twin_envs(B, obs_buffers, kind):
    a, b = twins(B, obs_buffers=obs_buffers)
    acts = actions(kind, B, a.num_agents, STEPS)
    for t in range(STEPS):
        step_both(a, b, acts[t], "at step %d" % t)
    assert used_delta(a) and not used_delta(b)
    a.check_errors()
    b.check_errors()


@pytest.mark.parametrize("name,B", [("MarlGrid-2AgentEmpty9x9-v0", 67), ("MarlGrid-2AgentEmpty9x9-v0", 4099),
                                    ("Goalcycle-demo-solo-v0", 67)])
def test_twin_envs_one_and_two_agents(name, B):
    """588 / 1 176 chunks per env: 2 / 4 four-trip blocks and 2 / 3 single trips with the per-lane predicate"""
    a, b = twins(B, name=name, obs_buffers=2)
    assert a.view_size == 7 and a.tile_size == 8 and a.num_agents in (1, 2)
    acts = actions("uniform", B, a.num_agents, STEPS, seed=7)
    for t in range(STEPS):
        step_both(a, b, acts[t], "at step %d" % t)
    assert used_delta(a)
    # ... and the single trips do skip: all-`done` actions into a sentinel-filled set leave every band untouched
    done = actions("done", B, a.num_agents, 4)
    for t in range(2):
        step_both(a, b, done[t])
    nxt = a._ring[(a._ring_i + 1) % 2]["obs"]
    nxt.fill_(0xA5)
    oa = a.step(done[2])[0]
    ob = b.step(done[2])[0]
    stale = (bands(oa) == 0xA5).all(dim=-1)
    assert stale[:, -1, -1].any(), "the last band — a single trip — was never skipped"
    assert torch.equal(bands(oa)[~stale], bands(ob)[~stale])
    a.invalidate_obs()
    step_both(a, b, done[3])
    step_both(a, b, done[3])
    a.check_errors()


def test_captured_step_sees_invalidations():
    """warm-up (every set's signature valid), capture one step, replay; reset() — mg_render_obs into the very set the graph
    writes —, replay; the caller scribbles into the set and calls invalidate_obs(), replay: each replay equals the eager twin"""
    B = 67
    a, b = twins(B, obs_buffers=2)
    acts = actions("uniform", B, a.num_agents, 40, seed=11)
    for t in range(4):
        step_both(a, b, acts[t])
    static = acts[4].clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        oa, ra, da, _ = a.step(static)

    def replay_and_compare(t, where):
        static.copy_(acts[t])
        g.replay()
        ob, rb, db, _ = b.step(acts[t])
        assert torch.equal(oa, ob), "obs differ " + where
        assert torch.equal(ra, rb) and torch.equal(da, db), where
    for t in range(5, 12):
        replay_and_compare(t, "replay %d" % t)
    assert torch.equal(a.reset(), b.reset())
    for t in range(12, 18):
        replay_and_compare(t, "replay %d after reset()" % t)
    mask = torch.zeros(B, dtype=torch.bool, device="cuda:0")
    mask[[1, 9, 65]] = True
    assert torch.equal(a.reset(env_mask=mask), b.reset(env_mask=mask))
    for t in range(18, 24):
        replay_and_compare(t, "replay %d after a masked reset" % t)
    oa.fill_(0xA5)
    a.invalidate_obs()
    for t in range(24, 30):
        replay_and_compare(t, "replay %d after invalidate_obs()" % t)
    assert used_delta(a)
    a.check_errors()


def bands(obs):
    """(B, n, P, P, 3) -> (B, n, view rows, bytes of a band)"""
    B, n, P = obs.shape[:3]
    return obs.reshape(B, n, P // 8, 8 * P * 3)


def test_bands_are_skipped_and_invalidate_obs_stores_them():
    B = 67
    a, b = twins(B, obs_buffers=2)
    done = actions("done", B, a.num_agents, 8)
    for t in range(4):                      # both buffer sets hold a signature
        step_both(a, b, done[t])
    nxt = a._ring[(a._ring_i + 1) % 2]["obs"]
    nxt.fill_(0xA5)                         # behind the env's back
    oa, ra, da, _ = a.step(done[4])
    ob, rb, db, _ = b.step(done[4])
    assert oa.data_ptr() == nxt.data_ptr()
    ba, bb = bands(oa), bands(ob)
    stale = (ba == 0xA5).all(dim=-1)        # (no band of a real image is 0xA5 throughout)
    assert not (bb == 0xA5).all(dim=-1).any()
    frac = stale.float().mean().item()
    print("\nbands skipped with all-done actions: %.3f" % frac)
    assert stale.any(), "no band was skipped"
    assert torch.equal(ba[~stale], bb[~stale])
    assert torch.equal(ra, rb) and torch.equal(da, db)
    # the other set is intact; this one is repaired by invalidate_obs()
    step_both(a, b, done[5])
    a.invalidate_obs()
    oa, ob = step_both(a, b, done[6])
    assert oa.data_ptr() == nxt.data_ptr()
    step_both(a, b, done[7])


@pytest.mark.parametrize("path", ["masked_reset", "put_obj", "registry", "place_obs_buffers", "state_dict"])
def test_invalidation_paths(path):
    B = 67
    a, b = twins(B, obs_buffers=2)
    acts = actions("uniform", B, a.num_agents, 24, seed=3)
    for t in range(8):
        step_both(a, b, acts[t])
    if path == "masked_reset":
        mask = torch.zeros(B, dtype=torch.bool, device="cuda:0")
        mask[[0, 5, 66]] = True
        assert torch.equal(a.reset(env_mask=mask), b.reset(env_mask=mask))
    elif path == "put_obj":
        # (on the border, where no agent can stand: put_obj on an agent's cell evicts it, and its next move raises as upstream)
        from marlgrid_amd.objects import Goal
        for e in (a, b):
            v = e.obj_reg.version
            e.put_obj(Goal(color="green", reward=1), 0, 7)          # the scenario's own goal kind: the tables stay
            assert e.obj_reg.version == v
    elif path == "registry":
        from marlgrid_amd.objects import Wall
        for e in (a, b):
            v = e.obj_reg.version
            e.put_obj(Wall(color="red"), 0, 3)                      # a kind the registry has not seen: new object table and atlas
            assert e.obj_reg.version != v
    elif path == "place_obs_buffers":
        for e in (a, b):
            e._place_obs_buffers(min_bytes=1, seconds=0.2)
    elif path == "state_dict":
        for e in (a, b):
            sd = e.state_dict()
            e.step(acts[23])
            e.load_state_dict(sd)
    for t in range(8, 20):
        step_both(a, b, acts[t], "after %s, step %d" % (path, t))
    assert used_delta(a)


def _unsupported_cases():
    return [
        ("tile5", "MarlGrid-3AgentCluttered15x15-v0", dict(), dict(view_tile_size=5)),
        ("prestige", "MarlGrid-3AgentCluttered15x15-v0", dict(), dict(color="prestige")),
        ("episode_info", NAME, dict(episode_info=True), None),
        ("encode_in_step", NAME, dict(encode_in_step=True), None),
    ]


@pytest.mark.parametrize("case", [c[0] for c in _unsupported_cases()])
def test_unsupported_shapes_fall_back(case):
    _, name, kw, agent_kw = next(c for c in _unsupported_cases() if c[0] == case)
    B = 67
    seeds = 1337 + np.arange(B)

    def build(obs_delta):
        if agent_kw is None:
            return make(name, batch_size=B, device="cuda:0", seeds=seeds, auto_reset=True, obs_delta=obs_delta, **kw)
        from marlgrid_amd.envs import ClutteredMultiGrid
        agents = [dict(view_size=7, view_tile_size=8, observation_style="image", color=c) for c in ("red", "blue", "purple")]
        agents[0].update(agent_kw)
        if "view_tile_size" in agent_kw:
            for g in agents:
                g.update(agent_kw)
        return ClutteredMultiGrid(agents=agents, grid_size=15, n_clutter=20, batch_size=B, device="cuda:0", seeds=seeds,
                                  auto_reset=True, obs_delta=obs_delta, **kw)
    a, b = build("auto"), build(False)
    assert torch.equal(a.reset(), b.reset())
    acts = actions("uniform", B, a.num_agents, 12, seed=5)
    for t in range(12):
        step_both(a, b, acts[t], "%s step %d" % (case, t))
    assert not used_delta(a)
    if agent_kw is not None:
        # the C call itself: nothing launched, MG_E_UNSUPPORTED
        sig = torch.zeros(B * N.delta_sig_bytes(a.num_agents, a.view_size), dtype=torch.uint8, device="cuda:0")
        act = acts[0].contiguous()
        rc = a._lib.mg_step_render_delta(C.byref(a._cfg), C.byref(a._state), act.data_ptr(), act.element_size(), a.rewards.data_ptr(),
                                         None, a.obs.data_ptr(), sig.data_ptr(), N.DELTA_FORCE, a._stream())
        assert rc == N.E_UNSUPPORTED
        assert not a._delta_ok                  # ... which is what "auto" heard
    a.check_errors()
