"""GPU (-m gpu): obs_delta=True together with episode outputs (episode_info, auto_reset="next_step") and encode_in_step — the
launches of mg_step_render_delta_ex, render_kernel<7, 8, 16 | 4, 96 | 80 | 112, 0> — against the same env stepped with
obs_delta=False.  The twin takes mg_step_render_ep / mg_step_render_encode (or, with both, mg_step_render_ep + mg_encode), which
the whole-shard tests hold against the oracle; everything here is torch.equal, byte for byte.

1. twin envs over 120 steps at max_steps = 25 (every env truncates four times; in next-step mode each end is followed by the env's
   reset call), five option mixes, batches 1 / 67 / 4 099 (4- and 16-wave workgroups, a ragged last wave), obs_buffers 1 / 2 / 3:
   observations, rewards, done, every info tensor and grid_encoding on every step — terminal observations and the reset calls
   behind them included, and counted on the twin's side;
2. the action patterns of tests/test_hip_obs_delta.py that make the ring and the masks hard;
3. every one of the six kernels DOES skip (a sentinel behind the env's back survives where nothing changed), and
   invalidate_obs() ends that;
4. a step captured into a graph sees reset() and invalidate_obs() as an eager step does;
5. make(..., pipeline=2) passes the combination to both parts;
6. the C call answers MG_E_UNSUPPORTED for a tile-5 env and launches nothing; obs_delta=True raises there at the first step;
7. the oracle differential (tests/wide_diff.py) at 4 099 envs over 220 steps, next-step mode with episode_info, staggered resets,
   without and with encode_in_step.  Its seeds are 444200 + env index (wide_diff.SEED0 + 20000): with SEED0 itself (and the four
   bases between) the CPU oracle alone sees no episode TERMINATE within 220 steps of these actions — with 444200, env 3660 does,
   at step 92."""
import ctypes as C

import numpy as np
import pytest
import torch

import wide_diff
from marlgrid_amd import _native as N
from marlgrid_amd.envs import make

pytestmark = pytest.mark.gpu

NAME = "MarlGrid-3AgentCluttered15x15-v0"
LEFT, RIGHT, FORWARD, DONE = 0, 1, 2, 6
STEPS = 120
MAX_STEPS = 25

OPTIONS = {
    "episode_info": dict(episode_info=True),
    "next_step": dict(auto_reset="next_step"),
    "next_step+episode_info": dict(auto_reset="next_step", episode_info=True),
    "encode_in_step": dict(encode_in_step=True),
    "encode_in_step+next_step+episode_info": dict(encode_in_step=True, auto_reset="next_step", episode_info=True),
}
# the instantiation (its V) each mix runs
KERNEL_V = {"episode_info": 96, "next_step": 96, "next_step+episode_info": 96, "encode_in_step": 80,
            "encode_in_step+next_step+episode_info": 112}


def twins(B, options, **kw):
    seeds = 1337 + np.arange(B)
    kw = dict(dict(auto_reset=True, max_steps=MAX_STEPS), **dict(OPTIONS[options], **kw))
    a = make(NAME, batch_size=B, device="cuda:0", seeds=seeds, obs_delta=True, **kw)
    b = make(NAME, batch_size=B, device="cuda:0", seeds=seeds, obs_delta=False, **kw)
    assert torch.equal(a.reset(), b.reset())
    if a.encode_in_step:
        assert torch.equal(a.grid_encoding, b.grid_encoding)
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
    """one step of both; everything a step returns (and grid_encoding) is equal.  -> what the TWIN returned"""
    oa, ra, da, ia = a.step(act)
    ob, rb, db, ib = b.step(act)
    assert torch.equal(oa, ob), "obs differ " + where
    assert torch.equal(ra, rb), "rewards differ " + where
    assert torch.equal(da, db), "done differs " + where
    assert set(ia) == set(ib) and (len(ib) == 5) == b.episode_info, (sorted(ia), sorted(ib))
    for k in ib:
        assert torch.equal(ia[k], ib[k]), "info[%r] differs %s" % (k, where)
    if b.encode_in_step:
        assert torch.equal(a.grid_encoding, b.grid_encoding), "grid_encoding differs " + where
    return ob, rb, db, ib


class Coverage(object):
    """what the run went through, read off the TWIN (the reference side), accumulated on the device"""

    def __init__(self, b):
        self.b = b
        z = lambda: torch.zeros((), dtype=torch.int64, device="cuda:0")
        self.ended, self.truncated, self.reset_calls, self.terminal_steps, self.steps_after = z(), z(), z(), z(), z()
        self.prev_done = torch.zeros(b.batch_size, dtype=torch.bool, device="cuda:0")

    def add(self, done, info):
        self.ended += done.sum()
        self.terminal_steps += done.any()
        self.steps_after += self.prev_done.any()       # (next-step mode: the call after an env's end is its reset)
        if self.b.episode_info:
            self.truncated += info["truncated"].sum()
            self.reset_calls += info["reset"].sum()
            if self.b.auto_reset_mode == "next_step":
                assert torch.equal(info["reset"], self.prev_done)
        self.prev_done = done.clone()

    def check(self):
        b = self.b
        assert int(self.ended) >= b.batch_size, "not every env ended"
        if b.episode_info:
            assert int(self.truncated) >= 1
        if b.auto_reset_mode == "next_step":
            # terminal observations were compared (the steps on which some env reported done), and so were the reset calls
            # behind them
            assert int(self.terminal_steps) >= 1 and int(self.steps_after) >= 1
            if b.episode_info:
                assert int(self.reset_calls) >= 1


def run_twins(a, b, acts):
    cov = Coverage(b)
    for t in range(len(acts)):
        _, _, db, ib = step_both(a, b, acts[t], "at step %d" % t)
        cov.add(db, ib)
    assert a._delta_wanted() and a._delta_launches > 0
    assert b._delta_launches == 0
    a.check_errors()
    b.check_errors()
    cov.check()
    return cov


@pytest.mark.parametrize("obs_buffers", [1, 2, 3])
@pytest.mark.parametrize("B", [1, 67, 4099])
@pytest.mark.parametrize("options", sorted(OPTIONS))
def test_twin_envs(options, B, obs_buffers):
    a, b = twins(B, options, obs_buffers=obs_buffers)
    run_twins(a, b, actions("uniform", B, a.num_agents, STEPS))
    assert a._delta_launches == STEPS


@pytest.mark.parametrize("kind", ["done", "leftright", "moving"])
def test_twin_envs_action_patterns(kind):
    a, b = twins(67, "next_step+episode_info", obs_buffers=2)
    run_twins(a, b, actions(kind, 67, a.num_agents, STEPS))


def bands(obs):
    """(B, n, P, P, 3) -> (B, n, view rows, bytes of a band)"""
    B, n, P = obs.shape[:3]
    return obs.reshape(B, n, P // 8, 8 * P * 3)


@pytest.mark.parametrize("B", [67, 4099])
@pytest.mark.parametrize("options", ["next_step+episode_info", "encode_in_step", "encode_in_step+next_step+episode_info"])
def test_each_kernel_skips_bands(options, B):
    """render_kernel<7, 8, 4 | 16, 96 | 80 | 112, 0>: a kernel that stored everything would pass every twin test"""
    a, b = twins(B, options, obs_buffers=2)
    assert KERNEL_V[options] in (96, 80, 112)
    done = actions("done", B, a.num_agents, 5)
    for t in range(2):                      # both buffer sets hold a signature
        step_both(a, b, done[t])
    nxt = a._ring[(a._ring_i + 1) % 2]["obs"]
    nxt.fill_(0xA5)                         # behind the env's back
    oa, ra, da, ia = a.step(done[2])
    ob, rb, db, ib = b.step(done[2])
    assert oa.data_ptr() == nxt.data_ptr()
    ba, bb = bands(oa), bands(ob)
    stale = (ba == 0xA5).all(dim=-1)        # (no band of a real image is 0xA5 throughout)
    assert not (bb == 0xA5).all(dim=-1).any()
    assert stale.any(), "no band was skipped"
    assert stale[:, -1, -1].any(), "the last band of the last agent was never skipped"
    assert torch.equal(ba[~stale], bb[~stale])
    assert torch.equal(ra, rb) and torch.equal(da, db)
    for k in ib:
        assert torch.equal(ia[k], ib[k]), k
    if b.encode_in_step:
        assert torch.equal(a.grid_encoding, b.grid_encoding)
    a.invalidate_obs()
    step_both(a, b, done[3], "after invalidate_obs()")
    oa = step_both(a, b, done[4], "after invalidate_obs(), the scribbled set")[0]
    assert a.obs.data_ptr() == nxt.data_ptr()
    assert a._delta_launches == 5 and b._delta_launches == 0
    a.check_errors()
    b.check_errors()


def test_captured_step_sees_invalidations():
    """warm-up, capture one step, replay; reset() — mg_render_obs into the very set the graph writes —, replay; the caller
    scribbles into the set and calls invalidate_obs(), replay: each replay equals the eager twin, info tensors included"""
    B = 67
    a, b = twins(B, "next_step+episode_info", obs_buffers=2)
    acts = actions("uniform", B, a.num_agents, 60, seed=11)
    for t in range(4):
        step_both(a, b, acts[t])
    static = acts[4].clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        oa, ra, da, ia = a.step(static)
    ended = 0

    def replay_and_compare(t, where):
        static.copy_(acts[t])
        g.replay()
        ob, rb, db, ib = b.step(acts[t])
        assert torch.equal(oa, ob), "obs differ " + where
        assert torch.equal(ra, rb) and torch.equal(da, db), where
        for k in ib:
            assert torch.equal(ia[k], ib[k]), (k, where)
        return int(db.sum())
    for t in range(5, 30):                  # (across the time limit at step 25: terminal observations and reset calls)
        ended += replay_and_compare(t, "replay %d" % t)
    assert ended >= B
    assert torch.equal(a.reset(), b.reset())
    for t in range(30, 36):
        replay_and_compare(t, "replay %d after reset()" % t)
    oa.fill_(0xA5)
    a.invalidate_obs()
    for t in range(36, 42):
        replay_and_compare(t, "replay %d after invalidate_obs()" % t)
    assert a._delta_launches > 0
    a.check_errors()


def test_pipeline_passes_the_combination():
    B, kw = 134, dict(auto_reset="next_step", episode_info=True, max_steps=MAX_STEPS)
    pipe = make(NAME, pipeline=2, batch_size=B, seed=1337, obs_delta=True, **kw)
    one = make(NAME, batch_size=B, seeds=1337 + np.arange(B), obs_delta=False, **kw)
    assert pipe.parts == 2 and all(e.obs_delta is True and e.batch_size == 67 for e in pipe.envs)
    want = one.reset()
    parts = pipe.reset()
    pipe.synchronize()
    assert torch.equal(torch.cat(parts), want)
    acts = actions("uniform", B, 3, 60, seed=21)
    ended = 0
    for t in range(60):
        torch.cuda.current_stream().synchronize()              # (ShardPipeline.step asks for ready actions)
        o, r, d, info = one.step(acts[t])
        parts = pipe.step(acts[t])
        pipe.synchronize()
        for i, w in enumerate((o, r, d)):
            assert torch.equal(torch.cat([p[i] for p in parts]), w), (t, i)
        for k in info:
            assert torch.equal(torch.cat([p[3][k] for p in parts]), info[k]), (t, k)
        ended += int(d.sum())
    assert ended >= 2 * B
    assert all(e._delta_launches == 60 for e in pipe.envs) and one._delta_launches == 0
    pipe.check_errors()
    one.check_errors()


def _tile5_env(B, **kw):
    from marlgrid_amd.envs import ClutteredMultiGrid
    agents = [dict(view_size=7, view_tile_size=5, observation_style="image", color=c) for c in ("red", "blue", "purple")]
    return ClutteredMultiGrid(agents=agents, grid_size=15, n_clutter=20, batch_size=B, device="cuda:0", seeds=1337 + np.arange(B),
                              auto_reset=True, **kw)


def test_c_call_unsupported_launches_nothing():
    B = 67
    e = _tile5_env(B, obs_delta=False, episode_info=True)
    obs0 = e.reset().clone()
    sig = torch.zeros(B * N.delta_sig_bytes(3, 7), dtype=torch.uint8, device="cuda:0")
    enc = torch.full((B, 15, 15, 3), 0xA5, dtype=torch.uint8, device="cuda:0")
    act = actions("uniform", B, 3, 1)[0].contiguous()
    state = [t.clone() for t in (e.grid_state, e.agent_state, e.step_count_t, e.mt_pos, e.mt_head, e.done_t, e.rewards)]
    ep = e._ring[0]["ep"]
    head = (C.byref(e._cfg), C.byref(e._state), act.data_ptr(), act.element_size(), e.rewards.data_ptr(), None, e.obs.data_ptr(),
            sig.data_ptr(), N.DELTA_FORCE)
    for extras in ((enc.data_ptr(), None), (None, C.byref(ep)), (enc.data_ptr(), C.byref(ep))):
        assert e._lib.mg_step_render_delta_ex(*head, *extras, e._stream()) == N.E_UNSUPPORTED
    torch.cuda.synchronize()
    assert torch.equal(e.obs, obs0) and not sig.any() and (enc == 0xA5).all()
    for was, now in zip(state, (e.grid_state, e.agent_state, e.step_count_t, e.mt_pos, e.mt_head, e.done_t, e.rewards)):
        assert torch.equal(was, now)
    e.check_errors()
    # ... and the env that demands it says so at its first step
    d = _tile5_env(B, obs_delta=True, episode_info=True)
    d.reset()
    with pytest.raises(NotImplementedError, match="episode outputs"):
        d.step(act)
    assert d._delta_launches == 0


@pytest.mark.parametrize("kw", [dict(fused_step=False), dict(obs_format="encoded")], ids=["two_launches", "encoded_views"])
def test_true_raises_off_the_fused_image_step(kw):
    """obs_delta=True with episode outputs is a demand: an env whose step is not the fused image launch raises at its first step"""
    e = make(NAME, batch_size=5, device="cuda:0", seeds=1337 + np.arange(5), auto_reset=True, obs_delta=True, episode_info=True, **kw)
    e.reset()
    with pytest.raises(NotImplementedError, match="fused image step"):
        e.step(actions("uniform", 5, 3, 1)[0])
    assert e._delta_launches == 0


class _CountingSubject(wide_diff.HipSubject):
    """HipSubject that also counts what the (oracle-checked) info reported"""
    terminated = truncated = reset_calls = 0

    def step(self, a):
        o, r, d, info = wide_diff.HipSubject.step(self, a)
        self.terminated += int(info["terminated"].sum())
        self.truncated += int(info["truncated"].sum())
        self.reset_calls += int(info["reset"].sum())
        return o, r, d, info


WIDE_B, WIDE_T, WIDE_SEED0 = 4099, 220, wide_diff.SEED0 + 20000


@pytest.mark.parametrize("encode", [False, True], ids=["episodes", "episodes+encode"])
def test_oracle_differential(encode):
    import product_envs
    seeds = WIDE_SEED0 + np.arange(WIDE_B)
    kw = dict(encode_in_step=True) if encode else {}
    env = product_envs.build(wide_diff.HEADLINE, batch_size=WIDE_B, seeds=seeds, obs_delta=True, auto_reset="next_step",
                             episode_info=True, **kw)
    sub = _CountingSubject(env)
    s = wide_diff.run(sub, wide_diff.HEADLINE, seeds, WIDE_T, obs_every=20, deep_every=wide_diff.DEEP_EVERY, mode="next_step",
                      episode_info=True, stagger=True)
    assert env._delta_wanted() and env._delta_launches == WIDE_T
    assert s["terminal_obs"].sum() > 0
    assert sub.terminated >= 1, "no episode terminated: the seeds no longer do what the oracle alone showed"
    assert sub.truncated >= WIDE_B and sub.reset_calls >= WIDE_B
    env.check_errors()
