"""GPU (-m gpu): episode boundaries under auto-reset — auto_reset="next_step" (the step that ends an episode returns the
TERMINAL observation, the env's next step() is its reset) and episode_info=True (terminated / truncated / reset flags,
episode return and length written by the step's own launch) — against the CPU oracle's independent envs sequenced the
same way (tests/episode_ref.py), pixels and encoded views, every launch path of step()."""
import numpy as np
import pytest

import episode_ref
import product_envs
import scenarios

pytestmark = pytest.mark.gpu
REW_TOL = 1e-6          # per step: tests/test_core_hostemu.py
P_ACT = [.15, .15, .5, .05, .05, .05, .05]
INFO_KEYS = {"terminated", "truncated", "episode_return", "episode_length", "reset"}


def _np_info(info):
    assert set(info.keys()) == INFO_KEYS
    out = {k: v.cpu().numpy() for k, v in info.items()}
    assert out["terminated"].dtype == out["truncated"].dtype == out["reset"].dtype == np.bool_
    assert out["episode_return"].dtype == np.float64 and out["episode_length"].dtype == np.int32
    return out


def _check_step(r, d, info, r2, d2, want, what):
    """rewards, done and every info field of one step, all envs"""
    assert np.abs(r.cpu().numpy().astype(np.float64) - r2).max() <= REW_TOL, what
    assert np.array_equal(d.cpu().numpy(), d2), what
    got = _np_info(info)
    episode_ref.assert_info(got, want, what)
    tol = REW_TOL * np.maximum(want["episode_length"], 1)[:, None]
    assert (np.abs(got["episode_return"] - want["episode_return"]) <= tol).all(), what
    return got


def _same_obs(obs, want, what):
    got = obs.cpu().numpy()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere((got != want).reshape(len(got), -1).any(axis=1))
    assert bad.size == 0, (what, "envs", bad[:8].ravel().tolist())
    return got


NEXT_STEP_CASES = ["MarlGrid-2AgentEmpty9x9-v0", "Test-4AgentEmpty5x5-crowded", "MarlGrid-3AgentCluttered15x15-v0"]


@pytest.mark.parametrize("fmt", ["image", "encoded"])
@pytest.mark.parametrize("name", NEXT_STEP_CASES)
def test_next_step_parity_and_terminal_observations(name, fmt):
    """509 envs (partial wave batches, a partial workgroup), 330 steps: rewards / done / every info field and the FULL
    observation tensor, bit-exact, every step, all envs — the observation of a step with done=True is the terminal state's,
    which a same-step env never returns.  The bench workload only ever ends by its time limit, all envs at once: there the
    first 100 steps stagger the episodes (env b is reset by hand after step b % 100, in the product and in the oracle), so
    that afterwards every step ends somebody's episode."""
    import torch
    B, T = 509, 330
    stagger = name == "MarlGrid-3AgentCluttered15x15-v0"
    seeds = 4200 + np.arange(B)
    env = product_envs.build(name, batch_size=B, seeds=seeds, place_obs=False, auto_reset="next_step", episode_info=True,
                             obs_format=fmt)
    same = product_envs.build(name, batch_size=B, seeds=seeds, place_obs=False, auto_reset="same_step", obs_format=fmt)
    assert env.auto_reset is True and env.auto_reset_mode == "next_step" and same.auto_reset_mode == "same_step"
    ref = episode_ref.EpisodeOracle(scenarios.registered(name), seeds, mode="next_step", render=fmt)
    _same_obs(env.reset(), ref.reset(), "reset")
    same.reset()
    rng = np.random.RandomState(5)
    n = env.num_agents
    steps_with_done = 0
    for t in range(T):
        a = rng.choice(7, size=(B, n), p=P_ACT)
        at = torch.from_numpy(a)
        obs, r, d, info = env.step(at)
        so, _, _, sinfo = same.step(at)
        assert sinfo == {}
        want_obs, r2, d2, want = ref.step(a)
        what = "%s %s step %d" % (name, fmt, t)
        _check_step(r, d, info, r2, d2, want, what)
        got = _same_obs(obs, want_obs, what)
        if d2.any():
            steps_with_done += 1
            assert (got != so.cpu().numpy()).any(), what       # (else nothing was shown)
        if stagger and t < 100:
            mask = (np.arange(B) % 100) == t
            _same_obs(env.reset(env_mask=torch.from_numpy(mask)), ref.reset_envs(mask), what + " (reset by hand)")
            same.reset(env_mask=torch.from_numpy(mask))
    env.check_errors()
    assert steps_with_done >= 100, steps_with_done
    assert ref.episodes.min() >= 2
    if name != "MarlGrid-3AgentCluttered15x15-v0":
        assert ref.n_terminated >= 10 and ref.n_truncated >= 10


def test_same_step_episode_info_changes_nothing_else():
    """auto_reset=True with episode_info against auto_reset=True alone, 4 096 envs, 260 steps: obs, rewards, done
    bit-identical; the info against the oracle stepped with the same-step reset (taken before its reset)"""
    import torch
    name, B, T = "MarlGrid-2AgentEmpty9x9-v0", 4096, 260
    seeds = 4200 + np.arange(B)
    env = product_envs.build(name, batch_size=B, seeds=seeds, place_obs=False, auto_reset=True, episode_info=True)
    plain = product_envs.build(name, batch_size=B, seeds=seeds, place_obs=False, auto_reset=True)
    assert env.kernel_name == plain.kernel_name
    ref = episode_ref.EpisodeOracle(scenarios.registered(name), seeds, mode="same_step")
    assert torch.equal(env.reset(), plain.reset())
    ref.reset()
    rng = np.random.RandomState(5)
    for t in range(T):
        a = rng.choice(7, size=(B, env.num_agents), p=P_ACT)
        at = torch.from_numpy(a).to(env.device)
        o1, r1, d1, info = env.step(at)
        o2, r2, d2, none = plain.step(at)
        assert none == {}
        assert torch.equal(o1, o2) and torch.equal(r1, r2) and torch.equal(d1, d2), t
        _o, rr, dd, want = ref.step(a)
        got = _check_step(r1, d1, info, rr, dd, want, "step %d" % t)
        assert not got["reset"].any()
    assert torch.equal(env.grid_state, plain.grid_state) and torch.equal(env.agent_state, plain.agent_state)
    assert ref.n_terminated >= 10 and ref.n_truncated >= 10
    env.check_errors()


def _equal_steps(e1, e2, T, seed=5):
    import torch
    rng = np.random.RandomState(seed)
    n_done = 0
    for t in range(T):
        a = torch.from_numpy(rng.choice(7, size=(e1.batch_size, e1.num_agents), p=P_ACT)).to(e1.device)
        o1, r1, d1, i1 = e1.step(a)
        o2, r2, d2, i2 = e2.step(a)
        assert torch.equal(o1, o2) and torch.equal(r1, r2) and torch.equal(d1, d2), t
        assert set(i1.keys()) == set(i2.keys()) == INFO_KEYS
        for k in i1:
            assert torch.equal(i1[k], i2[k]), (t, k)
        n_done += int(d1.sum())
    return n_done


@pytest.mark.parametrize("fmt", ["image", "encoded"])
@pytest.mark.parametrize("mode", ["next_step", "same_step"])
def test_two_launch_step_equals_fused(mode, fmt):
    name, B = "MarlGrid-2AgentEmpty9x9-v0", 333
    seeds = 4200 + np.arange(B)
    kw = dict(batch_size=B, seeds=seeds, place_obs=False, auto_reset=mode, episode_info=True, obs_format=fmt)
    fused = product_envs.build(name, **kw)
    two = product_envs.build(name, fused_step=False, **kw)
    fused.reset(), two.reset()
    assert _equal_steps(fused, two, 140) >= 100
    if fmt == "image":
        assert fused._ep_fused          # view 7, 8-pixel tiles: the step's own launch (mg_step_render_ep)


def test_next_step_without_episode_info():
    """auto_reset="next_step" alone: info == {} and the same trajectory as with episode_info"""
    import torch
    name, B = "MarlGrid-2AgentEmpty9x9-v0", 200
    seeds = 4200 + np.arange(B)
    kw = dict(batch_size=B, seeds=seeds, place_obs=False, auto_reset="next_step")
    bare = product_envs.build(name, **kw)
    full = product_envs.build(name, episode_info=True, **kw)
    bare.reset(), full.reset()
    rng = np.random.RandomState(5)
    for t in range(140):
        a = torch.from_numpy(rng.choice(7, size=(B, 2), p=P_ACT))
        o1, r1, d1, i1 = bare.step(a)
        o2, r2, d2, _ = full.step(a)
        assert i1 == {}
        assert torch.equal(o1, o2) and torch.equal(r1, r2) and torch.equal(d1, d2), t


def test_next_step_with_per_agent_views_vs_oracle():
    """agents with their own view geometry: mg_step_ep, then one raster launch per view group"""
    import torch
    name, B, T = "Test-3AgentCluttered9x9-hetero-views", 48, 140
    seeds = 4200 + np.arange(B)
    env = product_envs.build(name, batch_size=B, seeds=seeds, place_obs=False, auto_reset="next_step", episode_info=True)
    assert env._hetero
    ref = episode_ref.EpisodeOracle(scenarios.registered(name), seeds, mode="next_step", render="image", views=True)

    def same(obs, want, what):
        assert isinstance(obs, list) and len(obs) == len(want)
        for k, (g, w) in enumerate(zip(obs, want)):
            g = (g["pov"] if isinstance(g, dict) else g).cpu().numpy()
            assert g.shape == w.shape and np.array_equal(g, w), (what, k)
    same(env.reset(), ref.reset(), "reset")
    rng = np.random.RandomState(5)
    for t in range(T):
        a = rng.choice(7, size=(B, env.num_agents), p=P_ACT)
        obs, r, d, info = env.step(torch.from_numpy(a))
        want_obs, r2, d2, want = ref.step(a)
        _check_step(r, d, info, r2, d2, want, "step %d" % t)
        same(obs, want_obs, "step %d" % t)
    assert ref.episodes.min() >= 1 and ref.n_truncated + ref.n_terminated >= 48
    env.check_errors()


def test_pipeline_equals_the_one_env():
    import torch
    from marlgrid_amd.envs import make
    name, B = "MarlGrid-2AgentEmpty9x9-v0", 256
    kw = dict(batch_size=B, seed=4200, place_obs=False, auto_reset="next_step", episode_info=True)
    pipe = make(name, pipeline=2, **kw)
    one = make(name, **kw)
    assert all(e.auto_reset_mode == "next_step" and e.episode_info for e in pipe.envs)
    po, oo = pipe.reset(), one.reset()
    pipe.synchronize()
    assert torch.equal(torch.cat(po), oo)
    rng = np.random.RandomState(5)
    n_done = 0
    for t in range(140):
        a = torch.from_numpy(rng.choice(7, size=(B, 2), p=P_ACT)).to(one.device)
        torch.cuda.current_stream().synchronize()          # (the parts' streams do not wait for the stream that made `a`)
        parts = pipe.step(a)
        o, r, d, info = one.step(a)
        pipe.synchronize()
        assert torch.equal(torch.cat([p[0] for p in parts]), o) and torch.equal(torch.cat([p[1] for p in parts]), r), t
        assert torch.equal(torch.cat([p[2] for p in parts]), d), t
        for k in INFO_KEYS:
            assert torch.equal(torch.cat([p[3][k] for p in parts]), info[k]), (t, k)
        n_done += int(d.sum())
    assert n_done >= 100
    # one part alone (the double-buffered sampler's call) hands the info dict back too
    a0 = torch.zeros((B // 2, 2), dtype=torch.int64, device=one.device)
    torch.cuda.current_stream().synchronize()
    assert set(pipe.step_part(0, a0)[3].keys()) == INFO_KEYS
    pipe.check_errors()


@pytest.mark.parametrize("mode", ["next_step", "same_step"])
def test_encode_in_step_still_fills_grid_encoding(mode):
    import torch
    name, B = "MarlGrid-3AgentCluttered15x15-v0", 203
    seeds = 77 + np.arange(B)
    env = product_envs.build(name, batch_size=B, seeds=seeds, place_obs=False, auto_reset=mode, episode_info=True,
                             encode_in_step=True, max_steps=30)
    env.reset()
    assert torch.equal(env.grid_encoding, env.grid.encode())
    rng = np.random.RandomState(3)
    n_done = 0
    for t in range(130):
        o, r, d, info = env.step(torch.from_numpy(rng.randint(0, 7, size=(B, env.num_agents))))
        assert torch.equal(env.grid_encoding, env.grid.encode()), t
        n_done += int(d.sum())
    assert n_done >= 3 * B
    env.check_errors()


def test_checkpoint_between_the_terminal_step_and_its_reset():
    """state_dict() taken right after a step with done=True (next-step mode) resumes, in a fresh env, into the reset call"""
    import torch
    name, B = "MarlGrid-2AgentEmpty9x9-v0", 96
    seeds = 4200 + np.arange(B)
    kw = dict(batch_size=B, place_obs=False, auto_reset="next_step", episode_info=True)
    env = product_envs.build(name, seeds=seeds, **kw)
    env.reset()
    rng = np.random.RandomState(5)
    for t in range(400):
        a = torch.from_numpy(rng.choice(7, size=(B, 2), p=P_ACT))
        _, _, d, info = env.step(a)
        if t > 30 and int(d.sum()) >= 2:
            break
    else:
        raise AssertionError("no step ended two episodes")
    pending = d.clone()
    sd = env.state_dict()
    assert "ep_return_t" in sd and bool((sd["ep_return_t"] != 0).any())
    fresh = product_envs.build(name, seeds=900 + np.arange(B), **kw)
    fresh.load_state_dict(sd)
    rng2 = np.random.RandomState(6)
    for t in range(50):
        a = torch.from_numpy(rng2.choice(7, size=(B, 2), p=P_ACT)).to(env.device)
        o1, r1, d1, i1 = env.step(a)
        o2, r2, d2, i2 = fresh.step(a)
        if t == 0:
            assert torch.equal(i2["reset"], pending) and not bool(d2[pending].any())
        assert torch.equal(o1, o2) and torch.equal(r1, r2) and torch.equal(d1, d2), t
        for k in INFO_KEYS:
            assert torch.equal(i1[k], i2[k]), (t, k)
    # a checkpoint of an env without episode_info has no accumulator key, and the two do not mix
    plain = product_envs.build(name, seeds=seeds, batch_size=B, place_obs=False, auto_reset="next_step")
    assert "ep_return_t" not in plain.state_dict()
    with pytest.raises(KeyError):
        plain.load_state_dict(sd)


def test_manual_reset_zeroes_the_accumulators_of_the_masked_envs():
    import torch
    name, B = "MarlGrid-2AgentEmpty9x9-v0", 64
    seeds = 4200 + np.arange(B)
    env = product_envs.build(name, batch_size=B, seeds=seeds, place_obs=False, episode_info=True)      # auto_reset=False
    ref = episode_ref.EpisodeOracle(scenarios.registered(name), seeds, mode=None)
    env.reset()
    ref.reset()
    rng = np.random.RandomState(5)
    n_done = 0
    for t in range(200):
        a = rng.choice(7, size=(B, 2), p=P_ACT)
        _, r, d, info = env.step(torch.from_numpy(a))
        _o, r2, d2, want = ref.step(a)
        _check_step(r, d, info, r2, d2, want, "step %d" % t)
        if d2.any():
            n_done += int(d2.sum())
            env.reset(env_mask=d)
            for b in np.nonzero(d2)[0]:
                ref._reset_env(b)
            acc = env.ep_return_t.cpu().numpy()
            assert not acc[d2].any() and np.array_equal(acc[~d2], info["episode_return"].cpu().numpy()[~d2])
    assert n_done >= 20


def test_defaults_are_what_they_were():
    import torch
    from marlgrid_amd.envs import make
    for kw in ({}, {"auto_reset": True}):
        env = make("MarlGrid-3AgentCluttered15x15-v0", batch_size=64, place_obs=False, **kw)
        assert env.episode_info is False and env.auto_reset_mode == ("same_step" if kw else None)
        assert env.kernel_name == "mg::render_kernel<7, 8, 4, 0, 0>"
        env.reset()
        for t in range(3):
            out = env.step(torch.zeros((64, 3), dtype=torch.int64))
            assert out[3] == {}
        assert not env._use_ep and env.ep_return_t is None
    big = make("MarlGrid-3AgentCluttered15x15-v0", batch_size=4096, place_obs=False, auto_reset=True)
    assert big.kernel_name == "mg::render_kernel<7, 8, 16, 0, 0>"


def test_strict_ignores_the_action_row_of_a_reset_call():
    import torch
    name, B = "MarlGrid-2AgentEmpty9x9-v0", 64
    seeds = 4200 + np.arange(B)
    env = product_envs.build(name, batch_size=B, seeds=seeds, place_obs=False, auto_reset="next_step", episode_info=True,
                             strict=True)
    env.reset()
    rng = np.random.RandomState(5)
    for t in range(400):
        a = rng.choice(7, size=(B, 2), p=P_ACT)
        _, _, d, _ = env.step(torch.from_numpy(a))
        d = d.cpu().numpy()
        if d.any():
            break
    else:
        raise AssertionError("no episode ended")
    a = rng.choice(7, size=(B, 2), p=P_ACT)
    a[d] = 7                                    # invalid, in rows the reset call ignores
    _, r, d2, info = env.step(torch.from_numpy(a))
    env.check_errors()                          # nothing recorded
    fresh = info["reset"].cpu().numpy()
    assert np.array_equal(fresh, d) and not r.cpu().numpy()[d].any()
    a = rng.choice(7, size=(B, 2), p=P_ACT)
    a[np.nonzero(fresh)[0][0], 0] = 7           # the same value in a live row (just reset: the agent is active)
    env.step(torch.from_numpy(a))
    with pytest.raises(ValueError):
        env.check_errors()
