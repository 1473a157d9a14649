"""GPU (-m gpu): every kind of step launch the library accepts at view 7 with 8-pixel tiles (marlgrid_amd/step_launch.py) against
a twin built with fused_step=False, obs_delta=False — mg_step[_ep], one views launch, mg_encode behind them — and the same seeds
and actions: observations, rewards, done, every info tensor and grid_encoding are torch.equal on every step, and the kind the
plan remembered is the expected one.  70 envs: more than the 64 lanes of mg_step's workgroup, no multiple of the 8-env staged
batch; max_steps=8 over 24 steps: every env resets inside a launch three times.  (The `specialize` kinds: tests/test_hip_specialize.py.)"""
import numpy as np
import pytest
import torch

from marlgrid_amd import step_launch as SL
from marlgrid_amd.envs import ClutteredMultiGrid, make

pytestmark = pytest.mark.gpu

NAME = "MarlGrid-3AgentCluttered15x15-v0"
B, STEPS, MAX_STEPS = 70, 24, 8

CASES = {
    "delta": (dict(obs_delta="auto"), SL.DELTA),
    "delta_ex_episode": (dict(obs_delta=True, episode_info=True), SL.DELTA_EX_EP),
    "delta_ex_encode": (dict(obs_delta=True, encode_in_step=True), SL.DELTA_EX_ENCODE),
    "delta_ex_both": (dict(obs_delta=True, episode_info=True, encode_in_step=True), SL.DELTA_EX_BOTH),
    "render": (dict(obs_delta=False), SL.RENDER),
    "render_encode": (dict(obs_delta="auto", encode_in_step=True), SL.RENDER_ENCODE),
    "render_ep": (dict(obs_delta="auto", episode_info=True), SL.RENDER_EP),
    "encode_views": (dict(obs_format="encoded"), SL.ENCODE_VIEWS),
    "encode_views_ep": (dict(obs_format="encoded", episode_info=True), SL.ENCODE_VIEWS_EP),
    "two_launches": (dict(fused_step=False, encode_in_step=True), SL.TWO),
}


def run_against_twin(build, kw, kind):
    env = build(**kw)
    twin = build(**dict(kw, fused_step=False, obs_delta=False))
    assert torch.equal(env.reset(), twin.reset())
    assert env._plan.chosen is None and not env._plan.refused
    acts = torch.randint(0, 7, (STEPS, B, env.num_agents), generator=torch.Generator().manual_seed(3)).to("cuda:0")
    ends = torch.zeros(B, dtype=torch.int64, device="cuda:0")
    for t in range(STEPS):
        o, r, d, i = env.step(acts[t])
        o2, r2, d2, i2 = twin.step(acts[t])
        assert torch.equal(o, o2) and torch.equal(r, r2) and torch.equal(d, d2), t
        assert set(i) == set(i2) and (len(i2) == 5) == env.episode_info, (sorted(i), sorted(i2))
        for k in i2:
            assert torch.equal(i[k], i2[k]), (k, t)
        if env.encode_in_step:
            assert torch.equal(env.grid_encoding, twin.grid_encoding) and torch.equal(twin.grid_encoding, twin.grid.encode()), t
        ends += d2
        assert env._plan.chosen[0] is kind, (t, env._plan.chosen[0])
    env.check_errors()
    twin.check_errors()
    assert int(ends.min()) >= 2, "an env did not reset twice"
    assert twin._plan.chosen[0] is (SL.TWO_EP if env.episode_info else SL.TWO) and twin._delta_launches == 0
    assert env._delta_launches == (STEPS if kind.latch == "delta" else 0)
    return env


@pytest.mark.parametrize("case", sorted(CASES))
def test_kind_equals_two_launches(case):
    kw, kind = CASES[case]
    seeds = 1337 + np.arange(B)
    env = run_against_twin(lambda **k: make(NAME, batch_size=B, device="cuda:0", seeds=seeds, auto_reset=True, max_steps=MAX_STEPS, **k),
                           kw, kind)
    assert not env._plan.refused and env._enc_fused and env._ep_fused and env._delta_ok == (kw.get("obs_delta") is not False)


def test_refused_delta_is_the_plain_render():
    """view 7 at 5-pixel tiles: the library has no delta instantiation — "auto" hears the refusal in its first step, which is
    mg_step_render, and keeps it"""
    seeds = 1337 + np.arange(B)
    agents = [dict(view_size=7, view_tile_size=5, observation_style="image", color=c) for c in ("red", "blue", "purple")]
    env = run_against_twin(lambda **k: ClutteredMultiGrid(agents=agents, grid_size=15, n_clutter=20, batch_size=B, device="cuda:0",
                                                          seeds=seeds, auto_reset=True, max_steps=MAX_STEPS, **k),
                           dict(obs_delta="auto"), SL.RENDER)
    assert env._plan.refused == {"delta"} and not env._delta_ok and not env._delta_wanted()
    assert all(r["sig"] is None for r in env._ring)
