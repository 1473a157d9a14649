"""GPU (-m gpu): the compact signature of the delta launch — one byte per view cell in a 64-byte slot per agent image, written
back only for the images with a changed band (marlgrid_amd/csrc/mg_step_layout.h: delta_sig_*) — held the only way a caller can
see it: an env stepped with obs_delta=True against its twin with obs_delta=False, torch.equal on every step.

1. twin envs over 12 steps at max_steps = 5: two mass resets inside the launch (steps 5 and 10), an invalidate_obs() and a
   reset(env_mask=...) in the middle; batches 1 / 67 / 4 099 (render_kernel<7, 8, 4 | 16, 64, 0>, a ragged last wave),
   obs_buffers 1 / 2 / 3;
2. the same run through render_kernel<7, 8, 16, 112, 0>: the delta launch with the episode outputs and the encode;
3. all agents `done` for four steps — no image changes, so no band is stored (a sentinel in the observation buffer, behind the
   env's back, shows that band by band; it says nothing about the signature) and no slot has a reason to be rewritten — and
   then steps that move;
4. the write-back itself, the only way it shows: ONE buffer set and left / right in turns, so the set's image alternates between
   two.  A changed image whose slot did not go back leaves the signature of the image before it, which the next step's image
   equals: its bands would be skipped and the buffer would keep the wrong picture;
5. a configuration with more than 63 tiles (Goals of eight more colours on the border), which keeps the 16-bit entries."""
import numpy as np
import pytest
import torch

from marlgrid_amd.envs import make

pytestmark = pytest.mark.gpu

NAME = "MarlGrid-3AgentCluttered15x15-v0"
LEFT, RIGHT, FORWARD, DONE = 0, 1, 2, 6
STEPS, MAX_STEPS = 12, 5


def twins(B, **kw):
    seeds = 1337 + np.arange(B)
    kw = dict(dict(auto_reset=True, max_steps=MAX_STEPS), **kw)
    a = make(NAME, batch_size=B, device="cuda:0", seeds=seeds, obs_delta=True, **kw)
    b = make(NAME, batch_size=B, device="cuda:0", seeds=seeds, obs_delta=False, **kw)
    assert torch.equal(a.reset(), b.reset())
    return a, b


def step_both(a, b, act, where):
    oa, ra, da, ia = a.step(act)
    ob, rb, db, ib = b.step(act)
    assert torch.equal(oa, ob), "obs differ " + where
    assert torch.equal(ra, rb) and torch.equal(da, db), where
    assert set(ia) == set(ib)
    for k in ib:
        assert torch.equal(ia[k], ib[k]), (k, where)
    if b.encode_in_step:
        assert torch.equal(a.grid_encoding, b.grid_encoding), "grid_encoding differs " + where
    return oa, ob, db


def run(a, b, B):
    g = torch.Generator().manual_seed(B)
    acts = torch.randint(0, 7, (STEPS, B, a.num_agents), generator=g).to("cuda:0")
    mask = (torch.arange(B) % 3 == 0).to("cuda:0")
    ended = 0
    for t in range(STEPS):
        if t == 4:
            a.invalidate_obs()
        if t == 7:
            assert torch.equal(a.reset(env_mask=mask), b.reset(env_mask=mask)), "obs differ after reset(env_mask)"
        ended += int(step_both(a, b, acts[t], "at step %d" % t)[2].sum())
    assert ended >= 2 * (B - int(mask.sum())), "two mass resets were meant to fall inside the run"
    assert a._delta_wanted() and a._delta_launches == STEPS and b._delta_launches == 0
    a.check_errors()
    b.check_errors()


@pytest.mark.parametrize("obs_buffers", [1, 2, 3])
@pytest.mark.parametrize("B", [1, 67, 4099])
def test_twin_envs(B, obs_buffers):
    a, b = twins(B, obs_buffers=obs_buffers)
    run(a, b, B)


def test_twin_envs_with_episode_outputs_and_encode():
    B = 4099
    a, b = twins(B, obs_buffers=2, encode_in_step=True, auto_reset="next_step", episode_info=True)
    assert torch.equal(a.grid_encoding, b.grid_encoding)
    run(a, b, B)


def bands(obs):
    """(B, n, P, P, 3) -> (B, n, view rows, bytes of a band)"""
    B, n, P = obs.shape[:3]
    return obs.reshape(B, n, P // 8, 8 * P * 3)


@pytest.mark.parametrize("B", [67, 4099])
def test_nothing_changes_then_a_step_that_moves(B):
    a, b = twins(B, obs_buffers=2, max_steps=1000)
    n = a.num_agents
    done = torch.full((B, n), DONE, device="cuda:0")
    for t in range(2):                      # both buffer sets hold a signature
        step_both(a, b, done, "done %d" % t)
    nxt = a._ring[(a._ring_i + 1) % 2]["obs"]
    nxt.fill_(0xA5)                         # behind the env's back
    oa = a.step(done)[0]
    ob = b.step(done)[0]
    assert oa.data_ptr() == nxt.data_ptr()
    stale = (bands(oa) == 0xA5).all(dim=-1)
    assert not (bands(ob) == 0xA5).all(dim=-1).any()      # (no band of a real image is 0xA5 throughout)
    assert stale.all(), "no image changed, yet %d bands were stored" % int((~stale).sum())
    a.invalidate_obs()
    step_both(a, b, done, "done 3, after invalidate_obs()")
    step_both(a, b, done, "done 4, the scribbled set")
    g = torch.Generator().manual_seed(5)
    for t in range(4):                      # every agent turns or walks: the slots of the images that change are rewritten
        act = torch.tensor([LEFT, RIGHT, FORWARD])[torch.randint(0, 3, (B, n), generator=g)].to("cuda:0")
        step_both(a, b, act, "moving %d" % t)
    for t in range(2):                      # ... and what they recorded is what the next unchanged steps compare against
        step_both(a, b, done, "done after moving %d" % t)
    assert a._delta_launches == 11 and b._delta_launches == 0
    a.check_errors()
    b.check_errors()


@pytest.mark.parametrize("B", [67, 4099])
def test_left_right_in_one_buffer_set(B):
    a, b = twins(B, obs_buffers=1, max_steps=1000)
    n = a.num_agents
    for t in range(12):
        act = torch.full((B, n), LEFT if t % 2 == 0 else RIGHT, device="cuda:0")
        step_both(a, b, act, "left / right %d" % t)
    assert a._delta_launches == 12 and b._delta_launches == 0
    a.check_errors()
    b.check_errors()


@pytest.mark.parametrize("B", [67, 4099])
def test_more_tiles_than_a_byte_of_codes_keeps_the_wide_layout(B):
    from marlgrid_amd.objects import Goal
    a, b = twins(B, obs_buffers=2)
    for i, c in enumerate(("orange", "blue", "cyan", "purple", "yellow", "olive", "pink", "white")):
        for e in (a, b):
            e.put_obj(Goal(color=c, reward=1), 0, 1 + i)        # (on the border, where no agent can stand)
    run(a, b, B)
    assert a._cfg.n_tiles > 63, a._cfg.n_tiles                  # 4 * n_tiles codes do not fit a byte
