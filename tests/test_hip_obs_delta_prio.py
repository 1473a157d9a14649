"""GPU (-m gpu): the delta launch's wave priorities (mg_render_kernel.h: s_setprio by the wave's progress in view groups,
delta_wave_prio) change when a wave's instructions issue and nothing else.  Twin envs as tests/test_hip_obs_delta.py builds them —
obs_delta=True against obs_delta=False, same seeds, same actions, two buffer sets —: observations, rewards and done are
byte-equal on each of 12 steps at max_steps = 5, i.e. with two in-launch resets of the whole batch among them.

Batches, by how a wave's run is divided on a 256-CU device (the priority is a function of the groups done and the groups in all):
67 — render_kernel<7, 8, 4, .>, one env per wave: one group, priority 3 throughout; 4 099 — <7, 8, 16, .>, two envs per wave:
one group; 12 289 — <7, 8, 16, .>, four envs per wave: two groups (3, then 1), and a last wave with a single env.
Once with the plain delta (<., 64, 0>), once with episode_info and encode_in_step (<., 112, 0>): there every info tensor and
grid_encoding are compared as well."""
import numpy as np
import pytest
import torch

from marlgrid_amd.envs import make

pytestmark = pytest.mark.gpu

NAME = "MarlGrid-3AgentCluttered15x15-v0"
STEPS = 12
MAX_STEPS = 5
MIXES = {"plain": dict(), "episode_info+encode_in_step": dict(episode_info=True, encode_in_step=True)}
WPB = {67: 4, 4099: 16, 12289: 16}


def twins(B, **kw):
    seeds = 1337 + np.arange(B)
    kw = dict(batch_size=B, device="cuda:0", seeds=seeds, auto_reset=True, max_steps=MAX_STEPS, obs_buffers=2, place_obs=False, **kw)
    a = make(NAME, obs_delta=True, **kw)
    b = make(NAME, obs_delta=False, **kw)
    assert torch.equal(a.reset(), b.reset())
    return a, b


@pytest.mark.parametrize("B", sorted(WPB))
@pytest.mark.parametrize("mix", sorted(MIXES))
def test_twin_envs(mix, B):
    a, b = twins(B, **MIXES[mix])
    # (the plain pick's name: the delta instantiation is that shape with V + 64 | 112 and takes its workgroup)
    assert a.kernel_name == b.kernel_name == "mg::render_kernel<7, 8, %d, 0, 0>" % WPB[B]
    g = torch.Generator().manual_seed(5)
    acts = torch.randint(0, 7, (STEPS, B, a.num_agents), generator=g).to("cuda:0")
    mass_resets = 0
    for t in range(STEPS):
        oa, ra, da, ia = a.step(acts[t])
        ob, rb, db, ib = b.step(acts[t])
        assert torch.equal(oa, ob), "obs differ at step %d" % t
        assert torch.equal(ra, rb), "rewards differ at step %d" % t
        assert torch.equal(da, db), "done differs at step %d" % t
        assert set(ia) == set(ib)
        for k in ib:
            assert torch.equal(ia[k], ib[k]), "info[%r] differs at step %d" % (k, t)
        if b.encode_in_step:
            assert torch.equal(a.grid_encoding, b.grid_encoding), "grid_encoding differs at step %d" % t
        mass_resets += int(bool(db.all()))
    assert mass_resets >= 1, "no step reset the whole batch inside its launch"
    assert a._delta_wanted() and a._delta_launches == STEPS      # every step was a delta launch
    assert b._delta_launches == 0
    a.check_errors()
    b.check_errors()
