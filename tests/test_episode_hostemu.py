"""Episode boundaries under auto-reset, on the host: the step bodies of marlgrid_amd/csrc/mg_core.h driven with an
MgEpisode (tests/native/mg_hostemu.cpp) — next-step reset (the terminal state is returned, the env's next call is
its reset), same-step reset with the episode outputs, termination / truncation flags, episode length and return —
against the oracle's independent envs sequenced the same way (tests/episode_ref.py).  Sequentially (`step_run`) and as the
obs kernel's fused step runs (`step_begin` / `step_par_*` / `step_end` over batches of 8).
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "native"))

import canon  # noqa: E402
import episode_ref  # noqa: E402
import scenarios  # noqa: E402
from marlgrid_amd import _native as N  # noqa: E402
from marlgrid_amd import seeding  # noqa: E402

REW_TOL = 1e-6      # per step: tests/test_core_hostemu.py
P_ACT = [.15, .15, .5, .05, .05, .05, .05]

# scenario, B, T, and what the oracle alone gives through this sequencing (next-step mode): terminated, truncated, the
# fewest episodes any env finished
CASES = [
    ("MarlGrid-2AgentEmpty9x9-v0", 64, 400, 67, 176, 3),
    ("Test-4AgentEmpty5x5-crowded", 64, 300, 157, 70, 2),
    ("MarlGrid-1AgentCluttered15x15-v0", 64, 400, 33, 188, 3),
    ("Test-3AgentCluttered9x9-respawn", 48, 400, 0, 144, 3),
    ("Test-3AgentEmpty7x7-spawn-delay", 48, 300, 13, 324, 7),     # late spawns must not fire in a reset call
    ("MarlGrid-3AgentCluttered15x15-v0", 32, 400, 0, 96, 3),      # the bench workload
    ("Goalcycle-demo-solo-v0", 24, 400, 0, 72, 3),
]


def _same_state(emu, ref, what):
    st = emu.canonical()
    for b in range(emu.B):
        canon.assert_same(st[b], canon.oracle_canonical(ref.envs[b]), "%s env %d" % (what, b))
        assert seeding.same_stream(emu.numpy_rng_state(b), ref.envs[b].mt_state()), "%s env %d: RNG" % (what, b)


def _run(name, B, T, mode, par):
    import hostemu_episode
    seeds = 4200 + np.arange(B)
    emu = hostemu_episode.EpisodeEmu(name, B, seeds, mode=mode, par=par)
    ref = episode_ref.EpisodeOracle(scenarios.registered(name), seeds, mode=mode)
    emu.reset()
    ref.reset()
    rng = np.random.RandomState(5)
    own = np.zeros((B, emu.n), np.float64)          # the float64 running sum of the emulator's own float32 rewards
    for t in range(T):
        a = rng.choice(7, size=(B, emu.n), p=P_ACT)
        r, d, info = emu.step(a)
        _o, r2, d2, want = ref.step(a)
        what = "%s %s step %d" % (name, mode, t)
        assert np.abs(r.astype(np.float64) - r2).max() <= REW_TOL, what
        assert np.array_equal(d, d2), what
        episode_ref.assert_info(info, want, what)
        own = np.where(want["reset"][:, None], 0.0, own + r.astype(np.float64))
        assert np.array_equal(info["episode_return"], own), what
        tol = REW_TOL * np.maximum(want["episode_length"], 1)[:, None]
        assert (np.abs(info["episode_return"] - want["episode_return"]) <= tol).all(), what
        # the accumulator: the running sum, 0 where the launch reset the env
        cleared = want["reset"] if mode == "next_step" else d2 if mode == "same_step" else np.zeros(B, bool)
        assert np.array_equal(emu.ep_return, np.where(cleared[:, None], 0.0, own)), what
        own = np.where(cleared[:, None], 0.0, own)
        if mode is None and d.any():
            emu.reset(env_mask=d)
            emu.ep_return[d] = 0
            own[d] = 0
            for b in np.nonzero(d)[0]:
                ref._reset_env(b)
        if t % 7 == 0 or t == T - 1:
            _same_state(emu, ref, what)
    assert not emu.error.any()
    return emu, ref


@pytest.mark.parametrize("par", [False, True])
@pytest.mark.parametrize("name,B,T,n_term,n_trunc,min_eps", CASES)
def test_next_step_reset_vs_oracle(name, B, T, n_term, n_trunc, min_eps, par):
    emu, ref = _run(name, B, T, "next_step", par)
    # (the test cannot pass by never meeting an ending: what it saw is what the oracle alone gives)
    assert (ref.n_terminated, ref.n_truncated, int(ref.episodes.min())) == (n_term, n_trunc, min_eps)
    assert ref.episodes.min() >= 2
    if CASES.index((name, B, T, n_term, n_trunc, min_eps)) < 3:
        assert ref.n_terminated >= 10 and ref.n_truncated >= 10


@pytest.mark.parametrize("par", [False, True])
@pytest.mark.parametrize("name,B,T", [(c[0], c[1], c[2]) for c in CASES[:3] + CASES[3:6]])
def test_same_step_reset_episode_outputs_vs_oracle(name, B, T, par):
    emu, ref = _run(name, B, T, "same_step", par)
    assert ref.episodes.min() >= 2 and ref.n_truncated >= 10


@pytest.mark.parametrize("par", [False, True])
def test_no_auto_reset_accumulates_until_a_manual_reset(par):
    emu, ref = _run("MarlGrid-2AgentEmpty9x9-v0", 32, 250, None, par)
    assert ref.episodes.min() >= 1 and ref.n_terminated >= 5


@pytest.mark.parametrize("par", [False, True])
def test_ignored_action_row_records_no_error(par):
    """an ended env's action row is ignored altogether in next-step mode: the value 7 there is no ValueError; in a live row it is"""
    import hostemu_episode
    name, B = "MarlGrid-2AgentEmpty9x9-v0", 16
    seeds = 4200 + np.arange(B)
    emu = hostemu_episode.EpisodeEmu(name, B, seeds, mode="next_step", par=par)
    emu.reset()
    rng = np.random.RandomState(5)
    d = np.zeros(B, bool)
    for t in range(400):
        a = rng.choice(7, size=(B, emu.n), p=P_ACT)
        if d.any():
            a[d] = 7
            r, d2, info = emu.step(a)
            assert np.array_equal(info["reset"], d) and not emu.error.any() and not r[d].any() and not d2[d].any()
            break
        r, d, info = emu.step(a)
    else:
        raise AssertionError("no episode ended")
    fresh = info["reset"]                # just reset: every agent is active
    a = rng.choice(7, size=(B, emu.n), p=P_ACT)
    a[fresh, 0] = 7
    emu.step(a)
    assert (emu.error[fresh] == N.ERR_VALUE).all() and not emu.error[~fresh].any()
