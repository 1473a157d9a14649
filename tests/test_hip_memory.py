"""GPU tests of the memory maps (`MultiGridEnv(memory=True)`: env.memory / env.seen_step beside the four exploration tensors, all
written by ONE mg_memory_update launch per view group behind every reset() and step()).  The scenario table of
tests/memory_cases.py against tests/memory_ref.py — the oracle's post-hide top codes and vis masks through the reference's
crop-and-rotate — at batches 1, 67 (3 x 67 pairs: less than one 256-pair workgroup) and 171 (513 pairs: three workgroups, the
last partial, envs straddling a workgroup boundary); the six tensors are compared, exactly, after reset() and after EVERY step,
with the invariants between them.  Then `headline` at 4 099 envs, the 255 x 255 grid, the sentinels, the reset drivers, a
product-only cross-check against obs_format="encoded", and the contracts: checkpoints, splits, fork, lookahead, the option off."""
import ctypes as C

import numpy as np
import pytest

import explore_ref as XR
import memory_cases as MC

pytestmark = pytest.mark.gpu
BATCHES = (1, 67, 171)
MODES = {False: False, "same_step": True, "next_step": "next_step"}
# doorkey under the driver's seeds and action stream: at 67 envs no door is ever unlocked, at 171 one opens in full view of
# both agents — the oracle's grids say so, whatever the subject does (memory_ref's counts: 0 and 0).  A remembered door that
# differs from the door is met 11 times at this batch (29 at 1 027, 173 at 2 051), so doorkey's condition (b) is asserted in a
# run of its own there; doorkey_colored meets it in the table, 32 times at 67 envs and 7 times at 171
DOORKEY_STALE_B = 515


class HipSubject(object):
    def __init__(self, case, B, **kw):
        self.env = case.build(batch_size=B, seeds=case.seeds(B), memory=True, auto_reset=MODES[case.mode], place_obs=False, **kw)
        self.W, self.H, self.n = self.env.width, self.env.height, self.env.num_agents
        self.info = {}

    def reset(self, mask=None):
        import torch
        self.env.reset() if mask is None else self.env.reset(env_mask=torch.from_numpy(np.asarray(mask, bool)))

    def step(self, a):
        import torch
        _, _, done, self.info = self.env.step(torch.from_numpy(a))
        return done.cpu().numpy()

    def tensors(self):
        return {k: getattr(self.env, k).cpu().numpy() for k in MC.KEYS}

    def place(self, k, x, y, d):
        self.env.set_agent(k, x=x, y=y, dir=d)


def _launches(sub, case, steps):
    groups = len(sub.env._groups)
    assert sub.env._explore.launches == groups * (2 + steps)       # (the constructor's reset, run's reset, the steps)


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("key", [k for k in MC.TABLE if k not in ("manual_reset", "next_step")])
def test_the_scenario_table_matches_the_reference(key, B):
    case = MC.Case(key)
    sub = HipSubject(case, B)
    assert sub.env.explore is True and sub.env.memory.shape == (B, sub.n, sub.W, sub.H, 4)
    ref = MC.run(case, sub, B)
    sub.env.check_errors()
    assert ref.ref.memory.any() and (ref.ref.seen_step > 0).any()
    _launches(sub, case, case.steps)
    if B >= 67:        # coverage, on the reference's side
        MC.assert_coverage(case, ref, B, doors=key != "doorkey")       # (doorkey's (b): see DOORKEY_STALE_B)


def test_doorkey_remembers_a_door_that_has_changed_since():
    """doorkey's condition (b), at a batch of the driver's seeds that meets it: 1 545 pairs, seven workgroups"""
    case = MC.Case("doorkey")
    sub = HipSubject(case, DOORKEY_STALE_B)
    ref = MC.run(case, sub, DOORKEY_STALE_B)
    MC.assert_coverage(case, ref, DOORKEY_STALE_B)


def test_headline_at_4099_envs_clears_three_times():
    """24 steps at max_steps 7: three episodes and three clears per env, 12 297 pairs in 49 workgroups"""
    case = MC.Case("headline")
    sub = HipSubject(case, 4099)
    ref = MC.run(case, sub, 4099, steps=24)
    assert ref.ref.stats["clears"] >= 3 * 4099
    MC.assert_coverage(case, ref, 4099)


def test_a_large_grid_with_the_largest_view():
    """255 x 255, view 31, B = 2: the second env's planes start past 2 x 65 025 cells (260 100 bytes into `memory` per pair),
    the run-time view, the grid read in place"""
    case = MC.Case("large")
    sub = HipSubject(case, 2)
    ref = MC.run(case, sub, 2)
    assert ref.ref.seen.reshape(2, 2, -1).sum(axis=2).min() >= 1 and (ref.ref.seen_step.reshape(2, 2, -1).max(axis=2) == 10).all()


@pytest.mark.parametrize("B", (3, 67))
def test_a_launch_writes_only_its_own_agents_rows_and_selected_envs(B):
    """two view groups; sentinel-filled tensors the env never updates: the launch of group 0 leaves agent 1's rows alone, and a
    masked one the unselected envs"""
    import torch
    from marlgrid_amd import _native as N
    case = MC.Case("two_groups")
    sub = HipSubject(case, B)
    env = sub.env
    env.reset()
    assert [g.members for g in env._groups] == [[0, 2], [1]]
    dev = env.device
    shape = (B, 3, sub.W, sub.H)
    mine = dict(seen=torch.full(shape, 0x5A, dtype=torch.uint8, device=dev), visits=torch.full(shape, 0x5A, dtype=torch.int32, device=dev),
                new_cells=torch.full((B, 3), 0x5A, dtype=torch.int32, device=dev),
                visit_count=torch.full((B, 3), 0x5A, dtype=torch.int32, device=dev),
                memory=torch.full(shape + (4,), 0x5A, dtype=torch.uint8, device=dev),
                seen_step=torch.full(shape, 0x5A, dtype=torch.int32, device=dev))
    mask = torch.from_numpy((np.arange(B) % 3 != 0).astype(np.uint8)).to(dev)
    N.check(env._lib.mg_memory_update(C.byref(env._groups[0].cfg), C.byref(env._state), mask.data_ptr(),
                                      *[mine[k].data_ptr() for k in MC.KEYS], env._stream()))
    torch.cuda.synchronize()
    m = mask.bool().cpu().numpy()
    want = sub.tensors()
    assert (env.step_count.cpu().numpy() == 0).all()      # (fresh envs: the selected planes were cleared, then marked)
    for k in MC.KEYS:
        t = mine[k].cpu().numpy()
        assert (t[:, 1] == 0x5A).all() and (t[~m] == 0x5A).all(), k
        got = t[m][:, [0, 2]]
        assert np.array_equal(got.astype(bool) if k == "seen" else got, want[k][m][:, [0, 2]]), k


@pytest.mark.parametrize("B", BATCHES)
def test_a_reset_by_hand_leaves_the_other_envs_alone(B):
    case = MC.Case("manual_reset")
    sub = HipSubject(case, B)
    resets = []

    def after(t, done, ref):
        if not done.any():
            return False
        before = sub.tensors()
        sub.reset(done)
        ref.reset(done)
        now = sub.tensors()
        for k in MC.KEYS:
            assert np.array_equal(now[k][~done], before[k][~done]), (t, k)
        assert (now["seen_step"][done] <= 0).all()
        resets.append(int(done.sum()))
        return True
    MC.run(case, sub, B, after_step=after)
    assert sum(resets) >= B


@pytest.mark.parametrize("B", BATCHES)
def test_next_step_reset_remembers_the_terminal_step_and_clears_in_the_reset_call(B):
    """auto_reset="next_step" with episode_info=True: info["reset"] marks exactly the envs whose stamps are all 0 or -1"""
    case = MC.Case("next_step")
    sub = HipSubject(case, B, episode_info=True)
    n_resets = []

    def after(t, done, ref):
        fresh = (sub.tensors()["seen_step"] <= 0).all(axis=(1, 2, 3))
        assert np.array_equal(sub.info["reset"].cpu().numpy(), fresh), t
        assert np.array_equal(fresh, ref.was_reset), t
        n_resets.append(int(fresh.sum()))
        return False
    MC.run(case, sub, B, after_step=after)
    assert sum(n_resets) >= 3 * B


@pytest.mark.parametrize("name", [MC.HIDE3, MC.XC.DK8])
def test_the_memory_is_what_the_encoded_observation_showed(name):
    """product only: an env with obs_format="encoded" and memory=True.  Every step, every non-zero triple of the returned
    observation equals memory[..., :3] at its world cell (explore_ref.view_cells on the downloaded positions and headings), and
    `known` and `seen_step` are right there"""
    import torch
    from marlgrid_amd import _native as N
    import product_envs
    B = 67
    env = product_envs.build(name, batch_size=B, seed=41, place_obs=False, obs_format="encoded", memory=True, auto_reset=True, max_steps=12)
    n, W, H = env.num_agents, env.width, env.height
    rng = np.random.RandomState(11)
    checked = 0
    obs = env.reset()
    for t in range(30):
        if t:
            obs = env.step(torch.from_numpy(rng.randint(0, 7, size=(B, n))))[0]
        o = obs.cpu().numpy()                                   # (B, n, vs, vs, 3)
        assert o.shape[:2] == (B, n) and o.shape[-1] == 3
        vs = o.shape[2]
        x, y, d = [env._rec_byte(i).cpu().numpy().astype(np.int64) for i in (N.AG_X, N.AG_Y, N.AG_DIR)]
        sc = env.step_count.cpu().numpy()
        mem, stamp = env.memory.cpu().numpy().reshape(B, n, W * H, 4), env.seen_step.cpu().numpy().reshape(B, n, W * H)
        for k in range(n):
            cell = XR.view_cells(x[:, k], y[:, k], d[:, k], vs, env.agents[k].view_offset, W, H)
            shown = o[:, k].any(axis=-1)
            assert (cell[shown] >= 0).all()
            b = np.broadcast_to(np.arange(B)[:, None, None], cell.shape)[shown]
            got = mem[b, k, cell[shown]]
            assert np.array_equal(got[:, :3], o[:, k][shown]) and (got[:, 3] == 1).all(), (t, k)
            assert np.array_equal(stamp[b, k, cell[shown]], sc[b]), (t, k)
            checked += int(shown.sum())
    assert checked > 30 * B * n


# ---- contracts -----------------------------------------------------------------------------------------------------------
S15 = MC.XC.S15


def _make(B=67, **kw):
    from marlgrid_amd.envs import make
    return make(S15, batch_size=B, seed=900, place_obs=False, **kw)


def _actions(rng, B, n=3):
    import torch
    return torch.from_numpy(rng.randint(0, 7, size=(B, n)))


def _maps(env):
    return [getattr(env, k).clone() for k in MC.KEYS]


def _same(a, b):
    import torch
    return all(torch.equal(x.cpu(), y.cpu()) for x, y in zip(a, b))


def _holds(env):
    seen, mem, stamp = env.seen.cpu(), env.memory.cpu(), env.seen_step.cpu()
    return bool(((mem[..., 3] == 1) == seen).all() and ((stamp >= 0) == seen).all())


def test_a_checkpoint_carries_the_maps_and_one_without_them_clears_all_six():
    import torch
    rng = np.random.RandomState(3)
    env = _make(memory=True, auto_reset=True, max_steps=9)
    for _ in range(12):
        env.step(_actions(rng, 67))
    sd = env.state_dict()
    assert sd["memory"].dtype == torch.uint8 and sd["memory"].shape == (67, 3, 15, 15, 4) and sd["seen_step"].dtype == torch.int32
    twin = _make(memory=True, auto_reset=True, max_steps=9)
    twin.load_state_dict(sd)
    for i in (0, 1, 4, 5):
        assert torch.equal(_maps(env)[i], _maps(twin)[i])
    for _ in range(10):
        a = _actions(rng, 67)
        env.step(a)
        twin.step(a)
        assert _same(_maps(env), _maps(twin))
    # they come together, or KeyError
    with pytest.raises(KeyError):
        twin.load_state_dict({k: v for k, v in sd.items() if k != "seen_step"})
    # a checkpoint without the two keys (an explore=True env's) clears all six maps: the invariants hold
    twin.load_state_dict({k: v for k, v in sd.items() if k not in ("memory", "seen_step")})
    assert not twin.seen.any() and not twin.visits.any() and not twin.memory.any() and bool((twin.seen_step == -1).all())
    assert not twin.new_cells.any() and not twin.visit_count.any() and _holds(twin)
    twin.step(_actions(rng, 67))
    assert _holds(twin) and bool(twin.seen.any())
    # ... and one without any of the four
    twin.load_state_dict({k: v for k, v in sd.items() if k not in ("memory", "seen_step", "seen", "visits")})
    assert not twin.seen.any() and not twin.memory.any() and bool((twin.seen_step == -1).all())
    # an env without the option does not take the keys, as `seen` and `visits` are treated
    with pytest.raises(KeyError):
        _make(explore=True).load_state_dict(sd)


@pytest.mark.parametrize("split", ["pipeline", "devices"])
def test_a_checkpoint_round_trips_across_splits(split):
    import torch
    rng = np.random.RandomState(4)
    B = 66
    one = _make(B, memory=True, auto_reset=True, max_steps=9)
    parts = _make(B, memory=True, auto_reset=True, max_steps=9, **({"pipeline": 2} if split == "pipeline" else {"devices": [0, 0]}))
    for _ in range(12):
        a = _actions(rng, B)
        one.step(a)
        parts.step(a)
    torch.cuda.synchronize()
    for k in MC.KEYS:
        assert torch.equal(torch.cat([t.cpu() for t in getattr(parts, k)]), getattr(one, k).cpu()), k
    sd = parts.state_dict()
    assert torch.equal(sd["memory"], one.memory.cpu()) and torch.equal(sd["seen_step"], one.seen_step.cpu())
    fresh = _make(B, memory=True, auto_reset=True, max_steps=9)
    fresh.load_state_dict(sd)
    other = _make(B, memory=True, auto_reset=True, max_steps=9, pipeline=3)
    other.load_state_dict(one.state_dict())
    for _ in range(10):
        a = _actions(rng, B)
        one.step(a)
        fresh.step(a)
        other.step(a)
    torch.cuda.synchronize()
    assert _same(_maps(one), _maps(fresh))
    for k in MC.KEYS:
        assert torch.equal(torch.cat([t.cpu() for t in getattr(other, k)]), getattr(one, k).cpu()), k


def test_fork_copies_the_rows():
    import torch
    rng = np.random.RandomState(5)
    env = _make(memory=True)
    for _ in range(8):
        env.step(_actions(rng, 67))
    before = _maps(env)
    env.fork([3, 4], [10, 66])
    now = _maps(env)
    for b, t in zip(before, now):
        assert torch.equal(t[10], b[3]) and torch.equal(t[66], b[4])
        keep = torch.ones(67, dtype=torch.bool)
        keep[[10, 66]] = False
        assert torch.equal(t[keep], b[keep])
    assert not torch.equal(before[4][10], before[4][3]) and _holds(env)


def test_lookahead_changes_no_byte():
    import torch
    rng = np.random.RandomState(6)
    env = _make(memory=True)
    for _ in range(5):
        env.step(_actions(rng, 67))
    before = _maps(env)
    launches = env._explore.launches
    env.lookahead(torch.from_numpy(rng.randint(0, 7, size=(2, 6, 67, 3))).to(env.device))
    torch.cuda.synchronize()
    assert _same(before, _maps(env)) and env._explore.launches == launches


def test_the_option_off_allocates_and_launches_nothing_new():
    """twin envs, memory=True and explore=True: the same number of launches per step, equal observations, rewards, done, state
    and exploration tensors for 50 steps; without either option every property is None"""
    import torch
    rng = np.random.RandomState(7)
    on, ex, off = _make(memory=True, auto_reset=True), _make(explore=True, auto_reset=True), _make(auto_reset=True)
    assert off.explore is False and off._explore is None and off.memory is None and off.seen_step is None and off.seen is None
    assert ex.explore is True and ex.memory is None and ex.seen_step is None and ex._explore.memory is None
    assert on.explore is True and on.kernel_name == ex.kernel_name == off.kernel_name
    assert not any(k in ex.state_dict() for k in ("memory", "seen_step"))
    assert torch.equal(on.reset(), ex.reset())
    l_on, l_ex = on._explore.launches, ex._explore.launches
    for t in range(50):
        a = _actions(rng, 67)
        o1, r1, d1, i1 = on.step(a)
        o2, r2, d2, i2 = ex.step(a)
        assert torch.equal(o1, o2) and torch.equal(r1, r2) and torch.equal(d1, d2) and i1 == i2 == {}, t
        for k in MC.XC.KEYS:
            assert torch.equal(getattr(on, k), getattr(ex, k)), (t, k)
    assert on._explore.launches - l_on == ex._explore.launches - l_ex == 50      # one launch per step (one view group), as before
    s1, s2 = on.state_dict(), ex.state_dict()
    assert set(s1) - set(s2) == {"memory", "seen_step"}
    for k in s2:
        assert torch.equal(s1[k], s2[k]), k
