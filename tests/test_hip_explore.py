"""GPU tests of the exploration maps (`MultiGridEnv(explore=True)`: env.seen / visits / new_cells / visit_count, written by
mg_explore_update behind every reset() and step()).  The scenario table of tests/explore_cases.py against tests/explore_ref.py —
the oracle's own vis masks through the reference's crop-and-rotate — at batches 1, 67 (a partial workgroup) and 4 099 (several
workgroups, a partial last one); the four tensors are compared, exactly, after reset() and after EVERY step.  Then the
contracts: checkpoints, splits, fork, lookahead, and the option off."""
import ctypes as C

import numpy as np
import pytest

import explore_cases as XC

pytestmark = pytest.mark.gpu
BATCHES = (1, 67, 4099)
MODES = {False: False, "same_step": True, "next_step": "next_step"}


class HipSubject(object):
    def __init__(self, case, B, **kw):
        self.env = case.build(batch_size=B, seeds=case.seeds(B), explore=True, auto_reset=MODES[case.mode], place_obs=False, **kw)
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
        return {k: getattr(self.env, k).cpu().numpy() for k in XC.KEYS}

    def place(self, k, x, y, d):
        self.env.set_agent(k, x=x, y=y, dir=d)


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("key", [k for k in XC.TABLE if k not in ("manual_reset", "next_step")])
def test_the_scenario_table_matches_the_reference(key, B):
    case = XC.Case(key)
    sub = HipSubject(case, B)
    ref = XC.run(case, sub, B)
    sub.env.check_errors()
    assert ref.ref.seen.any() and ref.ref.visits.any()
    if B == BATCHES[-1]:        # coverage, on the oracle's side (explore_cases.Coverage)
        assert not ref.coverage.missing(), ref.coverage.missing()
    if key == "two_groups":
        assert len(sub.env._groups) == 2 and sub.env._explore.launches == 2 * (2 + case.steps)       # (the constructor's reset)
    else:
        assert sub.env._explore.launches == 2 + case.steps


@pytest.mark.parametrize("B", (3, 67))
def test_a_launch_writes_only_its_own_agents_rows_and_selected_envs(B):
    """two view groups; sentinel-filled tensors the env never updates: the launch of group 0 leaves agent 1's rows alone, and
    a masked one the unselected envs"""
    import torch
    case = XC.Case("two_groups")
    sub = HipSubject(case, B)
    env = sub.env
    env.reset()
    assert [g.members for g in env._groups] == [[0, 2], [1]]
    dev = env.device
    seen = torch.full((B, 3, sub.W, sub.H), 0x5A, dtype=torch.uint8, device=dev)
    visits = torch.full((B, 3, sub.W, sub.H), 0x5A, dtype=torch.int32, device=dev)
    new_cells = torch.full((B, 3), 0x5A, dtype=torch.int32, device=dev)
    visit_count = torch.full((B, 3), 0x5A, dtype=torch.int32, device=dev)
    mask = torch.from_numpy((np.arange(B) % 3 != 0).astype(np.uint8)).to(dev)
    from marlgrid_amd import _native as N
    N.check(env._lib.mg_explore_update(C.byref(env._groups[0].cfg), C.byref(env._state), mask.data_ptr(), seen.data_ptr(),
                                       visits.data_ptr(), new_cells.data_ptr(), visit_count.data_ptr(), env._stream()))
    torch.cuda.synchronize()
    m = mask.bool().cpu().numpy()
    want = sub.tensors()
    for k, t in (("seen", seen), ("visits", visits), ("new_cells", new_cells), ("visit_count", visit_count)):
        t = t.cpu().numpy()
        assert (t[:, 1] == 0x5A).all() and (t[~m] == 0x5A).all(), k
        got = t[m][:, [0, 2]]
        assert np.array_equal(got.astype(bool) if k == "seen" else got, want[k][m][:, [0, 2]]), k


@pytest.mark.parametrize("B", BATCHES)
def test_a_reset_by_hand_leaves_the_other_envs_alone(B):
    """auto_reset=False with reset(env_mask=done): the unselected envs' visits are not counted twice"""
    case = XC.Case("manual_reset")
    sub = HipSubject(case, B)
    resets = []

    def after(t, done, ref):
        if not done.any():
            return False
        before = sub.tensors()
        sub.reset(done)
        ref.reset(done)
        now = sub.tensors()
        for k in XC.KEYS:
            assert np.array_equal(now[k][~done], before[k][~done]), (t, k)
        resets.append(int(done.sum()))
        return True
    XC.run(case, sub, B, after_step=after)
    assert sum(resets) >= B


@pytest.mark.parametrize("B", BATCHES)
def test_next_step_reset_accumulates_the_terminal_step_and_clears_in_the_reset_call(B):
    """auto_reset="next_step" with episode_info=True: info["reset"] marks exactly the envs whose new_cells equals their seen count"""
    case = XC.Case("next_step")
    sub = HipSubject(case, B, episode_info=True)
    n_resets = []

    def after(t, done, ref):
        t_ = sub.tensors()
        fresh = (t_["new_cells"] == t_["seen"].reshape(B, sub.n, -1).sum(axis=2)).all(axis=1)
        assert np.array_equal(sub.info["reset"].cpu().numpy(), fresh), t
        assert np.array_equal(fresh, ref.was_reset), t
        n_resets.append(int(fresh.sum()))
        return False
    XC.run(case, sub, B, after_step=after)
    assert sum(n_resets) >= 3 * B


def test_a_large_grid_with_the_largest_view():
    """255 x 255, view 31, B = 3: the planes of the last env lie past 2 * 65 025 cells, the grid is read in place"""
    case = XC.Case("large")
    sub = HipSubject(case, 3)
    ref = XC.run(case, sub, 3)
    assert ref.ref.seen.reshape(3, 2, -1).sum(axis=2).min() >= 1 and ref.ref.visits.reshape(3, 2, -1).sum(axis=2).min() == 11


# ---- contracts -----------------------------------------------------------------------------------------------------------
S15 = XC.S15


def _make(B=67, **kw):
    from marlgrid_amd.envs import make
    return make(S15, batch_size=B, seed=900, place_obs=False, **kw)


def _actions(rng, B, n=3):
    import torch
    return torch.from_numpy(rng.randint(0, 7, size=(B, n)))


def _maps(env):
    return [getattr(env, k).clone() for k in XC.KEYS]


def _same(a, b):
    import torch
    return all(torch.equal(x.cpu(), y.cpu()) for x, y in zip(a, b))


def test_a_checkpoint_carries_the_maps():
    import torch
    rng = np.random.RandomState(3)
    env = _make(explore=True, auto_reset=True, max_steps=9)
    for _ in range(12):
        env.step(_actions(rng, 67))
    sd = env.state_dict()
    assert sd["seen"].dtype == torch.bool and sd["visits"].dtype == torch.int32
    twin = _make(explore=True, auto_reset=True, max_steps=9)
    twin.load_state_dict(sd)
    assert _same(_maps(env)[:2], _maps(twin)[:2])
    for _ in range(10):
        a = _actions(rng, 67)
        env.step(a)
        twin.step(a)
        assert _same(_maps(env), _maps(twin))
    # a checkpoint without the maps loads with cleared maps
    bare = {k: v for k, v in sd.items() if k not in ("seen", "visits")}
    twin.load_state_dict(bare)
    assert not twin.seen.any() and not twin.visits.any()
    with pytest.raises(KeyError):
        _make(explore=False).load_state_dict(sd)


@pytest.mark.parametrize("split", ["pipeline", "devices"])
def test_a_checkpoint_round_trips_across_splits(split):
    import torch
    rng = np.random.RandomState(4)
    B = 66
    one = _make(B, explore=True, auto_reset=True, max_steps=9)
    parts = _make(B, explore=True, auto_reset=True, max_steps=9, **({"pipeline": 2} if split == "pipeline" else {"devices": [0, 0]}))
    for _ in range(12):
        a = _actions(rng, B)
        one.step(a)
        parts.step(a)
    torch.cuda.synchronize()
    for k in XC.KEYS:
        assert torch.equal(torch.cat([t.cpu() for t in getattr(parts, k)]), getattr(one, k).cpu()), k
    sd = parts.state_dict()
    assert torch.equal(sd["seen"], one.seen.cpu()) and torch.equal(sd["visits"], one.visits.cpu())
    fresh = _make(B, explore=True, auto_reset=True, max_steps=9)
    fresh.load_state_dict(sd)
    other = _make(B, explore=True, auto_reset=True, max_steps=9, pipeline=3)
    other.load_state_dict(one.state_dict())
    for _ in range(10):
        a = _actions(rng, B)
        one.step(a)
        fresh.step(a)
        other.step(a)
    torch.cuda.synchronize()
    assert _same(_maps(one), _maps(fresh))
    for k in XC.KEYS:
        assert torch.equal(torch.cat([t.cpu() for t in getattr(other, k)]), getattr(one, k).cpu()), k


def test_fork_copies_the_rows_and_an_outside_id_copies_nothing():
    import torch
    rng = np.random.RandomState(5)
    env = _make(explore=True)
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
    dev = env.device
    env.fork(torch.tensor([5, 6, 67], device=dev), torch.tensor([67, -1, 7], device=dev))      # every pair names an id outside
    assert _same(now, _maps(env))
    env.fork(torch.tensor([5, 67], device=dev), torch.tensor([20, 21], device=dev))
    after = _maps(env)
    for b, t in zip(now, after):
        assert torch.equal(t[20], b[5]) and torch.equal(t[21], b[21])


def test_lookahead_leaves_the_maps_alone():
    import torch
    rng = np.random.RandomState(6)
    env = _make(explore=True)
    for _ in range(5):
        env.step(_actions(rng, 67))
    before = _maps(env)
    launches = env._explore.launches
    env.lookahead(torch.from_numpy(rng.randint(0, 7, size=(2, 6, 67, 3))).to(env.device))
    torch.cuda.synchronize()
    assert _same(before, _maps(env)) and env._explore.launches == launches


def test_the_option_changes_nothing_else():
    """twin envs with explore on and off: observations, rewards, done, state and RNG for 50 steps, and the kernel's name"""
    import torch
    rng = np.random.RandomState(7)
    on, off = _make(explore=True, auto_reset=True), _make(explore=False, auto_reset=True)
    assert on.kernel_name == off.kernel_name
    assert off._explore is None and off.seen is None and off.visits is None and off.new_cells is None and off.visit_count is None
    assert not any(k in off.state_dict() for k in ("seen", "visits"))
    assert torch.equal(on.reset(), off.reset())
    for t in range(50):
        a = _actions(rng, 67)
        o1, r1, d1, i1 = on.step(a)
        o2, r2, d2, i2 = off.step(a)
        assert torch.equal(o1, o2) and torch.equal(r1, r2) and torch.equal(d1, d2) and i1 == i2 == {}, t
    s1, s2 = on.state_dict(), off.state_dict()
    assert set(s1) - set(s2) == {"seen", "visits"}
    for k in s2:
        assert torch.equal(s1[k], s2[k]), k
    assert on.kernel_name == off.kernel_name
