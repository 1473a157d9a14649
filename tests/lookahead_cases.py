"""TEST INFRASTRUCTURE — what tests/test_lookahead_host.py (the host twin) and tests/test_hip_lookahead.py (the device) share: the
cases (scenario, batch, seeds, the prefix of real steps, the plans) and, per case, what the ORACLE says the plans return — a fresh
oracle env per (env, plan), same seed, replayed through the prefix, stepped through the plan with the freeze rule applied here:
from the first step that reports done on (or from the start, if the episode had ended) the env is not stepped again, its rewards
are 0 and done stays True.

The coverage conditions are asserted on the oracle's side alone (`Want.coverage`): a case cannot pass by exercising nothing.
Plan 0 of a `policy` case is not random: every agent follows mg_solve_distance's first action (the host build of it), so that
some env ends by termination, a key is picked up and a door opened."""
import ctypes as C
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "native"))

import canon  # noqa: E402
import product_envs  # noqa: E402
import wide_diff  # noqa: E402
from oracle import oracle as O  # noqa: E402

S15, DK8 = "MarlGrid-3AgentCluttered15x15-v0", "MarlGrid-2AgentDoorKey8x8-v0"
REW_TOL = wide_diff.REW_TOL     # the project's reward tolerance (1e-6)

# name -> scenario, batch, plans, steps, prefix of real steps, first seed; kw: constructor overrides; policy: plan 0 follows
# mg_solve_distance's policy.  Every case is held to the oracle.
CASES = {
    # 201 rows: a partial last wave, several workgroups; 268 rows
    "wide_k3": dict(name=S15, B=67, K=3, T=12, prefix=5, seed0=9100),
    "wide_k4": dict(name=S15, B=67, K=4, T=12, prefix=5, seed0=9100),
    # every row is truncated mid-rollout; env 33's agents are all within 7 actions of the goal (the seed was searched for)
    "truncated": dict(name=S15, B=67, K=3, T=12, prefix=0, seed0=87, kw=dict(max_steps=7), policy=True),
    # pickup and toggle write the shadow grid
    "doorkey": dict(name=DK8, B=33, K=4, T=24, prefix=3, seed0=5200, policy=True),
    "respawn": dict(name="Test-3AgentCluttered9x9-respawn", B=9, K=3, T=12, prefix=4, seed0=77),
    "prestige": dict(name="Test-3AgentCluttered9x9-prestige-mixed", B=9, K=3, T=12, prefix=4, seed0=78),
    "many_agents": dict(name="Limit-24AgentEmpty20x20-view5", B=5, K=2, T=6, prefix=2, seed0=79),      # iter_order in sc.ord
    "padded_stride": dict(name="Test-3AgentEmpty7x11-nonsquare", B=9, K=3, T=12, prefix=4, seed0=80),  # 77 cells in 80 bytes
}
ORACLE_CASES = sorted(CASES)


class Case(object):
    def __init__(self, key):
        c = CASES[key]
        self.key, self.name, self.B, self.K, self.T = key, c["name"], c["B"], c["K"], c["T"]
        self.kw = dict(c.get("kw", {}))
        self.seeds = c["seed0"] + np.arange(self.B)
        r = np.random.RandomState(1000 + len(key))
        self.n = None
        self._prefix_len, self._policy, self._rng = c["prefix"], bool(c.get("policy")), r

    def emu(self):
        """a HostEmu of the case in its state after the prefix"""
        import hostemu
        e = hostemu.HostEmu(self.name, self.B, self.seeds, auto_reset=False, **self.kw)
        for a in self.prefix(e.n):
            e.step(a)
        return e

    def oracle_spec(self):
        """the spec the ORACLE is built from: the scenario table's, DoorKey's hand-written one (tests/draw_envs.py)"""
        import draw_diff
        import scenarios
        if self.name == DK8:
            return draw_diff.spec_for(DK8, self.kw.get("max_steps", 100))
        return dict(scenarios.registered(self.name), **self.kw)

    def prefix(self, n):
        if self.n is None:
            self.n = n
            self._prefix = self._rng.randint(0, 7, (self._prefix_len, self.B, n)).astype(np.int64)
            self._plans = self._rng.randint(0, 7, (self.K, self.T, self.B, n)).astype(np.int64)
            if self._policy:
                self._plans[0] = self._policy_plan()
        return self._prefix

    def plans(self, n):
        self.prefix(n)
        return self._plans

    def _policy_plan(self):
        import hostemu_solve as HS
        e = self.emu()
        out = np.full((self.T, self.B, e.n), 6, np.int64)
        for t in range(self.T):
            _, act, _ = HS.run(e._cfg(), e.state, 64)
            out[t] = np.where(act < 0, 6, act)
            e.step(out[t])
        return out


@functools.lru_cache(maxsize=None)
def case(key):
    return Case(key)


def _ended(e, max_steps):
    s = e.state()
    return s["step_count"] >= max_steps or bool(s["done"].all())


def _step(e, a):
    """OracleEnv.step without the observations"""
    a = np.ascontiguousarray(a, dtype=np.int32)
    rew = np.zeros(e.n, np.float64)
    done = C.c_int32(0)
    order = np.zeros(e.n, np.int32)
    O._raise(e.L.mgo_step(e.h, O._p(a, C.c_int32), O._p(rew, C.c_double), C.byref(done), O._p(order, C.c_int32)))
    return rew, bool(done.value)


class Want(object):
    """the oracle's answer for a case: rewards (K, T, m, n) float64, done (K, T, m) bool, froze (K, m) — the first frozen row of
    the plan, T if none —, and the envs as the plans left them (row p * m + j)"""

    def __init__(self, cs, ids=None):
        spec = cs.oracle_spec()
        n = len(spec["agents"])
        ids = np.arange(cs.B) if ids is None else np.asarray(ids)
        prefix, plans = cs.prefix(n), cs.plans(n)
        K, T, m = cs.K, cs.T, len(ids)
        self.spec, self.ids = spec, ids
        self.rewards = np.zeros((K, T, m, n))
        self.done = np.zeros((K, T, m), bool)
        self.froze = np.full((K, m), T)
        self.envs = []
        for p in range(K):
            for j, b in enumerate(ids):
                e = O.OracleEnv(spec, int(cs.seeds[b]), _like=self.envs[0] if self.envs else None)
                for a in prefix:
                    _step(e, a[b])
                for t in range(T):
                    if self.froze[p, j] == T and _ended(e, spec["max_steps"]):
                        self.froze[p, j] = t
                    if self.froze[p, j] < T:
                        self.done[p, t, j] = True
                        continue
                    self.rewards[p, t, j], self.done[p, t, j] = _step(e, plans[p, t, b])
                self.envs.append(e)
        self.canon = [canon.oracle_canonical(e) for e in self.envs]

    def coverage(self, cs):
        """what the case is there for, from the oracle's envs alone"""
        K, m = cs.K, len(self.ids)
        differ = [j for j in range(m) if any(not _same(self.canon[j], self.canon[p * m + j]) for p in range(1, K))]
        assert differ, "no env whose plans end in different states"
        if cs.key == "truncated":
            ended = [(p, j) for p in range(K) for j in range(m) if self.froze[p, j] < cs.T or self.done[p, -1, j]]
            assert len(ended) == K * m, "every row ends inside the rollout"
            term = [all(self.canon[p * m + j]["done"]) for p, j in ended]
            assert any(term) and not all(term), "one row ends by termination and one by truncation"
        if cs.key == "doorkey":
            types = [o["type"] if o else None for o in self.spec["objects"]]
            key_ids = [i for i, t in enumerate(types) if t == "Key"]
            open_ids = [i for i, o in enumerate(self.spec["objects"]) if o and o["type"] == "Door" and o.get("state", 0) == 1]
            states = [e.state() for e in self.envs]
            assert any(np.isin(s["carrying"], key_ids).any() for s in states), "no plan picks the key up"
            assert any(np.isin(s["base"], open_ids).any() for s in states), "no plan opens the door"


def _same(a, b):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in canon.KEYS)


def compare(want, rewards, done, st, product_spec, what=""):
    """rewards (K, T, m, n), done (K, T, m) and the shadow state `st` — dict(grid (R, W, H), rec, step_count, mt, mt_pos,
    mt_head) — against the oracle: done exactly, rewards within REW_TOL, the state every row was left in (a frozen row: at the
    step it froze) and its generator in numpy's form and head words"""
    assert done.dtype == bool and np.array_equal(done, want.done), (what, np.argwhere(done != want.done)[:4])
    err = np.abs(rewards.astype(np.float64) - want.rewards)
    assert err.max() <= REW_TOL, (what, err.max(), np.argwhere(err > REW_TOL)[:4])
    R = len(want.envs)
    got = product_envs.canonical_arrays(product_spec, st["grid"][:R], st["rec"][:R], st["step_count"][:R])
    for r in range(R):
        canon.assert_same(got[r], want.canon[r], "%s row %d" % (what, r))
    okey, opos, onext = wide_diff.oracle_rng(want.envs)
    key, pos = wide_diff.numpy_form_rows(st["mt"][:R], st["mt_pos"][:R])
    bad = wide_diff.stream_diff(key, pos, okey, opos)
    assert not bad.any(), (what, "RNG state", np.nonzero(bad)[0][:8])
    head = np.ascontiguousarray(st["mt_head"][:R]).view(np.uint32)
    assert np.array_equal(head, onext), (what, "mt_head", np.nonzero((head != onext).any(axis=1))[0][:8])
