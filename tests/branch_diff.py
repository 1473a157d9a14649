"""TEST INFRASTRUCTURE — the differentials of `_gen_grid` programs that BRANCH on their draws (`_fork`, `_rand_elem`, `_rand_bool`:
guarded ops, MG_GEN_GUARD) or read per-env PARAMETERS (MG_GEN_PARAM, a symbolic count) against the CPU oracle: what the host
differential (tests/test_gen_branches_diff_host.py) and the GPU differentials (tests/test_hip_gen_branches_oracle.py) share.
Both go through tests/wide_diff.py:run with the hand-written specs of tests/gen_branch_envs.py and tests/param_envs.py, in which
a branch is an `if` block and a parameter a value the oracle is handed — nothing of the product's encoding.

Coverage is a condition of every case and is read on the ORACLE's side (`Coverage.watch`: the oracle's own `draw[]` after each
of its in-launch resets — not the reset() before the first step, not a reset by hand): a subject cannot pass by never taking
a path."""
import numpy as np

import gen_branch_envs as G
import param_envs as PE

CDK8 = "MarlGrid-2AgentColoredDoorKey8x8-v0"        # the id `make` builds (marlgrid_amd/envs/__init__.py)
CHOICE7, CHOICE7_TS5, SIDES9, LONG12, DEEP = ("Branch-2AgentChoice7", "Branch-2AgentChoice7-ts5", "Branch-2AgentSides9",
                                              "Branch-2AgentLong12", G.DEEP)
PARAM = {PE.name_of(kind): kind for kind in PE.KINDS}                  # "Param-clutter" -> "clutter"
SEED0 = 717100


def kind_of(name):
    """-> (scenario kind, W, H)"""
    if name == CDK8:
        return "cdk", 8, 8
    if name in PARAM:
        return PARAM[name], PE.KINDS[PARAM[name]][0], PE.KINDS[PARAM[name]][1]
    return dict(G.SCENARIOS, **G.ORACLE_ONLY)[name][:3]


def spec_for(name, max_steps):
    if name == CDK8:
        return G.spec("cdk", 8, 8, 7, 8, max_steps)
    if name in PARAM:
        return PE.spec(PARAM[name], max_steps=max_steps)
    return G.spec_of(name, max_steps=max_steps)


def second_values(kind, vals):
    """the values every other env goes to at half time: another value of the interval, half of it further on"""
    lo, hi = PE.interval(kind)
    return lo + (vals - lo + (hi - lo) // 2) % (hi - lo)


class Coverage(object):
    """what the oracle's `_gen_grid` runs did, over every in-launch reset of every env of a run"""

    def __init__(self, name):
        self.name = name
        self.kind, self.W, self.H = kind_of(name)
        self.param = name in PARAM
        self.paths = set()          # ids into G.paths(kind, W)
        self.values = [set() for _ in range(16)]
        self.combos = set()         # parameter kinds: (value, `_rand_bool`'s draw) — the draw is -1 where the text makes none
        self.dependent = set()      # Deep: whether the draw that only one path makes was made
        self.counts = set()         # clutter, Deep: the count of the symbolic placement
        self.resets = 0
        self._last_t = 0

    def watch(self, t, envs, mask):
        hand = t == 0 or t == self._last_t          # reset(), or the staggered reset by hand that follows step t's own call
        self._last_t = t
        if hand:
            return
        for b in np.nonzero(mask)[0]:
            d, w = envs[b].draws()
            self.resets += 1
            for r in np.nonzero(w >= 0)[0]:
                self.values[r].add(int(d[r]))
            if self.param:
                self.combos.add((int(d[0]), int(d[1])))
                if self.kind == "clutter":
                    self.counts.add(int(d[0]))
            else:
                self.paths.add(G.oracle_path(self.kind, self.W, envs[b]))
                if self.kind == "deep":
                    self.dependent.add(bool(w[5] >= 0))
                    self.counts.add(int(d[2]) - 1)                    # count=n - 1

    def require(self):
        name, W = self.name, self.W
        if self.param:
            lo, hi = PE.interval(self.kind)
            bools = (0, 1) if self.kind in ("kind", "long") else (-1,)
            want = {(v, b) for v in range(lo, hi) for b in bools}
            assert self.combos == want, (name, "missing (value, bool):", sorted(want - self.combos))
            if self.kind == "clutter":
                assert 0 in self.counts, (name, sorted(self.counts))
            return
        want = set(range(len(G.paths(self.kind, W))))
        assert self.paths == want, (name, "paths not taken:", [G.paths(self.kind, W)[p] for p in sorted(want - self.paths)])
        if self.kind == "cdk":      # _rand_int(2, W - 2), _rand_int(1, W - 2), the colour
            assert self.values[0] == set(range(2, W - 2)) and self.values[1] == set(range(1, W - 2)), (name, self.values[:2])
            assert self.values[2] == set(range(len(G.DOOR_COLORS))), (name, self.values[2])
        if self.kind == "deep":
            assert self.dependent == {False, True}, (name, self.dependent)
            assert self.counts == {0, 1, 2}, (name, self.counts)


def subject_env(subject):
    """the product env behind a subject of wide_diff (HipSubject.env, HostEmuSubject.emu.env)"""
    return subject.env if hasattr(subject, "env") else subject.emu.env


def host_subject(name, B, seeds, max_steps):
    import hostemu
    import hostemu_params
    import wide_diff
    G.register()
    PE.register()
    cls = hostemu_params.ParamEmu if name in PARAM else hostemu.HostEmu
    return wide_diff.HostEmuSubject(cls(name, B, seeds, auto_reset=True, par=True, max_steps=max_steps))


def run(subject, name, seeds, T, max_steps, **kw):
    """wide_diff.run against the hand-written spec, with the coverage of the case required -> (what run returns, Coverage).
    A parameter scenario runs with param_envs.values over the batch — set on both sides before the first reset (the
    constructors' resets ran with the default on both) —, and after step T // 2 every other env is given `second_values`, on
    both sides: an env's next reset reads it."""
    import wide_diff
    cov = Coverage(name)
    between = None
    if name in PARAM:
        kind = PARAM[name]
        pname = PE.KINDS[kind][2]
        B = subject.B
        vals = PE.values(kind, B)
        ids = np.arange(0, B, 2)

        def between(t, sub, envs):
            if t == 0:
                subject_env(sub).set_params(**{pname: vals})
                for b, e in enumerate(envs):
                    e.set_params(**{pname: int(vals[b])})
            elif t == T // 2:
                new = second_values(kind, vals[ids])
                assert (new != vals[ids]).all()
                subject_env(sub).set_params(env_ids=ids, **{pname: new})
                for b, v in zip(ids, new):
                    envs[b].set_params(**{pname: int(v)})
    out = wide_diff.run(subject, name, seeds, T, spec=spec_for(name, max_steps), watch=cov.watch, between=between, **kw)
    cov.require()
    assert out["episodes"].min() >= 3, out["episodes"].min()       # every env was reset inside a launch three times
    return out, cov
