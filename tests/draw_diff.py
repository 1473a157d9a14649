"""TEST INFRASTRUCTURE — the differentials of `_gen_grid` programs with `_rand_int` draws against the CPU oracle: what the
host differential (tests/test_gen_draws_diff_host.py) and the GPU differentials (tests/test_hip_gen_draws_oracle.py) share.
Both go through tests/wide_diff.py:run with the hand-written specs of tests/draw_envs.py.

Coverage is a condition of every case and is read on the ORACLE's side (`Coverage.watch`, the oracle's own `draw[]` after each
of its resets): a subject cannot pass by never reaching the edge."""
import numpy as np

import draw_envs as D

DOORKEY8 = "MarlGrid-2AgentDoorKey8x8-v0"        # the id `make` builds (marlgrid_amd/envs/__init__.py)
SPLIT7, EIGHT, IN_PLACE = "Draws-2AgentSplit7", "Draws-2AgentEight12x10", "Draws-2AgentSplit160x150"
SEED0 = 515100


def spec_for(name, max_steps):
    if name == DOORKEY8:
        return D.spec("doorkey", 8, 8, 7, 8, max_steps)
    return D.spec_of(name, max_steps=max_steps)


def legal_values(name):
    """register -> every value the reference can draw there, for the registers whose whole range a case must see: the split
    column and the gap / door row (from the `_gen_grid` texts: _rand_int(lo, hi) gives lo .. hi - 1)"""
    if name == DOORKEY8:
        return {0: set(range(2, 6)), 1: set(range(1, 6))}              # _rand_int(2, W - 2), _rand_int(1, W - 2), W = 8
    if name == SPLIT7:
        return {0: set(range(2, 5)), 1: set(range(1, 6))}              # _rand_int(2, W - 2), _rand_int(1, H - 1)
    if name == EIGHT:
        return {0: set(range(3, 9)), 1: set(range(1, 9))}              # _rand_int(3, W - 3), _rand_int(1, H - 1), 12 x 10
    return {}


class Coverage(object):
    """what the oracle drew, over every reset of every env of a run"""

    def __init__(self):
        self.values = [set() for _ in range(16)]
        self.max_words = np.zeros(16, np.int64)
        self.resets = 0

    def watch(self, t, envs, mask):
        for b in np.nonzero(mask)[0]:
            d, w = envs[b].draws()
            for r in np.nonzero(w >= 0)[0]:
                self.values[r].add(int(d[r]))
            self.max_words = np.maximum(self.max_words, w)
            self.resets += 1

    def require(self, name):
        for r, want in legal_values(name).items():
            assert self.values[r] == want, (name, "register", r, sorted(self.values[r]), sorted(want))
        if name == EIGHT:
            for r in (4, 5, 6, 7):
                assert len(self.values[r]) >= 2, (r, self.values[r])
            # place_obj(top=(h - 3, 0), size=(4, H + 5)), h = draw[6]: the left edge is clamped for h < 3 only
            assert any(h < 3 for h in self.values[6]) and any(h >= 3 for h in self.values[6]), self.values[6]
            assert self.max_words[:8].max() > 1, self.max_words      # masked rejection: a draw that took more than one word
            assert self.max_words[4] == 0                            # the one-value range whose bounds are draws
        if name == IN_PLACE:
            # 156 columns and 148 rows: a few hundred layouts cannot see them all.  Required instead: both halves of the
            # byte — a draw below 128 and one with the top bit set — in the column AND in the row
            for r in (0, 1):
                assert min(self.values[r]) < 128 <= max(self.values[r]), (r, min(self.values[r]), max(self.values[r]))


def host_subject(name, B, seeds, max_steps):
    import hostemu
    import wide_diff
    D.register()
    return wide_diff.HostEmuSubject(hostemu.HostEmu(name, B, seeds, auto_reset=True, par=True, max_steps=max_steps))


def run(subject, name, seeds, T, max_steps, **kw):
    """wide_diff.run against the hand-written spec, with the coverage of the case required -> (what run returns, Coverage)"""
    import wide_diff
    cov = Coverage()
    out = wide_diff.run(subject, name, seeds, T, spec=spec_for(name, max_steps), watch=cov.watch, **kw)
    cov.require(name)
    assert out["episodes"].min() >= 3, out["episodes"].min()       # every env was reset inside a launch three times
    return out, cov
