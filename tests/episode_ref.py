"""TEST INFRASTRUCTURE — the expected trajectory of the episode-boundary modes, from the oracle's independent envs.

`OracleBatch(...).envs[b]` are independent `OracleEnv`s with their own RNG.  Next-step reset, per env: if its last step
returned done -> `reset()` and this call's action row is consumed without being used (reward 0, done False, info "reset");
else `step(actions[b])`.  Same-step reset: `step`, and where done the info is taken BEFORE the `reset()` that follows.
Terminated = done and all(state()["done"]); truncated = done and not that; length = state()["step_count"]; return = the
float64 sum of the oracle's rewards.
"""
import ctypes as C

import numpy as np

from oracle import oracle as O


class EpisodeOracle(object):
    def __init__(self, spec, seeds, mode="next_step", render=False, views=False):
        """render: "image" -> obs (B, n, P, P, 3), "encoded" -> (B, n, V, V, 3) (tests/viewenc.py), False -> None.
        views: the scenario's agents carry their own view geometry — oracle.make_env's envs, stepped one by one; obs is then a
        list of n arrays (B, ...)."""
        assert mode in ("next_step", "same_step", None)
        self.mode, self.render, self.views = mode, render, views
        if views:
            self.orc = None
            self.envs = [O.make_env(spec, seed=int(s)) for s in seeds]
            self.B, self.n = len(self.envs), self.envs[0].n
        else:
            self.orc = O.OracleBatch(spec, seeds)
            self.envs = self.orc.envs
            self.B, self.n = self.orc.B, self.orc.n
        self.pending = np.zeros(self.B, bool)
        self.ret = np.zeros((self.B, self.n), np.float64)
        self.length = np.zeros(self.B, np.int64)
        self.n_terminated = self.n_truncated = 0
        self.episodes = np.zeros(self.B, np.int64)

    def reset(self):
        for b in range(self.B):
            self._reset_env(b)
        self.pending[:] = False
        return self.obs()

    def _reset_env(self, b):
        e = self.envs[b]
        for x in (e.envs if self.views else [e]):
            O._raise(x.L.mgo_reset(x.h, 1))
        self.ret[b] = 0
        self.length[b] = 0

    def reset_envs(self, mask):
        """a reset by hand of the masked envs (MultiGridEnv.reset(env_mask=...)): pending or not, they start a new episode"""
        for b in np.nonzero(mask)[0]:
            self._reset_env(b)
            self.pending[b] = False
        return self.obs()

    def obs(self):
        if not self.render:
            return None
        if self.render == "encoded":
            import viewenc
            per = [viewenc.oracle_views(e) for e in self.envs]
        else:
            per = [e.gen_obs() for e in self.envs]
        if self.views:
            return [np.stack([p[k] for p in per]) for k in range(self.n)]
        return np.stack([np.stack(p) for p in per])

    def step(self, actions, render=True):
        """-> obs (or None), rewards float64 (B, n), done (B,), info dict as MultiGridEnv.step(episode_info=True) returns it.
        render=False: obs is None for this call (a caller that does not look at every step); nothing else changes"""
        B, n = self.B, self.n
        a = np.ascontiguousarray(actions, np.int32).reshape(B, n)
        live = np.nonzero(~self.pending)[0]
        rew = np.zeros((B, n), np.float64)
        done = np.zeros(B, bool)
        info = dict(terminated=np.zeros(B, bool), truncated=np.zeros(B, bool), reset=self.pending.copy(),
                    episode_return=np.zeros((B, n), np.float64), episode_length=np.zeros(B, np.int32))
        for b in np.nonzero(self.pending)[0]:             # this call is the env's reset: the action row is not used
            self._reset_env(b)
        if len(live) and self.views:
            for b in live:
                e = self.envs[b]
                for x in e.envs:
                    r1 = np.zeros(n, np.float64)
                    d1 = C.c_int32(0)
                    order = np.zeros(n, np.int32)
                    O._raise(x.L.mgo_step(x.h, O._p(np.ascontiguousarray(a[b]), C.c_int32), O._p(r1, C.c_double), C.byref(d1),
                                          O._p(order, C.c_int32)))
                rew[b] = r1
                done[b] = bool(d1.value)
            self.ret[live] += rew[live]
            self.length[live] += 1
        elif len(live):
            h = (C.c_void_p * len(live))(*[self.envs[b].h for b in live])
            al = np.ascontiguousarray(a[live])
            rl = np.zeros((len(live), n), np.float64)
            dl = np.zeros(len(live), np.uint8)
            O._raise(self.orc.L.mgo_batch_step(h, len(live), O._p(al, C.c_int32), O._p(rl, C.c_double), O._p(dl, C.c_uint8),
                                               None, 0, 0))
            rew[live] = rl
            done[live] = dl.astype(bool)
            self.ret[live] += rl
            self.length[live] += 1
        info["episode_return"][live] = self.ret[live]
        info["episode_length"][live] = self.length[live]
        self.pending[:] = False
        for b in np.nonzero(done)[0]:
            st = self.envs[b].state()
            assert st["step_count"] == self.length[b], (b, st["step_count"], self.length[b])
            term = bool(st["done"].all())
            info["terminated"][b] = term
            info["truncated"][b] = not term
            self.n_terminated += int(term)
            self.n_truncated += int(not term)
            self.episodes[b] += 1
            if self.mode == "next_step":
                self.pending[b] = True
            elif self.mode == "same_step":
                self._reset_env(b)
        return (self.obs() if render else None), rew, done, info


def assert_info(got, want, what):
    """every info field, exactly (numpy arrays; the caller converts device tensors)"""
    for k in ("terminated", "truncated", "reset"):
        assert np.array_equal(np.asarray(got[k], bool), want[k]), "%s: %s" % (what, k)
    assert np.array_equal(np.asarray(got["episode_length"]).astype(np.int64), want["episode_length"].astype(np.int64)), "%s: length" % what
