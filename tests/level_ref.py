"""TEST INFRASTRUCTURE — the expected trajectory of replayable levels (MultiGridEnv.set_levels), from the oracle's independent
envs: episode_ref.EpisodeOracle whose reset of an env that has a level assigned is the reference's `env.seed(s); env.reset()`
(marlgrid/base.py:371-374, 402-416) — the env is swapped for `OracleEnv(spec, seed=s, construct=False)`, a generator freshly
seeded with s and nothing drawn from it, and then reset.  An env without a level (-1) keeps its running stream.  A level stays
assigned until another is: every reset of the env replays it.
"""
import numpy as np

import episode_ref
from oracle import oracle as O


class LevelOracle(episode_ref.EpisodeOracle):
    def __init__(self, spec, seeds, mode="next_step", render=False):
        assert mode in ("next_step", None)          # (a same-step reset takes no level)
        episode_ref.EpisodeOracle.__init__(self, spec, seeds, mode=mode, render=render, views=False)
        self.spec = spec
        self._proto = list(self.envs)               # the envs the batch was built with: what `_like` copies the tables from
        self.next_level = np.full(self.B, -1, np.int64)
        self.episode_level = np.full(self.B, -1, np.int64)
        self.levelled = np.zeros(self.B, np.int64)  # episodes each env started from a level

    def set_levels(self, seeds, mask=None):
        """seeds: an int or (B,) — -1: free-running —, for the envs of `mask` (all without one); from each env's next reset on"""
        s = np.broadcast_to(np.asarray(seeds, np.int64), (self.B,))
        m = np.ones(self.B, bool) if mask is None else np.asarray(mask, bool)
        self.next_level[m] = s[m]

    def _reset_env(self, b):
        s = int(self.next_level[b])
        if s >= 0:
            self.envs[b] = O.OracleEnv(self.spec, seed=s, construct=False, _like=self._proto[b])
            self.levelled[b] += 1
        self.episode_level[b] = s if s >= 0 else -1
        episode_ref.EpisodeOracle._reset_env(self, b)

    def step(self, actions, render=True):
        obs, rew, done, info = episode_ref.EpisodeOracle.step(self, actions, render=render)
        # the level of the episode each row reports on: a `done` row's finished episode, a `reset` row's new one
        info["level"] = self.episode_level.copy()
        return obs, rew, done, info


def assert_info(got, want, what):
    episode_ref.assert_info(got, want, what)
    assert np.array_equal(np.asarray(got["level"]).astype(np.int64), want["level"]), "%s: level" % what
