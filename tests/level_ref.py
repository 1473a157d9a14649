"""TEST INFRASTRUCTURE — the expected trajectory of replayable levels (MultiGridEnv.set_levels), from the oracle's independent
envs: episode_ref.EpisodeOracle whose reset of an env that has a level assigned is the reference's `env.seed(s); env.reset()`
(marlgrid/base.py:371-374, 402-416) — the env is swapped for `OracleEnv(spec, seed=s, construct=False)`, a generator freshly
seeded with s and nothing drawn from it, and then reset.  An env without a level (-1) keeps its running stream.  A level stays
assigned until another is: every reset of the env replays it.

A WHOLE level is (seed, parameters, edit list): the env that is swapped in is given the level's `set_params` / `set_edits`
before it resets.  A level that names no parameters (no list) leaves the env what it holds: the fresh env is given the old
one's.  A free-running env keeps its stream AND its own rows — what plain `set_params` / `set_edits` gave it, or what the last
level it took left: the product's tables are per env, and a level's rows are copied over them.

`BankRef` is a full LevelBank restated in a few lines — slots of (seed, parameter values, list) and the slot each env is pointed
at —; it resolves the slots into what `LevelOracle.set_levels` takes.  `WideRef` puts a LevelOracle behind tests/wide_diff.py:run.
"""
import ctypes as C

import numpy as np

import episode_ref
from oracle import oracle as O


KMAX = 64      # the longest list an env can hold (marlgrid_hip.h: MG_GEN_MAX_EDITS)


class LevelOracle(episode_ref.EpisodeOracle):
    def __init__(self, spec, seeds, mode="next_step", render=False):
        assert mode in ("next_step", "same_step", None)     # (a same-step reset takes no level: plain setters only)
        episode_ref.EpisodeOracle.__init__(self, spec, seeds, mode=mode, render=render, views=False)
        self.spec = spec
        self._proto = list(self.envs)               # the envs the batch was built with: what `_like` copies the tables from
        self.names = [p[0] for p in spec.get("params", ())]
        P = len(self.names)
        self.next_level = np.full(self.B, -1, np.int64)
        self.next_params = np.full((self.B, P), -1, np.int64)      # what the level carries; -1: that parameter is not named
        self.next_edits = [None] * self.B                          # ... and its list; None: the level carries none
        # the env's own rows — what its next free-running reset reads (the product's params_t / edits_t rows) ...
        self.table_params = np.tile(np.asarray([p[1] for p in spec.get("params", ())], np.int64), (self.B, 1))
        self.table_edits = [[] for _ in range(self.B)]
        self.table_edits_arr = np.zeros((self.B, KMAX, 3), np.int64)    # (the same lists as one array, zero behind each list's end)
        # ... and what the running episode of each env was built from
        self.episode_level = np.full(self.B, -1, np.int64)
        self.episode_params = self.table_params.copy()
        self.episode_edits = [[] for _ in range(self.B)]
        self.levelled = np.zeros(self.B, np.int64)  # episodes each env started from a level
        self.last_reset = np.zeros(self.B, bool)    # the envs whose reset ran in the last call
        self._keys = {}
        self._lists_c = {}          # id(list) -> (the list, its entries as int32, the pointer): a bank's lists are played many times

    # ---- what each env's next reset starts from -------------------------------------------------------------------------------
    def set_levels(self, seeds, mask=None, params=None, edits=None):
        """seeds: an int or (B,) — -1: free-running —, for the envs of `mask` (all without one); from each env's next reset on.
        params: {name: (B,) values} the levels carry; edits: B lists [(x, y, obj_id), ...] (None: the levels carry none)"""
        s = np.broadcast_to(np.asarray(seeds, np.int64), (self.B,))
        m = np.ones(self.B, bool) if mask is None else np.asarray(mask, bool)
        self.next_level[m] = s[m]
        self.next_params[m] = -1
        for name, v in (params or {}).items():
            self.next_params[m, self.names.index(name)] = np.broadcast_to(np.asarray(v, np.int64), (self.B,))[m]
        for b in np.nonzero(m)[0]:
            self.next_edits[b] = None if edits is None else edits[b]

    def set_params(self, mask=None, **values):
        """plain `set_params` on running envs: the env's own row, read by its next reset"""
        m = np.ones(self.B, bool) if mask is None else np.asarray(mask, bool)
        for name, v in values.items():
            j = self.names.index(name)
            self.table_params[m, j] = np.broadcast_to(np.asarray(v, np.int64), (self.B,))[m]
            for b in np.nonzero(m)[0]:
                self.envs[b].set_params(**{name: int(self.table_params[b, j])})

    def set_edits(self, lists, mask=None):
        """plain `set_edits`: `lists` one list for everyone selected, or B lists"""
        m = np.ones(self.B, bool) if mask is None else np.asarray(mask, bool)
        per_env = len(lists) == self.B and all(isinstance(x, list) for x in lists)
        for b in np.nonzero(m)[0]:
            self._own_edits(b, lists[b] if per_env else lists)
            self.envs[b].set_edits(self.table_edits[b])

    def _own_edits(self, b, lst):
        """env b's own list from now on (the list object itself is kept: a bank's list is shared by the envs that took it)"""
        self.table_edits[b] = lst
        self.table_edits_arr[b] = 0
        if lst:
            self.table_edits_arr[b, :len(lst)] = lst

    def _reset_env(self, b):
        s = int(self.next_level[b])
        if s >= 0:
            key = self._keys.get(s)
            if key is None:
                words = O.seed_key(s)
                key = self._keys[s] = (words, O._p(words, C.c_uint32), len(words))
            self.envs[b] = e = _Fresh(self.spec, key, self._proto[b])
            nxt = self.next_edits[b]
            if nxt is not None and nxt is not self.table_edits[b]:
                self._own_edits(b, nxt)
            # (OracleEnv.set_params / set_edits, without their conversions: this runs once per reset of every env of a wide batch)
            for j in range(len(self.names)):
                v = int(self.next_params[b, j])
                if v >= 0:
                    self.table_params[b, j] = v
                e.L.mgo_set_param(e.h, j, int(self.table_params[b, j]))
            lst = self.table_edits[b]
            if lst:
                c = self._lists_c.get(id(lst))
                if c is None or c[0] is not lst:
                    a = np.ascontiguousarray(np.asarray(lst, np.int32).reshape(-1, 3))
                    c = self._lists_c[id(lst)] = (lst, a, O._p(a, C.c_int32))
                O._raise(e.L.mgo_set_edits(e.h, c[2], len(lst)))
            self.levelled[b] += 1
        self.episode_level[b] = s if s >= 0 else -1
        self.episode_params[b] = self.table_params[b]
        self.episode_edits[b] = self.table_edits[b]
        self.last_reset[b] = True
        episode_ref.EpisodeOracle._reset_env(self, b)

    def reset(self):
        self.last_reset[:] = False
        return episode_ref.EpisodeOracle.reset(self)

    def reset_envs(self, mask):
        self.last_reset[:] = False
        return episode_ref.EpisodeOracle.reset_envs(self, mask)

    def step(self, actions, render=True):
        self.last_reset[:] = False
        obs, rew, done, info = episode_ref.EpisodeOracle.step(self, actions, render=render)
        # the level of the episode each row reports on: a `done` row's finished episode, a `reset` row's new one
        info["level"] = self.episode_level.copy()
        return obs, rew, done, info


class _Fresh(O.OracleEnv):
    """OracleEnv(spec, seed=s, construct=False, _like=proto) with the seed's key words handed in — (words, pointer, length) —: a
    level is played many times"""

    def __init__(self, spec, key, like):
        self.spec, self.L, self.cfg = spec, like.L, like.cfg
        self.h = self.L.mgo_create_like(like.h, key[1], key[2])
        self.n, self.W, self.H, self.vs, self.ts, self.P = like.n, like.W, like.H, like.vs, like.ts, like.P


def assert_info(got, want, what):
    episode_ref.assert_info(got, want, what)
    assert np.array_equal(np.asarray(got["level"]).astype(np.int64), want["level"]), "%s: level" % what


# ---- a full bank, restated ------------------------------------------------------------------------------------------------------
class BankRef(object):
    """L slots of (seed, {name: value}, list) and the slot every env is pointed at — `LevelBank(full=True)` and `set_levels(bank,
    ids)` in the oracle's terms.  An env takes what its slot holds WHEN IT RESETS: after every `point` / `assign`, `push` hands
    the LevelOracle the levels as they are now."""

    def __init__(self, L, B, defaults):
        self.L, self.B = L, B
        self.seeds = np.full(L, -1, np.int64)
        self.params = {name: np.full(L, v, np.int64) for name, v in defaults.items()}
        self.edits = [[] for _ in range(L)]
        self.ids = np.full(B, -1, np.int64)

    def assign(self, slots, seeds, params=None, edits=None):
        """edits: one list per slot named (oracle entries), or None: the slots keep theirs"""
        for i, (sl, s) in enumerate(zip(slots, seeds)):
            self.seeds[sl] = s
            for name, v in (params or {}).items():
                self.params[name][sl] = np.broadcast_to(np.asarray(v, np.int64), (len(slots),))[i]
            if edits is not None:
                self.edits[sl] = list(edits[i])

    def point(self, ids, mask=None):
        m = np.ones(self.B, bool) if mask is None else np.asarray(mask, bool)
        self.ids[m] = np.broadcast_to(np.asarray(ids, np.int64), (self.B,))[m]

    def resolved(self):
        """-> (seed per env, -1 where it runs free: no slot, a slot outside the bank, an emptied slot; the slot, clipped)"""
        ok = (self.ids >= 0) & (self.ids < self.L)
        at = np.clip(self.ids, 0, self.L - 1)
        return np.where(ok, self.seeds[at], -1), at

    def push(self, ref):
        s, at = self.resolved()
        ref.set_levels(s, None, params={name: v[at] for name, v in self.params.items()}, edits=[self.edits[i] for i in at])


# ---- behind tests/wide_diff.py:run ----------------------------------------------------------------------------------------------
class WideRef(object):
    """a LevelOracle as `run(ref=...)` takes it.  `extra(subject)`: what the levels add to every step's checks — the seed the
    running episode of each env was started from, and the env's own rows (the product's tables filtered by the rule for entries
    that count, level_envs.valid)"""

    def __init__(self, spec, seeds, mode, n_obj, column=None):
        self.lo = LevelOracle(spec, seeds, mode=mode, render=False)
        self.envs = self.lo.envs
        self.n_obj, self.column = n_obj, column

    def reset(self):
        self.lo.reset()

    def reset_envs(self, mask):
        self.lo.reset_envs(mask)

    def step(self, a, pixels):
        _, r, d, info = self.lo.step(a, render=False)
        return None, r, d, info

    def extra(self, subject):
        """-> [(field, differing envs, detail)]"""
        import level_envs as LE
        lo, out = self.lo, []
        st = subject.level_state()
        if st.get("episode_level") is not None:
            bad = np.nonzero(np.asarray(st["episode_level"]).astype(np.int64) != lo.episode_level)[0]
            if bad.size:
                out.append(("episode_level", bad, "env %d: got %d, want %d" % (bad[0], st["episode_level"][bad[0]], lo.episode_level[bad[0]])))
        if st.get("params") is not None and lo.names:
            got = np.stack([np.asarray(st["params"][name]).astype(np.int64) for name in lo.names], axis=1)
            bad = np.nonzero((got != lo.table_params).any(axis=1))[0]
            if bad.size:
                out.append(("params_t", bad, "env %d: got %s, want %s" % (bad[0], got[bad[0]].tolist(), lo.table_params[bad[0]].tolist())))
        if st.get("edits") is not None:
            tab = np.asarray(st["edits"]).astype(np.int64)
            ok = LE.valid(tab, self.n_obj)
            order = np.argsort(~ok, axis=1, kind="stable")                  # the entries that count to the front, in table order
            got = np.take_along_axis(tab[..., :3], order[..., None], axis=1) * np.take_along_axis(ok, order, axis=1)[..., None]
            bad = np.nonzero((got != lo.table_edits_arr[:, :tab.shape[1]]).any(axis=(1, 2))
                             | (ok.sum(axis=1) != [len(x) for x in lo.table_edits]))[0]
            if bad.size:
                out.append(("edits_t (the entries that count)", bad, "env %d: got %s, want %s" % (
                    bad[0], tab[bad[0]][ok[bad[0]]].tolist(), lo.table_edits[bad[0]])))
        return out
