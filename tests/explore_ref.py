"""TEST INFRASTRUCTURE — the reference the exploration maps (`MultiGridEnv(explore=True)`, mg_explore_update) are held to, on the
CPU and built on the ORACLE only: per (env, agent) the `vis` of `OracleEnv.view(k)` — the vis_mask of gen_obs_grid —, and of
`state()` the positions, directions, stack ordinals (-1: the agent is in no cell) and the step count; for agents with their own
view geometry the `OracleEnvViews` owner of each agent.  The C entry points behind `view()` and `state()` (mgo_view,
mgo_get_state) are called straight into arrays kept for the whole batch: 4 099 envs x 3 agents x 60 steps are 750 000 views.

It does NOT use mg_core.h's view_map.  View cell [i, j] is mapped to a world cell as the reference's gen_obs_grid does it: an
index grid (x * H + y, -1 outside) sliced at `get_view_exts` (agents.py:237-266, restated below) and rotated dir + 1 times by the
reference's `rotate_grid` (base.py:67-80, restated below).  The map is ANCHORED on every call: for every visible view cell whose
top code is an object id, `state()["base"]` must hold that id at the mapped cell, or `observe` raises.

`ExploreRef` keeps seen / visits per oracle env under the feature's rules: cleared when the oracle's step count is 0, one update
per observation.  `RefBatch` steps the oracle envs under the three reset modes and calls `observe` once per observation."""
import ctypes as C

import numpy as np

from oracle import oracle as O

AGENT_BASE = 1000       # MGO_AGENT_BASE (oracle/mg_oracle.h): a cell code from here on is an agent


def rotate_grid(grid, rot_k):
    """base.py:67-80 of the reference, on the last two axes of a stack of grids"""
    rot_k = rot_k % 4
    if rot_k == 3:
        return np.moveaxis(grid[..., :, ::-1], -2, -1)
    if rot_k == 1:
        return np.moveaxis(grid[..., ::-1, :], -2, -1)
    if rot_k == 2:
        return grid[..., ::-1, ::-1]
    return grid


def view_exts(x, y, d, vs, off):
    """get_view_exts (agents.py:237-266): (topX, topY) for arrays of positions and directions"""
    h = vs // 2
    top_x = np.select([d == 0, d == 1, d == 2], [x - off, x - h, x - vs + 1 + off], x - h)
    top_y = np.select([d == 0, d == 1, d == 2], [y - h, y - off, y - h], y - vs + 1 + off)
    return top_x, top_y


def view_cells(x, y, d, vs, off, W, H):
    """(m, vs, vs) int64: the world cell x * H + y under view cell [i, j] of m agents, -1 outside the grid — MultiGrid.slice
    (base.py:123-147: zero padding) of an index grid, then rotate_grid(dir + 1)"""
    pad = vs + 1
    index = np.full((W + 2 * pad, H + 2 * pad), -1, np.int64)
    index[pad:pad + W, pad:pad + H] = np.arange(W * H).reshape(W, H)
    top_x, top_y = view_exts(x, y, d, vs, off)
    # (an agent in no cell has position -1, -1: its window is clipped to the padded grid, and nothing of it is used)
    ii = np.clip(top_x[:, None] + np.arange(vs)[None, :] + pad, 0, W + 2 * pad - 1)
    jj = np.clip(top_y[:, None] + np.arange(vs)[None, :] + pad, 0, H + 2 * pad - 1)
    sub = index[ii[:, :, None], jj[:, None, :]]
    out = np.empty_like(sub)
    for k in range(4):
        m = d == k
        if m.any():
            out[m] = rotate_grid(sub[m], k + 1)
    return out


class ExploreRef(object):
    """seen (B, n, W, H) bool, visits (B, n, W, H) int32, new_cells / visit_count (B, n) int32 of a list of oracle envs
    (OracleEnv or OracleEnvViews), brought up to date by `observe`"""

    def __init__(self, envs):
        self.envs = envs
        e0 = envs[0]
        self.views = isinstance(e0, O.OracleEnvViews)
        first = e0.envs[0] if self.views else e0
        self.B, self.n, self.W, self.H = len(envs), first.n, first.W, first.H
        self.L = first.L
        owner = e0.owner if self.views else [0] * self.n
        subs = e0.envs if self.views else [e0]
        self.geom = [(subs[owner[k]].cfg.view_size, subs[owner[k]].cfg.view_offset) for k in range(self.n)]
        # handle of the env that owns agent k's geometry, per env; the state machine is shared: state from the first
        self.h_view = [[(e.envs[owner[k]] if self.views else e).h for k in range(self.n)] for e in envs]
        self.h_state = [(e.envs[0] if self.views else e).h for e in envs]
        B, n, W, H = self.B, self.n, self.W, self.H
        self.seen = np.zeros((B, n, W, H), bool)
        self.visits = np.zeros((B, n, W, H), np.int32)
        self.new_cells = np.zeros((B, n), np.int32)
        self.visit_count = np.zeros((B, n), np.int32)
        self.base = np.zeros((B, W, H), np.uint8)
        self.ag = np.zeros((B, n, 7), np.int32)
        self.sc = np.zeros(B, np.int32)
        self.vis = [np.zeros((B, vs, vs), np.uint8) for vs, _ in self.geom]
        self.cells = [np.zeros((B, vs, vs), np.int32) for vs, _ in self.geom]
        self.observations = 0

    def _fetch(self, ids):
        """state and views of the envs `ids` into the batch's arrays (the two entry points under prototypes that take plain
        addresses: no pointer object per call)"""
        n, W, H = self.n, self.W, self.H
        vp = C.c_void_p
        get_state = C.cast(self.L.mgo_get_state, C.CFUNCTYPE(None, vp, vp, vp, vp))
        view = C.cast(self.L.mgo_view, C.CFUNCTYPE(None, vp, C.c_int32, vp, vp))
        base, ag, sc, hs = self.base.ctypes.data, self.ag.ctypes.data, self.sc.ctypes.data, self.h_state
        for b in ids:
            get_state(hs[b], base + b * W * H, ag + b * n * 28, sc + b * 4)
        for k, (vs, _) in enumerate(self.geom):
            vis, cells, hv, vv = self.vis[k].ctypes.data, self.cells[k].ctypes.data, self.h_view, vs * vs
            for b in ids:
                view(hv[b][k], k, vis + b * vv, cells + b * vv * 4)

    def observe(self, ids=None):
        """one observation of the envs `ids` (default: all) has been returned: clear where the step count is 0, then accumulate"""
        ids = np.arange(self.B) if ids is None else np.asarray(ids, np.int64).reshape(-1)
        if ids.size == 0:
            return
        self._fetch(ids.tolist())
        self.observations += 1
        n, W, H = self.n, self.W, self.H
        fresh = ids[self.sc[ids] == 0]
        self.seen[fresh] = False
        self.visits[fresh] = 0
        seen_flat = self.seen.reshape(-1)
        for k, (vs, off) in enumerate(self.geom):
            ag = self.ag[ids, k]
            x, y, d, ordinal = ag[:, 0].astype(np.int64), ag[:, 1].astype(np.int64), ag[:, 2], ag[:, 6]
            vis = self.vis[k][ids] != 0
            codes = self.cells[k][ids]
            cell = view_cells(x, y, d, vs, off, W, H)
            # the anchor: a visible object of the view lies at the mapped world cell
            obj = vis & (codes > 0) & (codes < AGENT_BASE)
            at = np.where(obj, cell, 0)
            held = self.base[ids].reshape(len(ids), -1)[np.arange(len(ids))[:, None, None], at]
            bad = obj & ((cell < 0) | (held != codes))
            if bad.any():
                r, i, j = (int(v) for v in np.argwhere(bad)[0])
                raise AssertionError("explore_ref: env %d agent %d view cell [%d, %d] shows object %d, the mapped world cell %d "
                                     "holds %d" % (ids[r], k, i, j, codes[r, i, j], cell[r, i, j], held[r, i, j]))
            mark = vis & (cell >= 0)
            rows = np.broadcast_to(ids[:, None, None], cell.shape)[mark]
            flat = (rows * n + k) * (W * H) + cell[mark]
            new = ~seen_flat[flat]
            self.new_cells[ids, k] = np.bincount(np.searchsorted(ids, rows[new]), minlength=len(ids)) if ids.size else 0
            seen_flat[flat] = True
            placed = ordinal >= 0
            pb, px, py = ids[placed], x[placed], y[placed]
            self.visits[pb, k, px, py] += 1
            self.visit_count[ids, k] = 0
            self.visit_count[pb, k] = self.visits[pb, k, px, py]

    def tensors(self):
        return dict(seen=self.seen, visits=self.visits, new_cells=self.new_cells, visit_count=self.visit_count)


class RefBatch(object):
    """B oracle envs of one spec under a reset mode — False, "same_step" or "next_step" — with their ExploreRef: reset(mask)
    and step(actions) each end with one `observe` of the envs they cover, as the engine's reset() and step() do"""

    def __init__(self, spec, seeds, mode=False):
        views = any("view" in a for a in spec["agents"])
        self.orc = None if views else O.OracleBatch(spec, seeds)       # (one shared config, and the OpenMP step)
        self.envs = [O.make_env(spec, int(s)) for s in seeds] if views else self.orc.envs
        self.mode = mode
        self.ref = ExploreRef(self.envs)
        self.B, self.n = self.ref.B, self.ref.n
        self.pending = np.zeros(self.B, bool)       # next_step: the env's next call is its reset
        self.was_reset = np.zeros(self.B, bool)     # ... and this call was

    def _subs(self, b):
        e = self.envs[b]
        return e.envs if self.ref.views else [e]

    def _reset(self, b):
        for s in self._subs(b):
            O._raise(s.L.mgo_reset(s.h, 1))

    def reset(self, mask=None):
        ids = np.arange(self.B) if mask is None else np.nonzero(np.asarray(mask, bool))[0]
        for b in ids:
            self._reset(int(b))
        self.pending[ids] = False
        self.ref.observe(ids)

    def step(self, actions):
        """-> done (B,) bool"""
        a = np.ascontiguousarray(actions, np.int32).reshape(self.B, self.n)
        done = np.zeros(self.B, bool)
        self.was_reset[:] = False
        if self.mode == "next_step":
            self.was_reset[:] = self.pending
            for b in np.nonzero(self.pending)[0]:       # this call is the env's reset: its action row is not used
                self._reset(int(b))
        live = np.nonzero(~self.was_reset)[0]
        if self.orc is not None and live.size:
            h = (C.c_void_p * live.size)(*[self.envs[b].h for b in live])
            al, rl, dl = np.ascontiguousarray(a[live]), np.zeros((live.size, self.n), np.float64), np.zeros(live.size, np.uint8)
            O._raise(self.orc.L.mgo_batch_step(h, live.size, O._p(al, C.c_int32), O._p(rl, C.c_double), O._p(dl, C.c_uint8), None,
                                               int(self.mode == "same_step"), 0))
            done[live] = dl != 0
        else:
            rew, order, flag = np.zeros(self.n, np.float64), np.zeros(self.n, np.int32), C.c_int32(0)
            for b in live:
                for s in self._subs(b):
                    O._raise(s.L.mgo_step(s.h, O._p(a[b], C.c_int32), O._p(rew, C.c_double), C.byref(flag), O._p(order, C.c_int32)))
                done[b] = bool(flag.value)
                if done[b] and self.mode == "same_step":
                    self._reset(b)
        self.pending = done.copy()
        self.ref.observe()
        return done

    def state(self, b):
        return self._subs(b)[0].state()
