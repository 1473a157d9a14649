"""TEST INFRASTRUCTURE — the reference for solve_distance (numpy and the standard library only).

  * `full_bfs`   the definition: a forward search over (x, y, dir, carry, whole grid) with the five actions `left`, `right`,
                 `forward`, `pickup`, `toggle` under the step's rules (marlgrid_amd/csrc/mg_core.h: step_agents); the answer is
                 the number of actions up to and including the `forward` that enters a goal cell, -1 if there is none
  * `layered`    the model mg_solve_distance searches (marlgrid_amd/csrc/mg_solve_core.h), with its caps, as a batched numpy
                 relaxation over (layer, x, y, dir) arrays: -> dist, first action, exact
tests/test_solve_ref.py holds the two to each other, and `full_bfs`'s rules to the oracle.

An object table is a `Kinds`: per id the flags, reward_kind, color_idx, toggle_next and unlock_next of MgObjDesc."""
from collections import deque

import numpy as np

from marlgrid_amd import _native as N

DIRVEC = ((1, 0), (0, 1), (-1, 0), (0, -1))
LEFT, RIGHT, FORWARD, PICKUP, TOGGLE, DONE = 0, 1, 2, 3, 5, 6
BLOCKED, FREE, GOAL = 0, 1, 2


class Kinds(object):
    def __init__(self, flags, rk, color, tog, unl):
        self.flags, self.rk, self.color, self.tog, self.unl = (np.asarray(v, np.int64) for v in (flags, rk, color, tog, unl))
        self.n = len(self.flags)
        ends = (self.flags & N.OF_ENDS_EPISODE) != 0
        kind = np.where(ends, np.where(self.rk == 1, GOAL, BLOCKED), np.where((self.flags & N.OF_CAN_OVERLAP) != 0, FREE, BLOCKED))
        kind[0] = FREE
        self.kind = kind

    @classmethod
    def of_env(cls, env):
        tab = env._obj_table()
        return cls(*[[getattr(d, f) for d in tab] for f in ("flags", "reward_kind", "color_idx", "toggle_next", "unlock_next")])

    def cell_kind(self, ident):
        return int(self.kind[ident]) if ident < self.n else BLOCKED

    def is_item(self, ident):
        return 0 < ident < self.n and self.kind[ident] == BLOCKED and bool(self.flags[ident] & N.OF_CAN_PICKUP)

    def is_shut_door(self, ident):
        f = self.flags[ident] if 0 < ident < self.n else 0
        return bool(f & N.OF_IS_DOOR) and self.kind[ident] == BLOCKED and not f & (N.OF_CAN_PICKUP | N.OF_CAN_OVERLAP | N.OF_IS_BOX)

    def key_colour(self, ident):
        """the colour a carried object unlocks, -1 if it is no key"""
        return int(self.color[ident]) if 0 < ident < self.n and self.flags[ident] & N.OF_IS_KEY else -1

    def door_cost(self, ident):
        """0 not openable, 1 closed, 2 locked — mg_solve_core.h: solve_door_cost"""
        shut = ident
        locked = bool(self.flags[ident] & N.OF_DOOR_LOCKED)
        if locked:
            shut = int(self.unl[ident])
            if not self.is_shut_door(shut) or self.flags[shut] & N.OF_DOOR_LOCKED:
                return 0
        if self.cell_kind(int(self.tog[shut])) != FREE:
            return 0
        return 2 if locked else 1


# ---- the definition ---------------------------------------------------------------------------------------------------------
def full_bfs(grid, kinds, x, y, d, carry=0):
    """grid (W, H) of ids; the agent's state -> the number of actions, -1 if there is no sequence"""
    W, H = grid.shape
    flags, tog, unl, color, n_obj = kinds.flags.tolist(), kinds.tog.tolist(), kinds.unl.tolist(), kinds.color.tolist(), kinds.n
    kind = kinds.kind.tolist()
    g0 = bytes(np.asarray(grid, np.uint8).reshape(-1).tolist())
    if not (0 <= x < W and 0 <= y < H) or kinds.cell_kind(g0[x * H + y]) == BLOCKED:
        return -1
    start = (x, y, d, carry, g0)
    seen = {start}
    q = deque([(start, 0)])
    while q:
        (cx, cy, cd, cc, g), k = q.popleft()
        succ = [(cx, cy, (cd + 3) & 3, cc, g), (cx, cy, (cd + 1) & 3, cc, g)]
        fx, fy = cx + DIRVEC[cd][0], cy + DIRVEC[cd][1]
        if 0 <= fx < W and 0 <= fy < H:
            cell = fx * H + fy
            fb = g[cell]
            if fb < n_obj:          # (an id outside the table blocks and is never touched)
                fk, ff = kind[fb], flags[fb]
                if fk == GOAL:
                    return k + 1
                if fk == FREE:
                    succ.append((fx, fy, cd, cc, g))
                if fb and ff & N.OF_CAN_PICKUP and cc == 0:
                    succ.append((cx, cy, cd, fb, g[:cell] + b"\0" + g[cell + 1:]))
                if fb and not ff & N.OF_IS_BOX and ff & N.OF_IS_DOOR:
                    new = None
                    if ff & N.OF_DOOR_LOCKED:
                        if cc and cc < n_obj and flags[cc] & N.OF_IS_KEY and color[cc] == color[fb]:
                            new = unl[fb]
                    else:
                        new = tog[fb]
                    if new is not None:
                        succ.append((cx, cy, cd, cc, g[:cell] + bytes([new]) + g[cell + 1:]))
        for s in succ:
            if s not in seen:
                seen.add(s)
                q.append((s, k + 1))
    return -1


# ---- the layered model -------------------------------------------------------------------------------------------------------
BIG = 1 << 30


def _shift(a, d):
    """a (..., W, H) -> out[x, y] = a at (x, y) + DIRVEC[d], BIG outside the grid"""
    out = np.full_like(a, BIG)
    if d == 0:
        out[..., :-1, :] = a[..., 1:, :]
    elif d == 1:
        out[..., :, :-1] = a[..., :, 1:]
    elif d == 2:
        out[..., 1:, :] = a[..., :-1, :]
    else:
        out[..., :, 1:] = a[..., :, :-1]
    return out


def _interactables(grid, kinds, max_doors, max_items):
    """per row of grid (R, W, H): the tracked doors' and items' cells in index order, and `exact`"""
    R, W, H = grid.shape
    door_ids = np.array([kinds.is_shut_door(i) for i in range(256)])
    item_ids = np.array([kinds.is_item(i) for i in range(256)])
    flat = grid.reshape(R, -1)
    doors, items, exact = [], [], np.zeros(R, bool)
    for r in range(R):
        dc = np.flatnonzero(door_ids[flat[r]])
        ic = np.flatnonzero(item_ids[flat[r]])
        exact[r] = len(dc) <= max_doors and len(ic) <= max_items
        doors.append([(int(c) // H, int(c) % H) for c in dc[:max_doors]])
        items.append([(int(c) // H, int(c) % H) for c in ic[:max_items]])
    return doors, items, exact


def _relax(grid, kinds, doors, items, pass_key):
    """grid (R, W, H); doors / items: per row the tracked cells; pass_key (R,): the colour the agent's own carry unlocks, -1
    none.  -> dist (R, layers, W, H, 4) with BIG where there is none, D, and the edge list [(row, layer, target, x, y, cost)]"""
    R, W, H = grid.shape
    D = max([len(v) for v in doors] + [0])
    K = max([len(v) for v in items] + [0])
    layers = (1 + K) << D
    known = grid < kinds.n
    kind = np.where(known, kinds.kind[np.where(known, grid, 0)], BLOCKED)
    free = np.repeat((kind == FREE)[:, None], layers, axis=1)        # (R, layers, W, H)
    goal = (kind == GOAL)[:, None]
    edges = []
    for r in range(R):
        for L in range(layers):
            S, sel = L & ((1 << D) - 1), L >> D
            if S >> len(doors[r]) or sel > len(items[r]):
                free[r, L] = False          # (a layer this row does not have)
                continue
            held = pass_key[r]
            if sel:
                ix, iy = items[r][sel - 1]
                free[r, L, ix, iy] = True
                held = kinds.key_colour(int(grid[r, ix, iy]))
            for j, (dx, dy) in enumerate(doors[r]):
                if (S >> j) & 1:
                    free[r, L, dx, dy] = True
                    continue
                ident = int(grid[r, dx, dy])
                cost = kinds.door_cost(ident)
                if cost == 1 or (cost == 2 and held == kinds.color[ident]):
                    edges.append((r, L, L | (1 << j), dx, dy, cost))
            if not sel:
                for m, (ix, iy) in enumerate(items[r]):
                    edges.append((r, L, L + ((m + 1) << D), ix, iy, 1))
    open_ = free | goal
    dist = np.full((R, layers, W, H, 4), BIG, np.int64)
    for d in range(4):
        dist[..., d][open_ & (_shift(np.where(goal, 0, BIG), d) == 0)] = 1
    e = np.array(edges, np.int64).reshape(-1, 6)
    while True:
        new = dist.copy()
        for d in range(4):
            walk = _shift(np.where(free, dist[..., d], BIG), d)     # a goal cell is entered, never crossed
            cand = np.minimum(np.minimum(dist[..., (d + 1) & 3], dist[..., (d + 3) & 3]), walk) + 1
            new[..., d] = np.where(open_, np.minimum(new[..., d], cand), BIG)
            if len(e):
                px, py = e[:, 3] - DIRVEC[d][0], e[:, 4] - DIRVEC[d][1]
                ok = (px >= 0) & (px < W) & (py >= 0) & (py < H)
                r_, s_, t_, px, py, c_ = e[ok, 0], e[ok, 1], e[ok, 2], px[ok], py[ok], e[ok, 5]
                ok2 = open_[r_, s_, px, py]
                r_, s_, t_, px, py, c_ = r_[ok2], s_[ok2], t_[ok2], px[ok2], py[ok2], c_[ok2]
                np.minimum.at(new[..., d], (r_, s_, px, py), dist[r_, t_, px, py, d] + c_)
        new = np.minimum(new, BIG)
        if np.array_equal(new, dist):
            return dist, D, e
        dist = new


def _first_action(dist, D, e, kind_b, r, x, y, d):
    """kind_b (W, H): the cell kinds of the env that row r of dist belongs to"""
    d0 = dist[r, 0, x, y, d]
    if dist[r, 0, x, y, (d + 3) & 3] == d0 - 1:
        return LEFT
    if dist[r, 0, x, y, (d + 1) & 3] == d0 - 1:
        return RIGHT
    W, H = kind_b.shape
    fx, fy = x + DIRVEC[d][0], y + DIRVEC[d][1]
    if not (0 <= fx < W and 0 <= fy < H):
        return DONE
    if kind_b[fx, fy] == GOAL or (kind_b[fx, fy] == FREE and dist[r, 0, fx, fy, d] == d0 - 1):
        return FORWARD
    for (er, s_, t_, ox, oy, c_) in e[(e[:, 0] == r) & (e[:, 1] == 0)]:
        if (ox, oy) == (fx, fy) and dist[r, t_, x, y, d] == d0 - c_:
            return TOGGLE if t_ < (1 << D) else PICKUP
    return DONE


def layered(grid, kinds, x, y, d, in_cell, carry, max_doors=2, max_items=2):
    """grid (B, W, H) of ids; the agents' x, y, d, in_cell, carry as (B, n) arrays -> dist (B, n) int32, first action (B, n)
    int8 (6 where there is no path), exact (B,) bool"""
    grid = np.asarray(grid).astype(np.int64)
    B, W, H = grid.shape
    x, y, d, in_cell, carry = (np.asarray(v).astype(np.int64) for v in (x, y, d, in_cell, carry))
    in_cell = (in_cell != 0) & (x < W) & (y < H)
    out_d = np.full(x.shape, -1, np.int32)
    out_a = np.full(x.shape, DONE, np.int8)
    doors, items, exact = _interactables(grid, kinds, max_doors, max_items)
    known = grid < kinds.n
    kind0 = np.where(known, kinds.kind[np.where(known, grid, 0)], BLOCKED)

    def label(rows, pairs, dist, D, e):
        for r, (b, k) in zip(rows, pairs):
            v = dist[r, 0, x[b, k], y[b, k], d[b, k] & 3]
            if v < BIG:
                out_d[b, k] = v
                out_a[b, k] = _first_action(dist, D, e, kind0[b], r, int(x[b, k]), int(y[b, k]), int(d[b, k] & 3))

    # empty hands: one search per env that has such an agent
    envs = [b for b in range(B) if (in_cell[b] & (carry[b] == 0)).any()]
    if envs:
        dist, D, e = _relax(grid[envs], kinds, [doors[b] for b in envs], [items[b] for b in envs], np.full(len(envs), -1))
        pairs = [(b, k) for b in envs for k in range(x.shape[1]) if in_cell[b, k] and carry[b, k] == 0]
        row_of = {b: r for r, b in enumerate(envs)}
        label([row_of[b] for b, _ in pairs], pairs, dist, D, e)
    # an agent with something in hand: no item is tracked, its carry is the only key
    pairs = [(b, k) for b in range(B) for k in range(x.shape[1]) if in_cell[b, k] and carry[b, k] != 0]
    if pairs:
        rows = [b for b, _ in pairs]
        keys = np.array([kinds.key_colour(int(carry[b, k])) for b, k in pairs])
        dist, D, e = _relax(grid[rows], kinds, [doors[b] for b in rows], [[] for _ in rows], keys)
        label(range(len(pairs)), pairs, dist, D, e)
    return out_d, out_a, exact


def unpack(rec):
    """packed agent records (B, n) uint64 -> x, y, d, in_cell, carry"""
    rec = np.asarray(rec).astype(np.uint64)

    def byte(i):
        return ((rec >> np.uint64(8 * i)) & np.uint64(0xFF)).astype(np.int64)
    flags = byte(N.AG_FLAGS)
    return byte(N.AG_X), byte(N.AG_Y), byte(N.AG_DIR) & 3, ((flags & N.AF_ACTIVE) != 0) & ((flags & N.AF_EVICTED) == 0), byte(N.AG_CARRY)
