"""TEST INFRASTRUCTURE — the reference for goal_distance (numpy and the standard library only).

The definition, straight: a state is (x, y, dir); `left` / `right` change dir by -+1 mod 4; `forward` moves to
(x, y) + DIRVEC[dir] if that cell is inside the grid and enterable — nothing wraps —; the distance of a state is the smallest
number of actions after which a `forward` ENTERS a goal cell.  Entering a goal ends the episode, so a goal cell is never passed
through; an agent that stands on one has not entered it.  A state on a cell that is neither free nor goal has no distance, and
neither has an agent that is in no cell (not active, or evicted): -1.

  * `agent_bfs`     a forward queue search from ONE start state: the definition, linear in the number of states
  * `field_queue`   a reverse queue search for every state of ONE grid, linear too (the mazes' fields)
  * `field_levels`  the batched numpy field, level by level (the scenario batches); tests/test_goal_ref.py holds the three
                    to each other on the inputs the other tests use
"""
from collections import deque

import numpy as np

from marlgrid_amd import _native as N

DIRVEC = ((1, 0), (0, 1), (-1, 0), (0, -1))


def kinds_of(env):
    """(free_ids, goal_ids): bool per object id, by the rule of include/marlgrid_hip.h"""
    tab = env._obj_table()
    flags = np.array([d.flags for d in tab], np.int64)
    rk = np.array([d.reward_kind for d in tab], np.int64)
    ends = (flags & N.OF_ENDS_EPISODE) != 0
    goal = ends & (rk == 1)
    free = ((flags & N.OF_CAN_OVERLAP) != 0) & ~ends
    free[0] = True
    goal[0] = False
    return free, goal


def classify(grid, free_ids, goal_ids):
    """grid (..., W, H) of object ids -> (free, goal) bool arrays; an id outside the table blocks"""
    g = np.asarray(grid).astype(np.int64)
    known = g < len(free_ids)
    gi = np.where(known, g, 0)
    return free_ids[gi] & known, goal_ids[gi] & known


def agent_bfs(free, goal, x, y, d):
    """free, goal (W, H) bool; the distance of state (x, y, d), -1 if none"""
    W, H = free.shape
    if not (0 <= x < W and 0 <= y < H) or not (free[x, y] or goal[x, y]):
        return -1
    seen = np.zeros((W, H, 4), bool)
    seen[x, y, d] = True
    q = deque([(x, y, d, 0)])
    while q:
        cx, cy, cd, k = q.popleft()
        fx, fy = cx + DIRVEC[cd][0], cy + DIRVEC[cd][1]
        if 0 <= fx < W and 0 <= fy < H:
            if goal[fx, fy]:
                return k + 1
            if free[fx, fy] and not seen[fx, fy, cd]:
                seen[fx, fy, cd] = True
                q.append((fx, fy, cd, k + 1))
        for nd in ((cd + 3) & 3, (cd + 1) & 3):
            if not seen[cx, cy, nd]:
                seen[cx, cy, nd] = True
                q.append((cx, cy, nd, k + 1))
    return -1


def field_queue(free, goal):
    """free, goal (W, H) bool -> (W, H, 4) int32: every state's distance by a reverse queue search (linear in the states)"""
    W, H = free.shape
    fr, go = free.tolist(), goal.tolist()
    dist = [[[-1] * 4 for _ in range(H)] for _ in range(W)]
    q = deque()
    for x in range(W):
        for y in range(H):
            if fr[x][y] or go[x][y]:
                for d in range(4):
                    fx, fy = x + DIRVEC[d][0], y + DIRVEC[d][1]
                    if 0 <= fx < W and 0 <= fy < H and go[fx][fy]:
                        dist[x][y][d] = 1
                        q.append((x, y, d))
    while q:
        x, y, d = q.popleft()
        k = dist[x][y][d] + 1
        for nd in ((d + 3) & 3, (d + 1) & 3):     # the states that turn into (x, y, d)
            if dist[x][y][nd] < 0:
                dist[x][y][nd] = k
                q.append((x, y, nd))
        if fr[x][y]:                              # the state that walks into (x, y, d): a goal cell is entered, not crossed
            px, py = x - DIRVEC[d][0], y - DIRVEC[d][1]
            if 0 <= px < W and 0 <= py < H and (fr[px][py] or go[px][py]) and dist[px][py][d] < 0:
                dist[px][py][d] = k
                q.append((px, py, d))
    return np.array(dist, np.int32).reshape(W, H, 4)


def _ahead(a, d):
    """a (B, W, H) bool -> bit (x, y) = a at (x, y) + DIRVEC[d], False outside the grid"""
    out = np.zeros_like(a)
    if d == 0:
        out[:, :-1, :] = a[:, 1:, :]
    elif d == 1:
        out[:, :, :-1] = a[:, :, 1:]
    elif d == 2:
        out[:, 1:, :] = a[:, :-1, :]
    else:
        out[:, :, 1:] = a[:, :, :-1]
    return out


def field_levels(free, goal):
    """free, goal (B, W, H) bool -> (B, W, H, 4) int32, level by level over the whole batch"""
    B, W, H = free.shape
    open_ = free | goal
    dist = np.full((B, W, H, 4), -1, np.int32)
    front = np.stack([open_ & _ahead(goal, d) for d in range(4)], axis=-1)
    level = 1
    while front.any():
        dist[front] = level
        level += 1
        nxt = np.zeros_like(front)
        for d in range(4):
            nxt[..., d] = open_ & (front[..., (d + 1) & 3] | front[..., (d + 3) & 3] | _ahead(front[..., d] & free, d))
        front = nxt & (dist < 0)
    return dist


def agents_from_field(field, pos, dirs, flags):
    """field (B, W, H, 4), pos (B, n, 2), dirs (B, n), flags (B, n) -> (B, n) int32: the field at each agent's state, -1 for an
    agent in no cell"""
    field, pos, dirs, flags = (np.asarray(v) for v in (field, pos, dirs, flags))
    B, W, H, _ = field.shape
    x, y = pos[..., 0].astype(np.int64), pos[..., 1].astype(np.int64)
    in_cell = ((flags & N.AF_ACTIVE) != 0) & ((flags & N.AF_EVICTED) == 0) & (x < W) & (y < H)
    b = np.arange(B)[:, None]
    v = field[b, np.minimum(x, W - 1), np.minimum(y, H - 1), dirs.astype(np.int64) & 3]
    return np.where(in_cell, v, -1).astype(np.int32)


def unpack_records(rec):
    """packed agent records (B, n) uint64 -> pos (B, n, 2), dirs, flags"""
    rec = np.asarray(rec).astype(np.uint64)

    def byte(i):
        return ((rec >> np.uint64(8 * i)) & np.uint64(0xFF)).astype(np.int64)
    return np.stack([byte(N.AG_X), byte(N.AG_Y)], axis=-1), byte(N.AG_DIR), byte(N.AG_FLAGS)


def serpentine(W, H):
    """The serpentine maze: a border wall; a wall on every second column, x = 2, 4, ... < W - 1, with one gap each — at
    y = H - 2 for the first, at y = 1 for the second, and so on in turn —; the start is (1, 1) facing +x; the goal, put last, is
    the cell (W - 2, H - 2) after an even number of walls and (W - 2, 1) after an odd one: the far end of the last corridor
    (at an even W the last wall's own column: the goal replaces the wall cell the last corridor looks at).
    -> (wall (W, H) bool without the goal's cell, goal (x, y))"""
    wall = np.zeros((W, H), bool)
    wall[0, :] = wall[-1, :] = True
    wall[:, 0] = wall[:, -1] = True
    xs = list(range(2, W - 1, 2))
    for k, x in enumerate(xs):
        wall[x, 1:H - 1] = True
        wall[x, H - 2 if k % 2 == 0 else 1] = False
    goal = (W - 2, H - 2 if len(xs) % 2 == 0 else 1)
    wall[goal] = False
    return wall, goal


MAZES = {(35, 35): 609, (5, 70): 139, (70, 5): 199, (67, 131): 4353, (255, 255): 32509}
