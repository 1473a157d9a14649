"""The reference for solve_distance (tests/solve_ref.py), without a GPU: the definition (`full_bfs`) and the layered model
(`layered`) held to each other on seeded random grids — with caps that cover every grid, and with caps (1, 1), where `exact`
says which values are the definition's and the others may only be larger —, and the definition's transition rules held to the
oracle: a breadth-first search whose only transition function is OracleEnv itself."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "native"))

import solve_ref as S  # noqa: E402
from marlgrid_amd import _native as N  # noqa: E402

N_GRIDS = 2400


def _kinds():
    import hostemu_solve as HS
    return HS.SolveCase, HS.SolveCase.kinds()


def random_grid(seed):
    """-> (grid (W, H), agent (x, y, d, carry)): 5 .. 7 x 5 .. 7, walled, mostly cut by a wall with doors in it; up to 3 doors
    (open, closed, locked; two colours), up to 3 items (keys, ball, box), lava, floor; the agent with or without something in
    hand"""
    K, _ = _kinds()
    rng = np.random.RandomState(seed)
    W, H = rng.randint(5, 8), rng.randint(5, 8)
    g = np.zeros((W, H), np.uint8)
    g[0, :] = g[-1, :] = g[:, 0] = g[:, -1] = K.WALL
    inner = [(x, y) for x in range(1, W - 1) for y in range(1, H - 1)]
    doors = [K.OPEN_A, K.SHUT_A, K.LOCKED_A, K.OPEN_B, K.SHUT_B, K.LOCKED_B]
    n_doors = rng.randint(0, 4)
    wall_cells = []
    if rng.rand() < 0.7:
        if rng.rand() < 0.5:
            x = rng.randint(2, W - 2)
            wall_cells = [(x, y) for y in range(1, H - 1)]
        else:
            y = rng.randint(2, H - 2)
            wall_cells = [(x, y) for x in range(1, W - 1)]
        for c in wall_cells:
            g[c] = K.WALL
    for c in inner:
        if g[c] == 0:
            r = rng.rand()
            g[c] = K.WALL if r < 0.08 else (K.LAVA if r < 0.12 else (K.FLOOR if r < 0.17 else 0))
    for j in range(n_doors):
        pool = wall_cells if wall_cells and (j == 0 or rng.rand() < 0.6) else inner
        g[pool[rng.randint(len(pool))]] = doors[rng.randint(len(doors))]
    for _ in range(rng.randint(0, 4)):
        c = inner[rng.randint(len(inner))]
        if g[c] in (0, K.FLOOR):
            g[c] = (K.KEY_A, K.KEY_B, K.BALL, K.BOX)[rng.randint(4)]
    free = [c for c in inner if g[c] in (0, K.FLOOR)]
    if len(free) < 2:
        g[1, 1] = g[W - 2, H - 2] = 0
        free = [(1, 1), (W - 2, H - 2)]
    goal = free[rng.randint(len(free))]
    g[goal] = K.GOAL
    free.remove(goal)
    x, y = free[rng.randint(len(free))]
    carry = (0, 0, 0, K.KEY_A, K.KEY_B, K.BALL)[rng.randint(6)]
    return g, (x, y, int(rng.randint(4)), carry)


@pytest.fixture(scope="module")
def grids():
    """the grids by shape, each with the definition's answer"""
    _, kinds = _kinds()
    by_shape = {}
    for seed in range(N_GRIDS):
        g, a = random_grid(seed)
        by_shape.setdefault(g.shape, []).append((g, a, S.full_bfs(g, kinds, *a)))
    return by_shape


def _layered(cases, caps):
    _, kinds = _kinds()
    g = np.stack([c[0] for c in cases])
    a = np.array([c[1] for c in cases])[:, None, :]
    return S.layered(g, kinds, a[..., 0], a[..., 1], a[..., 2], np.ones(a.shape[:2], bool), a[..., 3], *caps)


def test_the_grids_hold_what_they_are_meant_to(grids):
    K, kinds = _kinds()
    cases = [c for v in grids.values() for c in v]
    full = np.array([c[2] for c in cases])
    assert len(cases) == N_GRIDS and len(grids) == 9
    assert (full < 0).sum() > 200 and (full > 0).sum() > 800
    n_doors = np.array([sum(kinds.is_shut_door(int(i)) for i in c[0].ravel()) for c in cases])
    n_items = np.array([sum(kinds.is_item(int(i)) for i in c[0].ravel()) for c in cases])
    assert n_doors.max() == 3 and n_items.max() == 3
    assert sum(1 for c in cases if c[1][3]) > 600                    # agents that start with something in hand
    # grids the static analysis gets wrong: a path exists, and only through a door or past an item
    static = np.array([S.layered(c[0][None], kinds, *[np.array([[v]]) for v in c[1][:3]], np.ones((1, 1), bool),
                                 np.array([[c[1][3]]]), 0, 0)[0][0, 0] for c in cases[:400]])
    assert ((static < 0) & (full[:400] > 0)).sum() > 20


def test_layered_equals_the_definition_when_nothing_is_capped(grids):
    for shape, cases in grids.items():
        dist, act, exact = _layered(cases, (3, 3))
        full = np.array([c[2] for c in cases])
        assert exact.all(), shape
        assert np.array_equal(dist[:, 0], full), (shape, np.flatnonzero(dist[:, 0] != full)[:5])
        assert ((act[:, 0] == S.DONE) == (full < 0)).all(), shape
        assert set(np.unique(act)) <= {0, 1, 2, 3, 5, 6}


def test_capped_values_are_exact_or_upper_bounds(grids):
    capped = 0
    for shape, cases in grids.items():
        dist, _, exact = _layered(cases, (1, 1))
        full = np.array([c[2] for c in cases])
        d = dist[:, 0]
        assert np.array_equal(d[exact], full[exact]), shape
        loose = ~exact
        assert ((d[loose] == -1) | ((full[loose] >= 0) & (d[loose] >= full[loose]))).all(), shape
        capped += int(loose.sum())
    assert capped > 300


def test_the_first_action_leads_one_action_nearer(grids):
    """the policy's contract on the reference itself: apply the action by the definition's rules, and the definition gives one
    less (the first toggle of a locked door: the door is then closed, and still one less)"""
    K, kinds = _kinds()
    checked = 0
    for shape, cases in grids.items():
        dist, act, _ = _layered(cases[:60], (3, 3))
        for (g, (x, y, d, carry), full), dd, a in zip(cases[:60], dist[:, 0], act[:, 0]):
            if full <= 1:
                assert a == (S.FORWARD if full == 1 else S.DONE)
                continue
            g = g.copy()
            fx, fy = x + S.DIRVEC[d][0], y + S.DIRVEC[d][1]
            if a == S.LEFT:
                d = (d + 3) & 3
            elif a == S.RIGHT:
                d = (d + 1) & 3
            elif a == S.FORWARD:
                x, y = fx, fy
            elif a == S.PICKUP:
                assert carry == 0
                carry, g[fx, fy] = int(g[fx, fy]), 0
            else:
                assert a == S.TOGGLE
                i = int(g[fx, fy])
                g[fx, fy] = kinds.unl[i] if kinds.flags[i] & N.OF_DOOR_LOCKED else kinds.tog[i]
            assert S.full_bfs(g, kinds, x, y, d, carry) == full - 1, (shape, a)
            checked += 1
    assert checked > 150


# ---- the definition's rules against the oracle ---------------------------------------------------------------------------------
def _oracle_kinds(cfg):
    o = [cfg.obj[i] for i in range(cfg.n_obj)]
    flags = [(N.OF_CAN_OVERLAP if d.can_overlap else 0) | (N.OF_CAN_PICKUP if d.can_pickup else 0)
             | (N.OF_ENDS_EPISODE if d.ends_episode else 0) | (N.OF_IS_KEY if d.is_key else 0)
             | (N.OF_IS_DOOR if d.toggle_kind == 1 else 0) | (N.OF_IS_BOX if d.toggle_kind == 2 else 0)
             | (N.OF_DOOR_LOCKED if d.toggle_kind == 1 and d.state == 3 else 0) for d in o]
    return S.Kinds(flags, [d.reward_kind for d in o], [d.color_idx for d in o], [d.toggle_next for d in o], [d.unlock_next for d in o])


@pytest.mark.parametrize("seed", range(1337, 1337 + 16))
def test_the_oracle_needs_exactly_as_many_actions(seed):
    """MarlGrid-2AgentDoorKey6x6-v0's level as the oracle lays it out for `seed`: a breadth-first search over agent 0's five
    actions whose transition function is OracleEnv (a fresh env, the action prefix replayed, one more step; agent 1 acts `done`),
    de-duplicated on state().  The first depth at which agent 0 is done is full_bfs's number for the initial state."""
    import draw_envs as D
    from oracle import oracle as O
    spec = D.spec("doorkey", 6, 6, 7, 8, max_steps=100)
    first = O.OracleEnv(spec, seed=seed)
    s0 = first.state()
    kinds = _oracle_kinds(first.cfg)
    want = S.full_bfs(s0["base"], kinds, int(s0["pos"][0, 0]), int(s0["pos"][0, 1]), int(s0["dir"][0]) & 3, int(s0["carrying"][0]))
    assert 0 < want <= 19

    def key(s):
        return (s["base"].tobytes(), tuple(s["pos"][0]), int(s["dir"][0]) & 3, int(s["carrying"][0]))

    seen = {key(s0)}
    frontier = [()]
    found = None
    for depth in range(1, want + 2):
        nxt = []
        for prefix in frontier:
            for a in (0, 1, 2, 3, 5):
                env = O.OracleEnv(spec, seed=seed, _like=first)
                for p in prefix + (a,):
                    env.step([p, 6])
                s = env.state()
                if s["done"][0]:
                    found = depth
                    break
                k = key(s)
                if k not in seen:
                    seen.add(k)
                    nxt.append(prefix + (a,))
            if found:
                break
        if found or not nxt:
            break
        frontier = nxt
    assert found == want, (found, want)
    assert len(seen) <= 2000
