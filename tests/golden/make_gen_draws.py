#!/usr/bin/env python
"""Generate tests/golden/gendraws_<scenario>.npz by EXECUTING THE REAL REFERENCE (imported through refload / refstate, like
make_golden.py) on the scenarios of tests/draw_envs.py, whose `_gen_grid` lays the grid out from `_rand_int` draws
(gym-minigrid's definition: `self.np_random.randint(low, high)`).  Build container only.

    python tests/golden/make_gen_draws.py [scenario ...]

Arrays only, in the key layout of traj_<scenario>.npz (make_golden.py:gen_traj) — seeds, actions, ctor_/reset_/step_ canonical
state, rewards, ep_done, reset_after, order, encode, mt_final(_pos) (the first MT_FULL seeds: 624 words a seed do not compress;
every seed's end state is in rng_step / rng_after_reset); for the scenarios the reference can render also obs_crc*,
obs_full / obs_reset_full (one env) — plus
  rng_ctor [S], rng_reset [S], rng_step [S][T]   draw_envs.rng_digest of the env's RNG: after the constructor, after reset(), after step t
  rng_after_reset [reset_after.sum()]            ... and after the caller-side reset that follows step t, one entry per True of
        reset_after in row-major order (draw_envs.golden gives it back as rng_next [S][T], = rng_step where there was no reset)
  venc_steps [K], venc_ctor_a<k> / venc_reset_a<k> [S][V][V][3], venc_step_a<k> [S][K][V][V][3]
        gen_obs_grid(agent k) + encode(vis_mask), as make_view_encodings.py records them (DoorKey: its pixels cannot be pinned)
and asserts the conditions the fixtures exist for (every split column, gap rows, one-value ranges, rewards, pickups, an
unlocked door; the eight-draw scenario: every register with more than one value, the overhanging place_obj clamped in some
layouts and not in others).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import refload  # noqa: E402
import refstate  # noqa: E402
import draw_envs as D  # noqa: E402

CANON = D.CANON_KEYS
DOOR, KEY, WALL, GOAL = 11, 9, 8, 4         # the type indices of the reference (checked in main)
VENC_EVERY = 6
MT_FULL = 4


def views(env):
    out = []
    for a in env.agents:
        g, vis = env.gen_obs_grid(a)
        out.append(np.asarray(g.encode(vis_mask=vis), np.uint8))
    return out


def rng_of(env):
    st = (env.np_random._rng if isinstance(env.np_random, refstate.OrderSpy) else env.np_random).get_state()
    return D.rng_digest((st[1], st[2]))


def gen(name, out):
    kind, W, H, view, tile, max_steps, pixels = D.SCENARIOS[name]
    S, T, n, P = len(D.SEEDS), D.EPISODES * max_steps, D.N_AGENTS, view * tile
    actions = np.random.RandomState(4242).randint(0, 7, size=(S, T, n)).astype(np.int8)      # uniform over the 7 ids
    d = dict(seeds=D.SEEDS, actions=actions)
    rec, ctor, rst = ({k: [] for k in CANON} for _ in range(3))
    rewards, ep_done, reset_after = np.zeros((S, T, n)), np.zeros((S, T), bool), np.zeros((S, T), bool)
    order, enc = np.zeros((S, T, n), np.int8), np.zeros((S, T, W, H, 3), np.uint8)
    crc, crc_reset, crc_ctor = np.zeros((S, T, n), np.uint32), np.zeros((S, n), np.uint32), np.zeros((S, n), np.uint32)
    obs_full, obs_reset_full = np.zeros((1, T, n, P, P, 3), np.uint8), np.zeros((1, n, P, P, 3), np.uint8)
    mt_final, mt_final_pos = np.zeros((MT_FULL, 624), np.uint32), np.zeros(MT_FULL, np.int32)
    rng_ctor, rng_reset = np.zeros(S, np.uint32), np.zeros(S, np.uint32)
    rng_step, rng_next = np.zeros((S, T), np.uint32), np.zeros((S, T), np.uint32)
    vsteps = np.arange(0, T, VENC_EVERY)
    v_ctor, v_rst = np.zeros((n, S, view, view, 3), np.uint8), np.zeros((n, S, view, view, 3), np.uint8)
    v_stp = np.zeros((n, S, len(vsteps), view, view, 3), np.uint8)
    layouts, draws, stats = [], [], dict(episodes=0, pickup_eps=0, door_eps=0, goal_rewards=0)

    def note_layout(env):
        layouts.append(env.grid.encode()[..., 0].copy())

    for si, seed in enumerate(D.SEEDS):
        env = D.ref_env(kind, W, H, view, tile, max_steps, seed)
        note_layout(env)
        c = refstate.canonical(env)
        for k in CANON:
            ctor[k].append(c[k])
        rng_ctor[si] = rng_of(env)
        v_ctor[:, si] = views(env)
        if pixels:
            crc_ctor[si] = [refstate.crc(x) for x in env.gen_obs()]
        if kind in ("doorkey", "eight"):    # every _rand_int from here on: (low, high, value, the RNG moved)
            def spied(low, high, _env=env, _draw=type(env)._rand_int):
                before = rng_of(_env)
                v = _draw(_env, low, high)
                draws.append((low, high, int(v), rng_of(_env) != before))
                return v
            env._rand_int = spied
        o = env.reset()
        note_layout(env)
        c = refstate.canonical(env)
        for k in CANON:
            rst[k].append(c[k])
        rng_reset[si] = rng_of(env)
        v_rst[:, si] = views(env)
        if pixels:
            crc_reset[si] = [refstate.crc(x) for x in o]
            if si == 0:
                obs_reset_full[0] = np.stack(o)
        spy = refstate.OrderSpy(env.np_random)
        env.np_random = spy
        per = {k: [] for k in CANON}
        picked = unlocked = False
        for t in range(T):
            o, r, dn, _ = env.step(actions[si, t])
            c = refstate.canonical(env)
            for k in CANON:
                per[k].append(c[k])
            rewards[si, t], ep_done[si, t], order[si, t] = r, dn, spy.last
            enc[si, t] = env.grid.encode()
            rng_step[si, t] = rng_next[si, t] = rng_of(env)
            picked |= bool(c["carry_enc"].any())
            door = enc[si, t][enc[si, t][..., 0] == DOOR]
            unlocked |= bool(len(door) and (door[:, 2] != 3).any())
            stats["goal_rewards"] += int((np.asarray(r) > 0).sum())
            if t % VENC_EVERY == 0:
                v_stp[:, si, t // VENC_EVERY] = views(env)
            if pixels:
                crc[si, t] = [refstate.crc(x) for x in o]
                if si == 0:
                    obs_full[0, t] = np.stack(o)
            if dn:
                stats["episodes"] += 1
                stats["pickup_eps"] += picked
                stats["door_eps"] += unlocked
                picked = unlocked = False
                env.reset()
                note_layout(env)
                reset_after[si, t] = True
                rng_next[si, t] = rng_of(env)
        for k in CANON:
            rec[k].append(np.stack(per[k]))
        if si < MT_FULL:
            st = spy._rng.get_state()
            mt_final[si], mt_final_pos[si] = st[1], st[2]
    for k in CANON:
        d["step_" + k], d["ctor_" + k], d["reset_" + k] = np.stack(rec[k]), np.stack(ctor[k]), np.stack(rst[k])
    d.update(rewards=rewards, ep_done=ep_done, reset_after=reset_after, order=order, encode=enc, mt_final=mt_final,
             mt_final_pos=mt_final_pos, rng_ctor=rng_ctor, rng_reset=rng_reset, rng_step=rng_step, rng_after_reset=rng_next[reset_after],
             venc_steps=vsteps)
    if pixels:
        d.update(obs_crc=crc, obs_crc_reset=crc_reset, obs_crc_ctor=crc_ctor, obs_full=obs_full, obs_reset_full=obs_reset_full)
    for k in range(n):
        d["venc_ctor_a%d" % k], d["venc_reset_a%d" % k], d["venc_step_a%d" % k] = v_ctor[k], v_rst[k], v_stp[k]
    # ---- the conditions this fixture exists for ------------------------------------------------------------------------
    assert stats["episodes"] >= EPISODES_MIN * len(D.SEEDS), stats
    L = np.stack(layouts)
    if kind == "split":
        s, gap = D.split_structure(np.where(np.isin(L, (WALL, GOAL)), L, 0), WALL, GOAL)
        assert set(s) == set(range(2, W - 2)), ("split columns", sorted(set(s)))
        assert len(set(gap)) >= 3, ("gap rows", sorted(set(gap)))
        stats.update(split_cols=sorted(set(int(v) for v in s)), gap_rows=sorted(set(int(v) for v in gap)))
    if kind == "doorkey":
        doors = set(zip(*[a.tolist() for a in np.nonzero(L == DOOR)[1:]]))
        one = [d for d in draws if d[1] - d[0] == 1]
        # a one-value range returns its only value and leaves the RNG where it was; every other draw moves it
        assert all(v == lo and not moved for lo, _hi, v, moved in one) and all(moved for d in draws if d[1] - d[0] > 1 for moved in d[3:])
        if W == 5:                          # _rand_int(2, 3): the wall of every 5 x 5 layout is column 2, the door in it
            assert sum(1 for d in one if d[:2] == (2, 3)) == len(L) - len(D.SEEDS)        # (every reset after the constructor's)
            assert (np.isin(L[:, 2, :], (WALL, DOOR))).all() and (np.nonzero(L == DOOR)[1] == 2).all()
        stats.update(door_cells=len(doors), one_value_draws=len(one))
        assert (L == DOOR).reshape(len(L), -1).sum(axis=1).tolist() == [1] * len(L)
    if kind == "eight":                     # eight draws a reset, in register order (draw_envs.py:eight)
        per = np.array([d[2] for d in draws]).reshape(-1, 8)
        assert all(len(set(per[:, r])) >= 2 for r in range(8)), "a register with one value"
        assert (per[:, 6] < 3).any() and (per[:, 6] >= 3).any()         # the overhanging place_obj: clamped / not clamped
        assert (per[:, 4] == per[:, 2]).all() and not any(d[3] for d in draws[4::8])      # _rand_int(c, c + 1): c, no RNG word
        assert (per[:, 2] < per[:, 0]).all() and (per[:, 3] > per[:, 0]).all()            # bounded above / below by a draw
        assert stats["goal_rewards"] >= 1
        stats.update(layouts=len(per), overhang_clamped=int((per[:, 6] < 3).sum()))
    np.savez_compressed(out, **d)
    return stats


EPISODES_MIN = D.EPISODES


def main():
    refload.load()
    from marlgrid.objects import Door, Goal, Key, Wall
    assert (Door("yellow", 3).encode()[0], Key("yellow").encode()[0], Wall().encode()[0], Goal(color="green", reward=1).encode()[0]) \
        == (DOOR, KEY, WALL, GOAL)
    total = dict(pickup_eps=0, door_eps=0, goal_rewards=0, one_value_draws=0)
    for name in sys.argv[1:] or list(D.SCENARIOS):
        out = os.path.join(HERE, "gendraws_%s.npz" % name)
        st = gen(name, out)
        if D.SCENARIOS[name][0] == "doorkey":
            total["pickup_eps"] += st["pickup_eps"]
            total["door_eps"] += st["door_eps"]
            total["one_value_draws"] += st["one_value_draws"]
        else:
            total["goal_rewards"] += st["goal_rewards"]
        print("gendraws", name, os.path.getsize(out), st, flush=True)
    if not sys.argv[1:]:
        # across the files: >= 10 DoorKey episodes with a pickup, >= 1 with the door unlocked, >= 1 goal reward, a one-value range
        assert total["pickup_eps"] >= 10 and total["door_eps"] >= 1 and total["goal_rewards"] >= 1, total
        assert total["one_value_draws"] >= 1, total         # (the 5 x 5 DoorKey's _rand_int(2, 3); checked draw by draw in gen)
    print("conditions hold:", total)


if __name__ == "__main__":
    main()
