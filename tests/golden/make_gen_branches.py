#!/usr/bin/env python
"""Generate tests/golden/genbranch_<scenario>.npz by EXECUTING THE REAL REFERENCE (imported through refload / refstate, like
make_gen_draws.py) on the scenarios of tests/gen_branch_envs.py, whose `_gen_grid` branches on random draws (`_rand_elem`,
`_rand_bool` as gym-minigrid defines them; `_fork` hands its argument back).  Build container only.

    python tests/golden/make_gen_branches.py [scenario ...]

Arrays only, in the key layout of gendraws_<scenario>.npz (make_gen_draws.py), plus the path every reset took, an index into
gen_branch_envs.paths(kind):
  path_ctor [S], path_reset [S]       the constructor's reset, the first reset()
  path_after_reset [reset_after.sum()]  the caller-side reset that follows step t, one entry per True of reset_after, row-major
and asserts the condition the fixtures exist for: every path of the scenario occurs in at least one reset AFTER the
constructor's (path_reset and path_after_reset together).
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
import gen_branch_envs as G  # noqa: E402

CANON = D.CANON_KEYS
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
    kind, W, H, view, tile, max_steps, pixels = G.SCENARIOS[name]
    S, T, n, P = len(G.SEEDS), G.EPISODES * max_steps, G.N_AGENTS, view * tile
    actions = np.random.RandomState(4243).randint(0, 7, size=(S, T, n)).astype(np.int8)
    d = dict(seeds=G.SEEDS, actions=actions)
    rec, ctor, rst = ({k: [] for k in CANON} for _ in range(3))
    rewards, ep_done, reset_after = np.zeros((S, T, n)), np.zeros((S, T), bool), np.zeros((S, T), bool)
    order, enc = np.zeros((S, T, n), np.int8), np.zeros((S, T, W, H, 3), np.uint8)
    crc, crc_reset, crc_ctor = np.zeros((S, T, n), np.uint32), np.zeros((S, n), np.uint32), np.zeros((S, n), np.uint32)
    obs_full, obs_reset_full = np.zeros((1, T, n, P, P, 3), np.uint8), np.zeros((1, n, P, P, 3), np.uint8)
    mt_final, mt_final_pos = np.zeros((MT_FULL, 624), np.uint32), np.zeros(MT_FULL, np.int32)
    rng_ctor, rng_reset = np.zeros(S, np.uint32), np.zeros(S, np.uint32)
    rng_step, rng_next = np.zeros((S, T), np.uint32), np.zeros((S, T), np.uint32)
    path_ctor, path_reset, path_next = np.zeros(S, np.int16), np.zeros(S, np.int16), np.full((S, T), -1, np.int16)
    vsteps = np.arange(0, T, VENC_EVERY)
    v_ctor, v_rst = np.zeros((n, S, view, view, 3), np.uint8), np.zeros((n, S, view, view, 3), np.uint8)
    v_stp = np.zeros((n, S, len(vsteps), view, view, 3), np.uint8)
    stats = dict(episodes=0, goal_rewards=0)

    for si, seed in enumerate(G.SEEDS):
        env = G.ref_env(kind, W, H, view, tile, max_steps, seed)
        path_ctor[si] = G.take_path(env, kind, W)
        c = refstate.canonical(env)
        for k in CANON:
            ctor[k].append(c[k])
        rng_ctor[si] = rng_of(env)
        v_ctor[:, si] = views(env)
        if pixels:
            crc_ctor[si] = [refstate.crc(x) for x in env.gen_obs()]
        o = env.reset()
        path_reset[si] = G.take_path(env, kind, W)
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
        for t in range(T):
            o, r, dn, _ = env.step(actions[si, t])
            c = refstate.canonical(env)
            for k in CANON:
                per[k].append(c[k])
            rewards[si, t], ep_done[si, t], order[si, t] = r, dn, spy.last
            enc[si, t] = env.grid.encode()
            rng_step[si, t] = rng_next[si, t] = rng_of(env)
            stats["goal_rewards"] += int((np.asarray(r) > 0).sum())
            if t % VENC_EVERY == 0:
                v_stp[:, si, t // VENC_EVERY] = views(env)
            if pixels:
                crc[si, t] = [refstate.crc(x) for x in o]
                if si == 0:
                    obs_full[0, t] = np.stack(o)
            if dn:
                stats["episodes"] += 1
                env.reset()
                path_next[si, t] = G.take_path(env, kind, W)
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
             venc_steps=vsteps, path_ctor=path_ctor, path_reset=path_reset, path_after_reset=path_next[reset_after])
    if pixels:
        d.update(obs_crc=crc, obs_crc_reset=crc_reset, obs_crc_ctor=crc_ctor, obs_full=obs_full, obs_reset_full=obs_reset_full)
    for k in range(n):
        d["venc_ctor_a%d" % k], d["venc_reset_a%d" % k], d["venc_step_a%d" % k] = v_ctor[k], v_rst[k], v_stp[k]
    # ---- the conditions this fixture exists for ------------------------------------------------------------------------
    assert stats["episodes"] >= G.EPISODES * S, stats
    seen = set(path_reset.tolist()) | set(path_next[reset_after].tolist())
    assert seen == set(range(len(G.paths(kind, W)))), ("paths never taken by a reset after the constructor's",
                                                       sorted(set(range(len(G.paths(kind, W)))) - seen))
    stats["paths"] = len(seen)
    np.savez_compressed(out, **d)
    return stats


def main():
    refload.load()
    for name in sys.argv[1:] or list(G.SCENARIOS):
        out = os.path.join(HERE, "genbranch_%s.npz" % name)
        st = gen(name, out)
        print("genbranch", name, os.path.getsize(out), st, flush=True)


if __name__ == "__main__":
    main()
