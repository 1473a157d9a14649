#!/usr/bin/env python
"""Generate tests/golden/genedits_<list>.npz by EXECUTING THE REAL REFERENCE (imported through refload / refstate, like
make_gen_branches.py) on tests/level_envs.py:ref_env — the reference's ClutteredMultiGrid 15 x 15 with a `_gen_grid` of ours on
top that ends with the per-instance list `for x, y, o in self.level: ...` —, for the lists of level_envs.PINNED.  Build
container only.

    python tests/golden/make_gen_edits.py [list ...]

Arrays only: seeds [S], actions [S, T, n] and the list itself (`level` [n_entries, 3]); the canonical state fields after the
first reset() (`reset_<field>` [S, ...]) and after every step (`step_<field>` [S, T, ...]); rewards, ep_done, the shuffle
order, MultiGrid.encode() [S, T, W, H, 3], the agents' view encodings every VENC_EVERY-th step, a digest of the RNG after
the reset, after every step and after the caller-side reset that follows a done step (`reset_after`), the final MT19937 words
of the first seed, and — where the reference can draw every kind of the list — a crc of every agent's observation.
The constructor's reset is not recorded: it runs before the list exists."""
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
import level_envs as LE  # noqa: E402

CANON = D.CANON_KEYS
VENC_EVERY = 6


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
    level, pixels = LE.PINNED[name]
    S, T, n = len(LE.PIN_SEEDS), LE.PIN_STEPS, LE.N_AGENTS
    actions = np.random.RandomState(4244).randint(0, 7, size=(S, T, n)).astype(np.int8)
    d = dict(seeds=LE.PIN_SEEDS, actions=actions, level=np.asarray(level, np.int16).reshape(-1, 3))
    rec, rst = ({k: [] for k in CANON} for _ in range(2))
    rewards, ep_done = np.zeros((S, T, n)), np.zeros((S, T), bool)
    order, enc = np.zeros((S, T, n), np.int8), np.zeros((S, T, LE.W, LE.H, 3), np.uint8)
    crc, crc_reset = np.zeros((S, T, n), np.uint32), np.zeros((S, n), np.uint32)
    rng_reset, rng_step, rng_next = np.zeros(S, np.uint32), np.zeros((S, T), np.uint32), np.zeros((S, T), np.uint32)
    vsteps = np.arange(0, T, VENC_EVERY)
    v_rst = np.zeros((n, S, LE.VIEW, LE.VIEW, 3), np.uint8)
    v_stp = np.zeros((n, S, len(vsteps), LE.VIEW, LE.VIEW, 3), np.uint8)
    stats = dict(episodes=0, picked_up=0)
    for si, seed in enumerate(LE.PIN_SEEDS):
        env = LE.ref_env(seed, level, render=pixels)
        o = env.reset()
        c = refstate.canonical(env)
        for k in CANON:
            rst[k].append(c[k])
        rng_reset[si] = rng_of(env)
        v_rst[:, si] = views(env)
        if pixels:
            crc_reset[si] = [refstate.crc(x) for x in o]
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
            stats["picked_up"] += int(c["carry_enc"].any())
            if t % VENC_EVERY == 0:
                v_stp[:, si, t // VENC_EVERY] = views(env)
            if pixels:
                crc[si, t] = [refstate.crc(x) for x in o]
            if dn:
                stats["episodes"] += 1
                env.reset()
                rng_next[si, t] = rng_of(env)
        for k in CANON:
            rec[k].append(np.stack(per[k]))
        if si == 0:
            st = spy._rng.get_state()
            d["mt_final"], d["mt_final_pos"] = np.asarray(st[1], np.uint32), np.int32(st[2])
    for k in CANON:
        d["step_" + k], d["reset_" + k] = np.stack(rec[k]), np.stack(rst[k])
    d.update(rewards=rewards, ep_done=ep_done, order=order, encode=enc, rng_reset=rng_reset, rng_step=rng_step,
             rng_after_reset=rng_next[ep_done], venc_steps=vsteps)
    if pixels:
        d.update(obs_crc=crc, obs_crc_reset=crc_reset)
    for k in range(n):
        d["venc_reset_a%d" % k], d["venc_step_a%d" % k] = v_rst[k], v_stp[k]
    assert stats["episodes"] >= 3 * S, stats
    np.savez_compressed(out, **d)
    return stats


def main():
    refload.load()
    for name in sys.argv[1:] or list(LE.PINNED):
        out = os.path.join(HERE, "genedits_%s.npz" % name)
        st = gen(name, out)
        print("genedits", name, os.path.getsize(out), st, flush=True)


if __name__ == "__main__":
    main()
