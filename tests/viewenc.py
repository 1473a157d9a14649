"""Shared by the encoded-view tests: the oracle's composition of gen_obs_grid(agent) -> grid.encode(vis_mask) (mgo_view's
post-hide_item_types top codes and visibility, each top code mapped to its triple as mgo_encode maps it), and the
reference fixtures tests/golden/viewenc_*.npz (tests/golden/make_view_encodings.py)."""
import glob
import os

import numpy as np

from oracle import oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def fixtures():
    return sorted(os.path.basename(p)[len("viewenc_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "viewenc_*.npz")))


def load(name):
    return np.load(os.path.join(GOLDEN, "viewenc_%s.npz" % name))


def _owner(e, k):
    """the oracle env that sees with agent k's geometry (OracleEnvViews: one env per geometry)"""
    return e.envs[e.owner[k]] if isinstance(e, O.OracleEnvViews) else e


def oracle_views(e):
    """[n] arrays (V_k, V_k, 3): agent k's gen_obs_grid -> encode on oracle env `e` (OracleEnv or OracleEnvViews)"""
    base = _owner(e, 0)
    cfg, n = base.cfg, base.n
    tab = np.zeros((1000 + 32, 3), np.uint8)     # top code -> triple: object ids below 1000, agent x at 1000 + x
    for o in range(1, cfg.n_obj):
        tab[o] = (cfg.obj[o].type_idx, cfg.obj[o].color_idx, cfg.obj[o].state)
    dirs = base.state()["dir"]
    for x in range(n):
        tab[1000 + x] = (cfg.agent_type_idx, cfg.agent_color_idx[x], dirs[x])
    out = []
    for k in range(n):
        vis, cells = _owner(e, k).view(k)
        out.append(np.where(vis[..., None], tab[cells], 0).astype(np.uint8))
    return out


def oracle_views_batch(envs):
    """oracle_views of many plain OracleEnvs (one scenario, one view geometry) -> (len(envs), n, V, V, 3): the table of
    object triples is built once, the agents' rows (their direction is the state field) are filled in env by env"""
    import ctypes as C
    e0 = envs[0]
    assert not isinstance(e0, O.OracleEnvViews)
    cfg, n, V, m = e0.cfg, e0.n, e0.vs, len(envs)
    tab = np.zeros((1000, 3), np.uint8)
    for o in range(1, cfg.n_obj):
        tab[o] = (cfg.obj[o].type_idx, cfg.obj[o].color_idx, cfg.obj[o].state)
    color = np.array([cfg.agent_color_idx[x] for x in range(n)], np.uint8)
    vis = np.zeros((m, n, V, V), np.uint8)
    cells = np.zeros((m, n, V, V), np.int32)
    dirs = np.zeros((m, n), np.uint8)
    u8p, i32p = C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
    for i, e in enumerate(envs):
        for k in range(n):
            e.L.mgo_view(e.h, k, vis[i, k].ctypes.data_as(u8p), cells[i, k].ctypes.data_as(i32p))
        dirs[i] = e.state()["dir"]
    agent = cells >= 1000
    out = tab[np.where(agent, 0, cells)]
    ii, _, _, _ = np.nonzero(agent)
    x = cells[agent] - 1000
    out[agent] = np.stack([np.full(x.shape, cfg.agent_type_idx, np.uint8), color[x], dirs[ii, x]], axis=1)
    return np.where(vis[..., None] != 0, out, 0).astype(np.uint8)
