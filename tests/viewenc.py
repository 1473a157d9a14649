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
