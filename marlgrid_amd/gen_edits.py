"""The per-env edit table of a reset program (`MultiGridEnv(level_edits=K)`, the EDITS op): `env._edits`, which the env holds
next to its ParamTable (gen_params.py).  K entries `(x, y, kind, on)` per env; on the device the table is the tail of the ONE
buffer that an env's programs share — template, `params[B][MG_GEN_DRAWS]`, `edits[B][K][4]` (marlgrid_hip.h) —, read by
`reset_env` at every reset of an env, after everything `_gen_grid` placed and before the agents are placed."""
import numpy as np

from . import _native as N, per_env as P


def check_k(K):
    if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or not 0 <= K <= N.GEN_MAX_EDITS:
        raise ValueError("level_edits: the number of edit entries per env, 0..%d (got %r)" % (N.GEN_MAX_EDITS, K))
    return int(K)


def rows(edits, K, n, ids, B, width, height, n_kinds, device, who):
    """`edits` as (K, 4) or (n, K, 4) uint8 — an array on the host (`device` None) or a tensor of `device` —: (K', 4) for every
    selected env or one list per selected env, K' <= K, the slots from K' on switched off.  `n`: the selected envs (B without
    `ids`; a (B, K', 4) value given with `ids` is gathered by them).  Host values are checked (ValueError); a device tensor is
    only clamped into a byte — the device guards what it reads."""
    if P.on_device(edits, device):
        import torch
        v = edits.to(device)
        _check_shape(tuple(v.shape), K, n, B, who)
        v = v.clamp(0, 255).to(torch.uint8)
        v = torch.cat([v[..., :3], (v[..., 3:] != 0).to(torch.uint8)], dim=-1)
        if v.shape[-2] < K:
            v = torch.cat([v, v.new_zeros(tuple(v.shape[:-2]) + (K - v.shape[-2], 4))], dim=-2)
    else:
        a = np.asarray(edits.cpu() if hasattr(edits, "cpu") else edits)
        if a.size == 0:
            a = np.zeros((0, 4) if a.ndim <= 2 else a.shape[:1] + (0, 4), np.int64)
        a = P.host_ints(a, "%s(edits=)" % who)
        _check_shape(a.shape, K, n, B, who)
        if a.size:
            if a.min() < 0:
                raise ValueError("%s(edits=): an entry is (x, y, kind, on) of non-negative integers" % who)
            for col, lim, what in ((0, width, "x"), (1, height, "y"), (2, n_kinds, "kind")):
                if a[..., col].max() >= lim:
                    raise ValueError("%s(edits=): %s %d outside 0..%d%s" % (who, what, a[..., col].max(), lim - 1,
                                                                           " (the registered kinds: env.edit_key(obj))" if col == 2 else ""))
        v = np.zeros(a.shape[:-2] + (K, 4), np.uint8)
        v[..., :a.shape[-2], :3] = a[..., :3]
        v[..., :a.shape[-2], 3] = a[..., 3] != 0
        v = P.to_device(v, device)
    if ids is not None and v.ndim == 3 and v.shape[0] == B != n:
        v = v[ids]
    return v


def _check_shape(shape, K, n, B, who):
    if len(shape) not in (2, 3) or shape[-1] != 4 or (len(shape) == 3 and shape[0] not in (n, B)):
        raise ValueError("%s(edits=): (K', 4) entries (x, y, kind, on), or one list per selected env, (%d, K', 4); got %s"
                         % (who, n, shape))
    if shape[-2] > K:
        raise ValueError("%s(edits=): %d entries, the env was built with level_edits=%d" % (who, shape[-2], K))


def write(dst, v, mask, ids):
    """rows of a (B, K, 4) table: `per_env.write` with the mask over whole rows"""
    P.write(dst, v, None if mask is None else mask.reshape(-1, 1, 1), ids)


class EditTable(object):
    def __init__(self, env, K):
        self.env = env
        self.K = check_k(K)
        self.table = None       # (B, K, 4) uint8: a view of the tail of the shared buffer (a numpy array when _dry); None at K = 0

    def alloc(self):
        """K > 0: the shared buffer — template, parameter table, edit table — is made here, before anything is recorded; the
        env's ParamTable takes its part of it"""
        env, K = self.env, self.K
        if not K:
            return
        B, cs = env.batch_size, env.cells_stride
        if env._dry:
            self.table = np.zeros((B, K, 4), np.uint8)
            return
        import torch
        par = env._params
        par.buf = torch.zeros(cs + B * N.GEN_DRAWS + B * K * 4, dtype=torch.uint8, device=env.device)
        par.table = par.buf[cs:cs + B * N.GEN_DRAWS].view(B, N.GEN_DRAWS)
        self.table = par.buf[cs + B * N.GEN_DRAWS:].view(B, K, 4)

    def set(self, edits, env_mask=None, env_ids=None):
        """MultiGridEnv.set_edits, whose docstring is the contract"""
        env, B = self.env, self.env.batch_size
        if not self.K:
            raise ValueError("set_edits: this env holds no edit table; construct it with level_edits=K (1..%d)" % N.GEN_MAX_EDITS)
        dev = None if env._dry else env.device
        mask, ids = P.select(B, dev, env_mask, env_ids, "set_edits", any_number=True)
        v = rows(edits, self.K, B if ids is None else int(ids.shape[0]), ids, B, env.width, env.height, len(env.obj_reg.objs),
                 dev, "set_edits")
        write(self.table, v, mask, ids)
