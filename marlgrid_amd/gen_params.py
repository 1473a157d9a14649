"""The per-env parameter table of `_gen_grid` (`self._param`, the PARAM op of a reset program): `env._params`, which the env holds
as it holds the recorder (`env._gen`).  One byte column per distinct name, a row per env; on the device the table is the tail of
ONE buffer whose head is the template of every program with a PARAM op (MultiGridEnv._program lays it out)."""
import numpy as np

from . import _native as N, per_env as P


class ParamTable(object):
    def __init__(self, env):
        self.env = env
        self.decl = {}          # `_param` names of this env's `_gen_grid`: name -> dict(col, lo, hi, default); columns stay
        self.buf = None         # the template of a program with a PARAM op and, behind it, the table (marlgrid_hip.h)
        self.tpl = None         # ... the template bytes the buffer holds now
        self.table = None       # the table: (B, MG_GEN_DRAWS) uint8 — a view of the buffer's tail (a numpy array when _dry)

    def column(self, name, low, high, default):
        """the table column of parameter `name`: its own from the first time `_gen_grid` names it on, filled with `default`
        then; the values set since survive every later recording"""
        env, d = self.env, self.decl.get(name)
        if d is None:
            if len(self.decl) >= N.GEN_DRAWS:
                raise NotImplementedError("_gen_grid has named more than %d parameters: the table has %d columns (MG_GEN_DRAWS)"
                                          % (N.GEN_DRAWS, N.GEN_DRAWS))
            if self.table is None and env._dry:
                self.table = np.zeros((env.batch_size, N.GEN_DRAWS), np.uint8)
            elif self.table is None:
                import torch
                self.buf = torch.zeros(env.cells_stride + env.batch_size * N.GEN_DRAWS, dtype=torch.uint8, device=env.device)
                self.table = self.buf[env.cells_stride:].view(env.batch_size, N.GEN_DRAWS)
            d = self.decl[name] = dict(col=len(self.decl), lo=low, hi=high, default=default)
            self.table[:, d["col"]] = default
        else:
            d.update(lo=low, hi=high, default=default)      # (what the table holds is clamped to the interval where it is loaded)
        return d["col"]

    def set(self, env_mask=None, env_ids=None, **values):
        """MultiGridEnv.set_params, whose docstring is the contract"""
        env, B = self.env, self.env.batch_size
        dev = None if env._dry else env.device
        mask, ids = P.select(B, dev, env_mask, env_ids, "set_params", any_number=True)
        env._ensure_recorded()
        for name in values:
            if name not in self.decl:
                raise KeyError("set_params: %r is no parameter of this env's _gen_grid (declared: %s)"
                               % (name, ", ".join(sorted(self.decl)) or "none"))
        for name, v in values.items():
            d = self.decl[name]
            v = P.values(v, d["lo"], d["hi"], B, ids, dev, "set_params(%s=)" % name,
                         "the parameter's interval [%d, %d)" % (d["lo"], d["hi"]), dtype=np.uint8, wide=False, clamp=True)
            P.write(self.table[:, d["col"]], v, mask, ids)
