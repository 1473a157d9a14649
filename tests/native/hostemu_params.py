"""TEST INFRASTRUCTURE — hostemu.HostEmu for reset programs with a PARAM op: the program's template is followed by the
per-env parameter table (`uint8_t params[B][MG_GEN_DRAWS]` at `template_grid + cells_stride`, marlgrid_hip.h), as the
product's `_program` lays it out on the device.  The table is the dry env's `params_t` as it is when the program is built —
every emulated launch builds it again, so a `set_params` between two steps is seen by the next —, or `table` when that is
set (any bytes: the out-of-range case).  A guard band behind the table shows a read or write past it.  Nothing under
marlgrid_amd/ imports it."""
import numpy as np

import hostemu
import hostemu_episode
from marlgrid_amd import _native as N

GUARD = 64


class _WithTable(object):
    table = None

    def _prog(self, trace):
        prog = super()._prog(trace)
        env = self.env
        if any(op[2] == N.GEN_PARAM for op in trace[1]):
            t = np.zeros(env.cells_stride + self.B * N.GEN_DRAWS + GUARD, np.uint8)
            t[:env.cells_stride] = prog._keep
            tab = env.params_t if self.table is None else self.table
            t[env.cells_stride:env.cells_stride + self.B * N.GEN_DRAWS] = np.asarray(tab, np.uint8).reshape(-1)
            t[-GUARD:] = 0xA5
            prog._keep = t
            prog.template_grid = t.ctypes.data
        return prog

    def set_params(self, *a, **kw):
        self.env.set_params(*a, **kw)

    def reseed(self):
        """every env's RNG as the constructor seeded it (`MultiGridEnv.seed()`): the constructor's reset of a parameter env
        ran with the defaults and drew other words than its twins'"""
        from marlgrid_amd import seeding
        keys, lens = seeding.batch_keys(self.env.seeds)
        self.L.emu_mt_seed(self.B, hostemu._ptr(keys), hostemu._ptr(lens), hostemu._ptr(self.mt), hostemu._ptr(self.mt_pos),
                           hostemu._ptr(self.mt_head))


class ParamEmu(_WithTable, hostemu.HostEmu):
    pass


class ParamEpisodeEmu(_WithTable, hostemu_episode.EpisodeEmu):
    pass
