"""TEST INFRASTRUCTURE — hostemu.HostEmu for reset programs with an EDITS op: the program's template is followed by the
parameter table and, directly behind it, the per-env edit table (`uint8_t edits[B][K][4]` at `template_grid + cells_stride +
B * MG_GEN_DRAWS`, marlgrid_hip.h), as the product's `_program` lays them out on the device.  The edit table is the dry env's
`edits_t` as it is when the program is built — every emulated launch builds it again, so a `set_edits` between two steps is
seen by the next —, or `edit_table` when that is set (any bytes: the out-of-range case).  A guard band behind the table shows a
read or write past it.  Nothing under marlgrid_amd/ imports it."""
import numpy as np

import hostemu
import hostemu_params
from marlgrid_amd import _native as N

GUARD = 64


class EditsEmu(hostemu_params._WithTable, hostemu.HostEmu):
    edit_table = None

    def _prog(self, trace):
        prog = super()._prog(trace)       # (a program with a PARAM op and no EDITS op: template and parameter table)
        env = self.env
        if any(op[2] == N.GEN_EDITS for op in trace[1]):
            K, cs, npar = env.level_edits, env.cells_stride, self.B * N.GEN_DRAWS
            t = np.zeros(cs + npar + self.B * K * 4 + GUARD, np.uint8)
            t[:cs] = prog._keep[:cs]
            par = env.params_t if self.table is None else self.table
            if par is not None:
                t[cs:cs + npar] = np.asarray(par, np.uint8).reshape(-1)
            tab = env.edits_t if self.edit_table is None else self.edit_table
            t[cs + npar:cs + npar + self.B * K * 4] = np.asarray(tab, np.uint8).reshape(-1)
            t[-GUARD:] = 0xA5
            prog._keep = t
            prog.template_grid = t.ctypes.data
        return prog

    def set_edits(self, *a, **kw):
        self.env.set_edits(*a, **kw)
