"""TEST INFRASTRUCTURE — hostemu.HostEmu stepped through an MgEpisode: the step bodies of marlgrid_amd/csrc/mg_core.h with
next-step / same-step reset and the episode outputs, on the host (libmg_hostemu.so's emu_step / emu_step_par with their
`ep` argument set).  Nothing under marlgrid_amd/ imports it.
"""
import ctypes as C

import numpy as np

import hostemu
from marlgrid_amd import _native as N


def lib():
    L = hostemu.lib()
    assert L.emu_ep_sizeof() == C.sizeof(N.Episode), (L.emu_ep_sizeof(), C.sizeof(N.Episode))
    return L


class EpisodeEmu(hostemu.HostEmu):
    """mode: "next_step" | "same_step" (needs the reset program: auto_reset) | None (no reset, accumulators only)"""

    def __init__(self, name, B, seeds, mode="next_step", par=False, **kw):
        lib()
        hostemu.HostEmu.__init__(self, name, B, seeds, auto_reset=mode is not None, par=par, **kw)
        self.ep_return = np.zeros((B, self.n), np.float64)
        self.out_return = np.full((B, self.n), np.nan, np.float64)
        self.out_length = np.full(B, -1, np.int32)
        self.out_flags = np.full(B, 0xFF, np.uint8)
        self.ep = N.Episode(N.RESET_NEXT_STEP if mode == "next_step" else N.RESET_SAME_STEP, 0,
                            self.ep_return.ctypes.data, self.out_return.ctypes.data, self.out_length.ctypes.data,
                            self.out_flags.ctypes.data)

    def step(self, actions):
        self._step(actions, C.byref(self.ep))
        f = self.out_flags
        info = dict(terminated=(f & N.EPF_TERMINATED) != 0, truncated=(f & N.EPF_TRUNCATED) != 0, reset=(f & N.EPF_RESET) != 0,
                    episode_return=self.out_return.copy(), episode_length=self.out_length.copy())
        return self.rewards.copy(), self.done.astype(bool), info
