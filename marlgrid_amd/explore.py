"""Exploration maps, host side: `EnvExplore`, what a `MultiGridEnv(explore=True)` keeps (the env holds one as `env._explore`, None
when the option is off): the four tensors — seen, visits, new_cells, visit_count — and the one mg_explore_update launch per view
group that follows every reset() and step().  The kernel is csrc/mg_explore.hip; the semantics are written down in
include/marlgrid_hip.h and in the `MultiGridEnv` properties' docstrings."""
import ctypes as C

from . import _native as N

STATE_KEYS = ("seen", "visits")     # what state_dict() carries of it


class EnvExplore(object):
    """`env._explore`; allocated with the env, rewritten in place by every call"""

    def __init__(self, env):
        import torch
        self.env = env
        B, n, dev = env.batch_size, env.num_agents, env.device
        self.seen_u8 = torch.zeros((B, n, env.width, env.height), dtype=torch.uint8, device=dev)
        self.visits = torch.zeros((B, n, env.width, env.height), dtype=torch.int32, device=dev)
        self.new_cells = torch.zeros((B, n), dtype=torch.int32, device=dev)
        self.visit_count = torch.zeros((B, n), dtype=torch.int32, device=dev)
        self.launches = 0

    @property
    def seen(self):
        import torch
        return self.seen_u8.view(torch.bool)

    def update(self, mask_ptr, stream):
        """one observation more: of the envs a reset's mask selects, or (None) of every env.  Agents that differ in view
        geometry are launched group by group, as `_launch_views` does; a launch writes its own agents' rows only"""
        env = self.env
        st = C.byref(env._state)
        for g in env._groups:
            N.check(env._lib.mg_explore_update(C.byref(g.cfg), st, mask_ptr, self.seen_u8.data_ptr(), self.visits.data_ptr(),
                                               self.new_cells.data_ptr(), self.visit_count.data_ptr(), stream))
            self.launches += 1

    def fork(self, put):
        """env.fork: the four rows go with the rest (`put`: lookahead.py's guarded row copy)"""
        for t in (self.seen_u8, self.visits, self.new_cells, self.visit_count):
            put(t)

    def state(self):
        return {"seen": self.seen.clone(), "visits": self.visits.clone()}

    def keys_of(self, sd):
        """the exploration keys a checkpoint has: both or none (a checkpoint without them loads with cleared maps)"""
        have = set(STATE_KEYS) & set(sd.keys())
        if len(have) == 1:
            raise KeyError("load_state_dict: 'seen' and 'visits' come together")
        return have

    def clear(self):
        for t in (self.seen_u8, self.visits, self.new_cells, self.visit_count):
            t.zero_()
