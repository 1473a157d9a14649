"""Exploration maps, host side: `EnvExplore`, what a `MultiGridEnv(explore=True)` keeps (the env holds one as `env._explore`, None
when the option is off): the four tensors — seen, visits, new_cells, visit_count — and the one mg_explore_update launch per view
group that follows every reset() and step().  The kernel is csrc/mg_explore.hip; the semantics are written down in
include/marlgrid_hip.h and in the `MultiGridEnv` properties' docstrings.

`MultiGridEnv(memory=True)` (it implies explore=True) adds two tensors — memory, seen_step: each agent's last view of every
cell and when it had it — and launches mg_memory_update INSTEAD: the same kernel with the memory compiled in, so the view
chain runs once for all six."""
import ctypes as C

from . import _native as N

STATE_KEYS = ("seen", "visits")     # what state_dict() carries of it
MEMORY_KEYS = ("memory", "seen_step")   # ... and of a memory=True env's two more


class EnvExplore(object):
    """`env._explore`; allocated with the env, rewritten in place by every call"""

    def __init__(self, env, memory=False):
        import torch
        self.env = env
        self.memory = self.seen_step = None
        B, n, dev = env.batch_size, env.num_agents, env.device
        self.seen_u8 = torch.zeros((B, n, env.width, env.height), dtype=torch.uint8, device=dev)
        self.visits = torch.zeros((B, n, env.width, env.height), dtype=torch.int32, device=dev)
        self.new_cells = torch.zeros((B, n), dtype=torch.int32, device=dev)
        self.visit_count = torch.zeros((B, n), dtype=torch.int32, device=dev)
        if memory:      # (type, colour, state, known) per cell: one aligned dword; the step count of the last sighting, -1: never
            self.memory = torch.zeros((B, n, env.width, env.height, 4), dtype=torch.uint8, device=dev)
            self.seen_step = torch.full((B, n, env.width, env.height), -1, dtype=torch.int32, device=dev)
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
        four = (self.seen_u8.data_ptr(), self.visits.data_ptr(), self.new_cells.data_ptr(), self.visit_count.data_ptr())
        for g in env._groups:
            if self.memory is None:
                N.check(env._lib.mg_explore_update(C.byref(g.cfg), st, mask_ptr, *four, stream))
            else:       # the one launch that does both
                N.check(env._lib.mg_memory_update(C.byref(g.cfg), st, mask_ptr, *four, self.memory.data_ptr(),
                                                  self.seen_step.data_ptr(), stream))
            self.launches += 1

    def fork(self, put):
        """env.fork: the four rows (six with the memory) go with the rest (`put`: lookahead.py's guarded row copy)"""
        for t in (self.seen_u8, self.visits, self.new_cells, self.visit_count):
            put(t)
        if self.memory is not None:
            put(self.memory)
            put(self.seen_step)

    def state(self):
        sd = {"seen": self.seen.clone(), "visits": self.visits.clone()}
        if self.memory is not None:
            sd.update(memory=self.memory.clone(), seen_step=self.seen_step.clone())
        return sd

    def keys_of(self, sd):
        """the exploration keys a checkpoint has: both or none (a checkpoint without them loads with cleared maps)"""
        have = set(STATE_KEYS) & set(sd.keys())
        if len(have) == 1:
            raise KeyError("load_state_dict: 'seen' and 'visits' come together")
        if self.memory is not None:     # a memory=True env: its two come together too; without the option they are not read
            mem = set(MEMORY_KEYS) & set(sd.keys())
            if len(mem) == 1:
                raise KeyError("load_state_dict: 'memory' and 'seen_step' come together")
            have |= mem
        return have

    def complete(self, have):
        """does a checkpoint with the keys `have` carry every map this env keeps?  (if not, load_state_dict clears them all:
        memory[..., 3] == seen and (seen_step >= 0) == seen hold after every call)"""
        return have == set(STATE_KEYS + (MEMORY_KEYS if self.memory is not None else ()))

    def clear(self):
        for t in (self.seen_u8, self.visits, self.new_cells, self.visit_count):
            t.zero_()
        if self.memory is not None:
            self.memory.zero_()
            self.seen_step.fill_(-1)
