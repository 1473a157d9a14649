"""Goal distance, host side: `EnvGoal`, what a MultiGridEnv keeps for `goal_distance` / `optimal_return` (the env holds one as
`env._goal`, as it holds `env._levels`): the two result tensors and the one mg_goal_distance launch.  The kernels are
csrc/mg_goal_dist.hip; the semantics are written down in include/marlgrid_hip.h."""
import ctypes as C

from . import _native as N, per_env as P
from .objects import Goal

PATHS = {None: N.GOAL_PATH_AUTO, "auto": N.GOAL_PATH_AUTO, "reg": N.GOAL_PATH_REG, "lds": N.GOAL_PATH_LDS}


class EnvGoal(object):
    """`env._goal`; MultiGridEnv.goal_distance / optimal_return, whose docstrings are the contract, delegate here.  Nothing is
    allocated or launched until `distance` is first called."""

    def __init__(self, env):
        self.env = env
        self.dist = None            # (B, n) int32, -1 until an env is first analysed
        self.field = None           # (B, W, H, 4) int32, made at the first call with field=True
        self.launches = 0
        self._mask_keep = None

    def distance(self, env_mask=None, env_ids=None, field=False, _path=None):
        import torch
        env = self.env
        if env._dry:
            raise RuntimeError("goal_distance runs on the device; a _dry env has none")
        B, dev = env.batch_size, env.device
        mask, ids = P.select(B, dev, env_mask, env_ids, "goal_distance")
        if ids is not None:
            # the launch takes a mask: the listed envs, in stream order, nothing read back.  Host ids were range-checked; an id of
            # a device tensor that lies outside the batch goes to a spare slot behind the mask and selects nothing
            spare = torch.where((ids >= 0) & (ids < B), ids, torch.full_like(ids, B))
            mask = torch.zeros(B + 1, dtype=torch.uint8, device=dev).index_fill_(0, spare, 1)[:B]
        if self.dist is None:
            self.dist = torch.full((B, env.num_agents), -1, dtype=torch.int32, device=dev)
        if field and self.field is None:
            self.field = torch.full((B, env.width, env.height, 4), -1, dtype=torch.int32, device=dev)
        env._sync_tables()
        self._mask_keep = mask      # (alive until the next call's mask replaces it: the launch is asynchronous)
        args = (C.byref(env._cfg), C.byref(env._state), None if mask is None else mask.data_ptr(), self.dist.data_ptr(),
                self.field.data_ptr() if field else None)
        if _path is None:
            N.check(env._lib.mg_goal_distance(*args, env._stream()))
        else:
            N.check(env._lib.mg_goal_distance_path(*args, PATHS[_path], env._stream()))
        self.launches += 1
        return (self.dist, self.field) if field else self.dist

    def goal_reward(self):
        """the reward the registered Goal kinds share"""
        rewards = sorted({float(o.reward) for o in self.env.obj_reg.objs if isinstance(o, Goal)})
        if len(rewards) != 1:
            raise ValueError("optimal_return: %s" % ("no Goal kind is registered" if not rewards else
                                                     "the registered Goal kinds differ in their reward (%s)" % rewards))
        return rewards[0]

    def optimal_return(self, dist=None):
        import torch
        env = self.env
        R = self.goal_reward()
        d = self.distance() if dist is None else dist
        t = env.step_count_t.unsqueeze(1).to(torch.int64) + d.to(torch.int64)
        value = torch.full(t.shape, R, dtype=torch.float64, device=t.device)
        if env.reward_decay:
            value = R * (1.0 - 0.9 * (t.to(torch.float64) / float(env.max_steps)))
        return torch.where((d < 0) | (t > env.max_steps), torch.zeros_like(value), value)
