"""Goal distance, host side: `EnvGoal`, what a MultiGridEnv keeps for `goal_distance` / `solve_distance` / `optimal_return` (the
env holds one as `env._goal`, as it holds `env._levels`): the result tensors and the one mg_goal_distance or mg_solve_distance
launch of a call.  The kernels are csrc/mg_goal_dist.hip and csrc/mg_solve_dist.hip; the semantics are written down in
include/marlgrid_hip.h."""
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
        self.solve_dist = None      # (B, n) int32 / int8 / (B,) uint8, made at the first solve_distance call
        self.solve_act8 = None
        self.solve_action = None    # (B, n) int64, made at the first call with policy=True
        self.exact_u8 = None
        self._solve_mask_keep = None

    def _mask(self, env_mask, env_ids, who):
        """the launch's mask (None: every env) from the call's selectors"""
        import torch
        env = self.env
        if env._dry:
            raise RuntimeError("%s runs on the device; a _dry env has none" % who)
        B, dev = env.batch_size, env.device
        mask, ids = P.select(B, dev, env_mask, env_ids, who)
        if ids is not None:
            # the launch takes a mask: the listed envs, in stream order, nothing read back.  Host ids were range-checked; an id of
            # a device tensor that lies outside the batch goes to a spare slot behind the mask and selects nothing
            spare = torch.where((ids >= 0) & (ids < B), ids, torch.full_like(ids, B))
            mask = torch.zeros(B + 1, dtype=torch.uint8, device=dev).index_fill_(0, spare, 1)[:B]
        return mask

    def distance(self, env_mask=None, env_ids=None, field=False, _path=None):
        import torch
        env = self.env
        mask = self._mask(env_mask, env_ids, "goal_distance")
        B, dev = env.batch_size, env.device
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

    @property
    def exact(self):
        import torch
        return None if self.exact_u8 is None else self.exact_u8.view(torch.bool)

    @staticmethod
    def solve_caps_that_fit(W, H):
        """the (max_doors, max_items) pairs whose layers fit LDS for a W x H grid, none of them under another"""
        fits = [(d, k) for d in range(N.SOLVE_MAX_DOORS + 1) for k in range(N.SOLVE_MAX_ITEMS + 1)
                if N.lib().mg_solve_distance_lds_bytes(W, H, d, k) <= N.SOLVE_LDS_LIMIT]
        return [(d, k) for d, k in fits if not any((d2 >= d and k2 >= k and (d2, k2) != (d, k)) for d2, k2 in fits)]

    def solve(self, env_mask=None, env_ids=None, max_doors=2, max_items=2, policy=False):
        import torch
        env = self.env
        mask = self._mask(env_mask, env_ids, "solve_distance")
        max_doors, max_items = int(max_doors), int(max_items)
        if not (0 <= max_doors <= N.SOLVE_MAX_DOORS and 0 <= max_items <= N.SOLVE_MAX_ITEMS):
            raise ValueError("solve_distance: max_doors is 0 .. %d and max_items 0 .. %d, got (%d, %d)"
                             % (N.SOLVE_MAX_DOORS, N.SOLVE_MAX_ITEMS, max_doors, max_items))
        W, H = env.width, env.height
        need = env._lib.mg_solve_distance_lds_bytes(W, H, max_doors, max_items)
        if need > N.SOLVE_LDS_LIMIT:        # (what the launch would answer with MG_E_UNSUPPORTED: said here, with the way out)
            raise NotImplementedError(
                "solve_distance: max_doors=%d, max_items=%d need %d bytes of LDS per env on a %d x %d grid, %d are there; caps that "
                "fit: %s" % (max_doors, max_items, need, W, H, N.SOLVE_LDS_LIMIT,
                             ", ".join("(%d, %d)" % c for c in self.solve_caps_that_fit(W, H)) or "none"))
        B, dev = env.batch_size, env.device
        if self.solve_dist is None:
            self.solve_dist = torch.full((B, env.num_agents), -1, dtype=torch.int32, device=dev)
            self.solve_act8 = torch.full((B, env.num_agents), 6, dtype=torch.int8, device=dev)
            self.exact_u8 = torch.zeros(B, dtype=torch.uint8, device=dev)
        env._sync_tables()
        self._solve_mask_keep = mask        # (alive until the next call's mask replaces it: the launch is asynchronous)
        N.check(env._lib.mg_solve_distance(C.byref(env._cfg), C.byref(env._state), None if mask is None else mask.data_ptr(),
                                           max_doors, max_items, self.solve_dist.data_ptr(), self.solve_act8.data_ptr(),
                                           self.exact_u8.data_ptr(), env._stream()))
        self.launches += 1
        if not policy:
            return self.solve_dist
        if self.solve_action is None:
            self.solve_action = torch.empty((B, env.num_agents), dtype=torch.int64, device=dev)
        self.solve_action.copy_(self.solve_act8)
        return self.solve_dist, self.solve_action

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
