"""Lookahead, host side: `EnvLookahead`, what a MultiGridEnv keeps for `lookahead` / `fork` (the env holds one as `env._look`, as it
holds `env._goal` and `env._levels`): the SHADOW state — a second MgState of R = K * m rows, named as the env's own tensors —, the
result tensors, and the two launches of a call (mg_fork_rows, mg_rollout).  The kernels are csrc/mg_lookahead.hip; the semantics
are written down in include/marlgrid_hip.h."""
import ctypes as C

import numpy as np

from . import _native as N, per_env as P

# bytes of a shadow row besides the grid slice and the records: generator, head, mt_pos, step count, done, error
ROW_FIXED_BYTES = N.MT_N * 4 + N.MT_HEAD * 4 + 4 + 4 + 1 + 4


def row_bytes(cells_stride, n_agents, prestige=False):
    """the footprint of one shadow row: cells_stride + 8 n + 2496 + 64 + 4 + 4 + 1 + 4 bytes, plus 8 n with 'prestige' agents"""
    return cells_stride + 8 * n_agents + ROW_FIXED_BYTES + (8 * n_agents if prestige else 0)


class _Rows(object):
    """`rows` rows of MgState tensors, named as the env's, and the MgState that points at them (error_flag NULL)"""
    KEYS = ("grid_state", "agent_state", "mt_state", "mt_pos", "mt_head", "step_count_t", "done_t", "error_t", "prestige_t")

    def __init__(self, env, rows):
        import torch
        n, dev = env.num_agents, env.device
        self.rows = rows
        self.grid_state = torch.zeros((rows, env.cells_stride), dtype=torch.uint8, device=dev)
        self.agent_state = torch.zeros((rows, n), dtype=torch.int64, device=dev)
        self.mt_state = torch.zeros((rows, N.MT_N), dtype=torch.int32, device=dev)
        self.mt_pos = torch.zeros((rows,), dtype=torch.int32, device=dev)
        self.mt_head = torch.zeros((rows, N.MT_HEAD), dtype=torch.int32, device=dev)
        self.step_count_t = torch.zeros((rows,), dtype=torch.int32, device=dev)
        self.done_t = torch.zeros((rows,), dtype=torch.uint8, device=dev)
        self.error_t = torch.zeros((rows,), dtype=torch.int32, device=dev)
        self.prestige_t = torch.zeros((rows, n), dtype=torch.float64, device=dev) if env.prestige_t is not None else None
        self.state = N.State(self.grid_state.data_ptr(), self.agent_state.data_ptr(), self.mt_state.data_ptr(), self.mt_pos.data_ptr(),
                             self.step_count_t.data_ptr(), self.done_t.data_ptr(), self.error_t.data_ptr(),
                             self.prestige_t.data_ptr() if self.prestige_t is not None else None, self.mt_head.data_ptr(), None)


class EnvLookahead(object):
    """`env._look`; MultiGridEnv.lookahead / fork, whose docstrings are the contract, delegate here.  Nothing is allocated or
    launched until the first call."""

    def __init__(self, env):
        self.env = env
        self.shadow = None          # _Rows: the shadow state, re-made only when K * m grows
        self.cfg = None             # the env's MgConfig with B = R
        self.out = {}               # {(K, T, m): (rewards, done_u8, errors)} of the last shape: rewritten by the next call of that shape
        self.staging = None         # _Rows: fork's staging rows
        self.launches = 0
        self._errors = None
        self._keep = None           # what an asynchronous launch still reads (ids, actions)

    # the shadow tensors under the env's names (None before the first call)
    def __getattr__(self, name):
        if name in _Rows.KEYS:
            return None if self.shadow is None else getattr(self.shadow, name)
        raise AttributeError(name)

    @property
    def errors(self):
        """(K, m) int32 of the last call: the first MG_ERR_* code a simulated step of the row recorded (None before a call)"""
        return self._errors

    def _config(self, rows):
        cfg = N.Config.from_buffer_copy(self.env._cfg)
        cfg.B = rows
        return cfg

    def lookahead(self, actions, env_ids=None):
        import torch
        env = self.env
        if env._dry:
            raise RuntimeError("lookahead runs on the device; a _dry env has none")
        B, n, dev = env.batch_size, env.num_agents, env.device
        if not torch.is_tensor(actions):
            actions = torch.as_tensor(np.asarray(actions))
        if actions.dim() == 3:
            actions = actions.unsqueeze(0)
        _, ids = P.select(B, dev, None, env_ids, "lookahead")
        ids = None if ids is None else ids.contiguous()     # (a strided view of ids: the kernel reads m consecutive words)
        m = B if ids is None else int(ids.shape[0])
        if actions.dim() != 4 or actions.shape[2] != m or actions.shape[3] != n:
            raise ValueError("lookahead: actions must have shape (K, T, %d, %d) or (T, %d, %d), got %s"
                             % (m, n, m, n, tuple(actions.shape)))
        if actions.dtype not in (torch.int64, torch.int32, torch.uint8):
            actions = actions.to(torch.int64)
        if actions.device != dev or not actions.is_contiguous():
            actions = actions.to(dev).contiguous()
        K, T = int(actions.shape[0]), int(actions.shape[1])
        R = K * m
        if R >= 2 ** 31:
            raise ValueError("lookahead: %d plans of %d envs are more rows than a launch takes" % (K, m))
        key = (K, T, m)
        if key not in self.out:     # (the last shape only: a planner whose m changes with every call keeps one set of outputs)
            self.out.clear()
            self.out[key] = (torch.zeros((K, T, m, n), dtype=torch.float32, device=dev),
                             torch.zeros((K, T, m), dtype=torch.uint8, device=dev),
                             torch.zeros((K, m), dtype=torch.int32, device=dev))
        rewards, done, errors = self.out[key]
        self._errors = errors
        if R == 0 or T == 0:
            return rewards, done.view(torch.bool)
        if self.shadow is None or self.shadow.rows < R:
            self.shadow = None      # (the old rows go first)
            self.shadow = _Rows(env, R)
        env._sync_tables()
        self.cfg = self._config(R)
        self._keep = (ids, actions)
        stream = env._stream()
        N.check(env._lib.mg_fork_rows(C.byref(env._cfg), C.byref(env._state), C.byref(self.shadow.state),
                                      None if ids is None else ids.data_ptr(), None, R, R, m, stream))
        N.check(env._lib.mg_rollout(C.byref(self.cfg), C.byref(self.shadow.state), actions.data_ptr(), actions.element_size(), T, m,
                                    rewards.data_ptr(), done.data_ptr(), errors.data_ptr(), stream))
        self.launches += 2
        return rewards, done.view(torch.bool)

    def _fork_ids(self, v, what):
        """ids of `fork`: (k,) int64 on the device, contiguous; host values are range-checked"""
        _, ids = P.select(self.env.batch_size, self.env.device, None, v, "fork(%s)" % what)
        return ids.contiguous()

    def fork(self, src_ids, dst_ids):
        import torch
        env = self.env
        if env._dry:
            raise RuntimeError("fork runs on the device; a _dry env has none")
        B, dev = env.batch_size, env.device
        if not P.on_device(dst_ids, dev):
            d = P.host_ids(dst_ids, B, "fork(dst_ids=)")
            if len(set(d.tolist())) != d.size:
                raise ValueError("fork: a dst env is named twice (%s)" % d.tolist())
        src, dst = self._fork_ids(src_ids, "src_ids"), self._fork_ids(dst_ids, "dst_ids")
        k = int(dst.shape[0])
        if int(src.shape[0]) != k:
            raise ValueError("fork: %d src_ids for %d dst_ids" % (int(src.shape[0]), k))
        if k == 0:
            return
        # ids of a device tensor are not read back: a pair with an id outside the batch copies nothing — its dst becomes -1,
        # which the scatter launch skips, and the torch copies below send it to a spare row
        guarded = P.on_device(src_ids, dev) or P.on_device(dst_ids, dev)
        if guarded:
            ok = (src >= 0) & (src < B) & (dst >= 0) & (dst < B)
            src, dst = src.clamp(0, B - 1), torch.where(ok, dst, torch.full_like(dst, -1))
        if self.staging is None or self.staging.rows < k:
            self.staging = None
            self.staging = _Rows(env, k)
        env._sync_tables()
        st, stream = self.staging, env._stream()
        self._keep = (src, dst)
        # gather into the staging rows, then scatter: a row may be a source and a destination of one call
        N.check(env._lib.mg_fork_rows(C.byref(env._cfg), C.byref(env._state), C.byref(st.state), src.data_ptr(), None, k, k, k, stream))
        N.check(env._lib.mg_fork_rows(C.byref(self._config(k)), C.byref(st.state), C.byref(env._state), None, dst.data_ptr(), B, k, k,
                                      stream))
        self.launches += 2
        # what state_dict() carries besides the MgState: the same rows, by torch (gathered before they are written)
        def put(t):
            if not guarded:
                t[dst] = t[src]
                return
            ext = torch.cat([t, t[:1]])             # (row B: where the pairs that copy nothing go)
            ext[torch.where(dst < 0, torch.full_like(dst, t.shape[0]), dst)] = t[src]
            t.copy_(ext[:t.shape[0]])

        for t in (env.ep_return_t, env.params_t if env._params.decl else None, env.edits_t if env.level_edits else None):
            if t is not None:
                put(t)
        env._levels.fork(put)       # set_levels: the running episode's level, and the level the env resets to next
        if env._explore is not None:
            env._explore.fork(put)  # explore=True: the four rows of the maps (memory=True: six)
        env.invalidate_obs()
