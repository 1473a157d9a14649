"""Batched multi-agent gridworld: the gym-style `MultiGridEnv.reset()/step()` surface of
kandouss/marlgrid (`marlgrid/base.py:334-708`) with a leading env-batch dimension B, the state in
HBM and every per-step operation a hand-written HIP kernel (libmarlgrid_hip.so, C ABI in
include/marlgrid_hip.h).  This module is host-side plumbing only: argument handling, the
`_gen_grid` recorder, table/atlas upload and kernel launches on torch's current stream.  There is
no CPU fallback.

State layout (all torch tensors on one MI355X; struct-of-arrays over B):
    grid_state   uint8  (B, cells_stride)   object id per cell, index x*H + y  (MultiGrid.grid[i, j])
    agent_state  int64  (B, n)              packed 8-byte agent records (MG_AG_* in the C header)
    mt_state     int32  (B, 624) + mt_pos   per-env MT19937, numpy RandomState stream (lazy form)
    mt_head      int32  (B, 16)             the next 16 outputs of that stream (what a step draws from)
    step_count   int32  (B,), done uint8 (B,), error int32 (B,)
    obs          uint8  (B, n, P, P, 3),   rewards float32 (B, n)

Differences from the reference that the batch forces (documented in DESIGN.md):
  * obs / rewards / done are tensors with a leading B (the reference returns a list of n arrays,
    a float64 ndarray and a bool); obs values are identical, dtype is uint8 as the declared
    observation space says (the reference actually returns int64 arrays, base.py:305);
  * `_gen_grid` is *recorded* once per reset (walls / put_obj -> static template, place_obj ->
    ordered rejection-sampling program) and replayed on the device for every env with that env's
    own RNG, so scenario subclasses written against the reference API keep working; layout logic
    that branches on a random draw in Python says so with `self._fork(draw)` (or draws through
    `_rand_elem` / `_rand_bool`) and is recorded once per value — the recorder, its op type and the
    packing of a program are marlgrid_amd/gen_recorder.py (the parameter table: gen_params.py; replayable levels: levels.py);
  * per-env runtime errors (the reference's exceptions) are collected in `error` and raised as the
    matching Python exception after the step (strict=True) or on `check_errors()`.
"""
import ctypes as C
import functools
import os

import numpy as np

from . import _native as N
from . import per_env, rendering, seeding, spaces
from .agents import GridAgentInterface
from .gen_edits import EditTable
from .gen_params import ParamTable
from .explore import EnvExplore
from .goal import EnvGoal
from .lookahead import EnvLookahead
from .gen_recorder import GenDraw, GenRecorder, _NO_BRANCH, _any_draw, _gen_add, _trace, decode_program, pack_program
from .levels import EnvLevels, LevelBank
from . import launch_tables as LT
from .launch_tables import _GENERIC_WARNED, _warn_generic_kernel      # noqa: F401  (tests reset the set through this module)
from .step_launch import StepPlan
from .objects import BonusTile, Goal, Wall, WorldObj

TILE_PIXELS = 32
DEFAULT_PLACE_OBS = "search"
STATE_DICT_VERSION = 3              # the C ABI version that last changed the MgState layout / RNG form the tensors follow


def _on_device(fn):
    """Run a method with the env's GPU as the current HIP device (kernels are launched on a stream of
    that device; a mismatch only happens when one process drives several GPUs)."""
    @functools.wraps(fn)
    def wrapper(self, *args, **kwargs):
        if self._dry:
            return fn(self, *args, **kwargs)
        import torch
        if torch.cuda.current_device() == self.device.index:
            return fn(self, *args, **kwargs)
        with torch.cuda.device(self.device):
            return fn(self, *args, **kwargs)
    return wrapper


class ObjectRegistry(object):
    """object kind <-> uint8 id (the reference keeps instance <-> key maps per grid,
    base.py:19-64; here ids index the device object table and are stable for the env's life)."""

    def __init__(self, max_num_objects=N.MAX_OBJ):
        self.objs = [None]
        self.key_to_id = {}
        self.max_num_objects = max_num_objects
        self.version = 0

    def __len__(self):
        return len(self.objs)

    def get_key(self, obj):
        if obj is None:
            return 0
        if not isinstance(obj, WorldObj) or obj.is_agent:
            raise ValueError("only non-agent WorldObj instances can be put in the grid")
        k = obj.key()
        if k in self.key_to_id:
            return self.key_to_id[k]
        if len(self.objs) >= self.max_num_objects:
            raise ValueError("Object registry full.")
        self.objs.append(obj)
        self.key_to_id[k] = len(self.objs) - 1
        self.version += 1
        for r in obj.related():
            self.get_key(r)
        return self.key_to_id[k]

    def obj_of_key(self, key):
        return self.objs[int(key)]

    def find(self, obj):
        return self.key_to_id.get(obj.key(), 0)

    # the rest of the reference's registry interface (base.py:32-53)
    def get_next_key(self):
        if len(self.objs) >= self.max_num_objects:
            raise ValueError("Object registry full.")
        return len(self.objs)

    def add_object(self, obj):
        return self.get_key(obj)

    def contains_object(self, obj):
        return obj is None or (isinstance(obj, WorldObj) and obj.key() in self.key_to_id)

    def contains_key(self, key):
        return 0 <= int(key) < len(self.objs)


def rotate_grid(grid, rot_k):
    """base.py:67-80 on tensors whose last two dims are (x, y): np.rot90 with the args used for images"""
    rot_k = rot_k % 4
    if rot_k == 3:
        return grid.flip(-1).transpose(-1, -2)
    if rot_k == 1:
        return grid.flip(-2).transpose(-1, -2)
    if rot_k == 2:
        return grid.flip(-1).flip(-2)
    return grid


class MultiGrid(object):
    """The grid container (base.py:83-331).  Constructed inside `_gen_grid`, where it records the
    static part of the layout; afterwards it is a view on the env's HBM grid."""

    def __init__(self, shape, obj_reg=None, orientation=0):
        env = getattr(_trace, "env", None)
        if env is None:
            raise RuntimeError("MultiGrid(...) is constructed inside MultiGridEnv._gen_grid")
        if not isinstance(shape, tuple):
            raise ValueError("Must create grid from shape tuple.")
        self.width, self.height = shape
        if self.width < 3 or self.height < 3:
            raise ValueError("Grid needs width, height >= 3")
        if (self.width, self.height) != (env.width, env.height):
            raise ValueError("_gen_grid must build a grid of the env's own (width, height)")
        self.orientation = orientation
        self._env = env
        self._rec = env._gen
        self.obj_reg = env.obj_reg
        self._template = np.zeros((self.width, self.height), np.uint8)
        # what `_gen_grid` itself has drawn so far — the template plus the static edits made after a place_obj (which go
        # into the reset program, not the template): what get() answers while `_gen_grid` runs
        self._shadow = np.zeros((self.width, self.height), np.uint8)
        # cells a recorded random placement may have filled since `_gen_grid` last drew on them (place_obj only takes empty
        # cells of its sampling rectangle; a later static edit of a cell decides it again)
        self._maybe = np.zeros((self.width, self.height), bool)
        self._rec.begin(self)

    # ---- layout recording / live edits --------------------------------------------------------
    def set(self, i, j, obj):
        rec = self._rec
        if rec.active and _any_draw(i, j):
            rec.fill_sym(self.obj_reg.get_key(obj), [(i, j, _gen_add(i, 1), _gen_add(j, 1))])
            return
        assert i >= 0 and i < self.width
        assert j >= 0 and j < self.height
        if rec.active:
            key = self.obj_reg.get_key(obj)
            if rec.static(("put", key, int(i), int(j)), key, [(int(i), int(j), int(i) + 1, int(j) + 1)]):
                self._template[i, j] = key
            self._shadow[i, j] = key
            self._maybe[i, j] = False
        else:
            self._env.put_obj(obj, i, j)

    def horz_wall(self, x, y, length=None, obj_type=Wall):
        if length is None:
            length = self.width - x
        if _any_draw(x, y, length):
            return self._wall_sym(obj_type, [(x, y, _gen_add(x, length), _gen_add(y, 1))])
        self._wall(("horz_wall", int(x), int(y), int(length)), [(x + i, y) for i in range(length)], obj_type,
                   [(x, y, x + length, y + 1)])

    def vert_wall(self, x, y, length=None, obj_type=Wall):
        if length is None:
            length = self.height - y
        if _any_draw(x, y, length):
            return self._wall_sym(obj_type, [(x, y, _gen_add(x, 1), _gen_add(y, length))])
        self._wall(("vert_wall", int(x), int(y), int(length)), [(x, y + j) for j in range(length)], obj_type,
                   [(x, y, x + 1, y + length)])

    def wall_rect(self, x, y, w, h, obj_type=Wall):
        if _any_draw(x, y, w, h):
            xe, ye = _gen_add(x, w), _gen_add(y, h)
            return self._wall_sym(obj_type, [(x, y, xe, _gen_add(y, 1)), (x, ye - 1, xe, ye), (x, y, _gen_add(x, 1), ye),
                                             (xe - 1, y, xe, ye)])
        cells = ([(x + i, y) for i in range(w)] + [(x + i, y + h - 1) for i in range(w)]
                 + [(x, y + j) for j in range(h)] + [(x + w - 1, y + j) for j in range(h)])
        self._wall(("wall_rect", int(x), int(y), int(w), int(h)), cells, obj_type,
                   [(x, y, x + w, y + 1), (x, y + h - 1, x + w, y + h), (x, y, x + 1, y + h), (x + w - 1, y, x + w, y + h)])

    def _wall_sym(self, obj_type, rects):
        """a wall helper with a draw among its arguments: its rectangles as fills of the reset program"""
        if not self._rec.active:
            raise NotImplementedError(_NO_BRANCH % "used outside _gen_grid")
        self._rec.fill_sym(self.obj_reg.get_key(obj_type()), rects)

    def _wall(self, sym, cells, obj_type, rects):
        rec = self._rec
        # (objects are value types here: every obj_type() of a helper is the same table row.  Walls of Walls are recorded
        # as what they are; a helper drawn with another type is, before the first place_obj, its cells one by one — the
        # template does not care — and after one a handful of rectangle fills in the reset program, not an op per cell)
        if rec.active and (obj_type is Wall or rec.in_program):
            key = self.obj_reg.get_key(obj_type())
            for (i, j) in cells:
                assert 0 <= i < self.width and 0 <= j < self.height
            if obj_type is not Wall:
                sym = [("put", key, int(i), int(j)) for (i, j) in dict.fromkeys(cells)]
            if rec.static(sym, key, [tuple(int(v) for v in r) for r in rects if r[2] > r[0] and r[3] > r[1]]):
                for (i, j) in cells:
                    self._template[i, j] = key
            for (i, j) in cells:
                self._shadow[i, j] = key
                self._maybe[i, j] = False
        else:
            for (i, j) in cells:
                self.set(i, j, obj_type())

    # ---- live views -----------------------------------------------------------------------------
    @property
    def grid(self):
        """(B, W, H) uint8 object ids (live HBM view)"""
        e = self._env
        return e.grid_state[:, :e.width * e.height].view(e.batch_size, e.width, e.height)

    def get(self, i, j, env=0):
        """the non-agent object kind in cell (i, j) of env `env` (host sync; debugging aid)"""
        assert i >= 0 and i < self.width
        assert j >= 0 and j < self.height
        if self._rec.active:        # inside `_gen_grid`: what it has drawn so far (random placements are per env: not in here)
            if self._maybe[i, j]:
                # upstream's grid.get() here sees what an earlier place_obj put into THIS env's cell; the recorder cannot —
                # the draw happens later, on the device, per env.  Layout code that branches on the answer would be recorded
                # with a layout the reference would not produce: say so instead of answering "empty" silently.
                import warnings
                warnings.warn("marlgrid_amd: grid.get(%d, %d) inside _gen_grid reads a cell an earlier random place_obj may "
                              "have filled — placements are drawn per env on the device, the recorder answers with the static "
                              "layout only (%s); a layout that branches on this value is not recorded faithfully"
                              % (i, j, "empty" if self._shadow[i, j] == 0 else "the object drawn there"), RuntimeWarning, stacklevel=2)
            return self.obj_reg.obj_of_key(int(self._shadow[i, j]))
        return self.obj_reg.obj_of_key(int(self.grid[env, i, j].item()))

    def encode(self, vis_mask=None):
        """(B, W, H, 3) uint8 — batched MultiGrid.encode (base.py:196-214)"""
        return self._env._encode(vis_mask)

    # host-side (torch) counterparts of the array helpers gen_obs_grid is written with upstream; the
    # obs kernel does its own crop / rotate / shadow cast, these are for callers and for tests
    @property
    def opacity(self):
        """(B, W, H) bool: cells one cannot see through (base.py:103-106; empty cells and agents are transparent)"""
        import torch
        e = self._env
        opaque = torch.tensor([False] + [not o.see_behind() for o in self.obj_reg.objs[1:]], device=e.device)
        return opaque[self.grid.long()]

    def rotate_left(self, k=1):
        """(B, W', H') object ids of the whole grid rotated like base.py:115-120"""
        return rotate_grid(self.grid, k)

    def slice(self, topX, topY, width, height, rot_k=0):
        """(B, w, h) object ids of a window of every env, zero-padded outside the grid and rotated
        (base.py:123-147).  topX / topY: ints or (B,) tensors (e.g. columns of `agent.get_view_exts()`)."""
        import torch
        e = self._env
        g = self.grid
        B = g.shape[0]
        tx = torch.as_tensor(topX, device=e.device).long().expand(B)
        ty = torch.as_tensor(topY, device=e.device).long().expand(B)
        xs = tx[:, None] + torch.arange(width, device=e.device)[None, :]          # (B, w)
        ys = ty[:, None] + torch.arange(height, device=e.device)[None, :]         # (B, h)
        ok = ((xs >= 0) & (xs < self.width))[:, :, None] & ((ys >= 0) & (ys < self.height))[:, None, :]
        flat = xs.clamp(0, self.width - 1)[:, :, None] * self.height + ys.clamp(0, self.height - 1)[:, None, :]
        sub = torch.gather(g.reshape(B, -1), 1, flat.reshape(B, -1)).view(B, width, height)
        return rotate_grid(torch.where(ok, sub, torch.zeros_like(sub)), rot_k)

    @classmethod
    def decode(cls, array):
        raise NotImplementedError      # as upstream (base.py:216-218)


class _HostFlag(object):
    """MgState.error_flag: one int32 in pinned host memory that the device can write (mg_host_flag_alloc)"""

    def __init__(self, lib):
        self._lib = lib
        h, d = C.POINTER(C.c_int32)(), C.POINTER(C.c_int32)()
        N.check(lib.mg_host_flag_alloc(C.byref(h), C.byref(d)))
        self._host = h
        self.dev = C.cast(d, C.c_void_p).value

    def raised(self):
        return self._host[0] != 0

    def clear(self):
        self._host[0] = 0

    def __del__(self):
        try:
            self._lib.mg_host_flag_free(self._host)
        except Exception:       # interpreter shutdown
            pass


class _LibBuffer(object):
    """Device memory straight from the driver (mg_obs_alloc: hipMalloc outside torch's caching allocator), handed
    to torch through the CUDA array interface: the tensor keeps this object alive, and the memory goes back to
    the driver — not into a cache — when the last view of it dies."""

    def __init__(self, lib, nbytes, device):
        self._lib, self.device, self.nbytes = lib, device, int(nbytes)
        self.ptr = lib.mg_obs_alloc(self.nbytes, device.index)
        self.ok = bool(self.ptr)
        if self.ok:
            self.__cuda_array_interface__ = {"shape": (self.nbytes,), "typestr": "|u1", "data": (self.ptr, False),
                                             "version": 2, "strides": None}

    def tensor(self, shape):
        import torch
        t = torch.as_tensor(self, device=self.device).view(shape)
        assert t.data_ptr() == self.ptr            # shares the memory (no copy)
        return t

    def __del__(self):
        if getattr(self, "ptr", None):
            try:
                import torch
                torch.cuda.synchronize(self.device)      # no launch may still be writing it
                self._lib.mg_obs_free(self.ptr)
            except Exception:   # interpreter shutdown
                pass
            self.ptr = None


class _PlacedBuffer(object):
    """An observation buffer mg_obs_place handed out (a window of a raw driver allocation chosen for where it lies in
    HBM), as torch sees it through the CUDA array interface.  The tensor keeps this object alive; with its last view the
    buffer goes back to the library (mg_obs_release), which remembers an arena of the fast class for the next env of the
    same size in this process."""

    def __init__(self, lib, ptr, nbytes, device):
        self._lib, self.device, self.nbytes, self.ptr = lib, device, int(nbytes), int(ptr)
        self.__cuda_array_interface__ = {"shape": (self.nbytes,), "typestr": "|u1", "data": (self.ptr, False),
                                         "version": 2, "strides": None}

    def tensor(self, shape):
        import torch
        t = torch.as_tensor(self, device=self.device).view(shape)
        assert t.data_ptr() == self.ptr            # shares the memory (no copy)
        return t

    def __del__(self):
        if getattr(self, "ptr", None):
            try:
                import torch
                with torch.cuda.device(self.device):
                    torch.cuda.synchronize(self.device)      # no launch may still be writing it
                    self._lib.mg_obs_release(self.ptr)
            except Exception:   # interpreter shutdown
                pass
            self.ptr = None


def release_obs_cache(device=None):
    """Return the observation arenas this process remembers (released buffers of the fast class, kept for the next env
    of the same size: mg_obs_release) to the driver.  `device`: a torch device / index, or None for every device.
    Returns how many there were."""
    idx = -1
    if device is not None:
        import torch
        idx = torch.device(device).index if not isinstance(device, int) else device
        idx = torch.cuda.current_device() if idx is None else idx
    return N.lib().mg_obs_trim(idx)


class _ViewGroup(object):
    """agents that share one view geometry: their launch config, atlas and observation buffers"""

    def __init__(self, key, members):
        self.key, self.members = key, members            # (view_size, tile_size, view_offset, see_through), agent ids
        self.view_size, self.tile_size, self.view_offset, self.see_through_walls = key
        self.pixels = self.view_size * self.tile_size
        self.cfg = self.atlas = self.atlas_dev = None
        self.ring = []                                   # obs tensors (B, n_g, P, P, 3), one per buffer set
        self.obs = None
        self.spec = {}                                   # specialize: want (N.WANT_*) -> handle of mg_render_specialize, or None
        self.spec_info = {}                              # ... and what the library said about it (MgSpecInfo as a dict)


class MultiGridEnv(object):
    """See module docstring.  Constructor keeps the reference's kwargs (base.py:335-347) and adds
    `batch_size`, `device`, `seeds`, `auto_reset`, `strict`."""

    metadata = {}

    def __init__(self, agents=[], grid_size=None, width=None, height=None, max_steps=100,
                 reward_decay=True, seed=1337, respawn=False, ghost_mode=True, agent_spawn_kwargs={},
                 batch_size=1, device=None, seeds=None, auto_reset=False, strict=True, obs_buffers=2,
                 fused_step=True, place_obs=True, encode_in_step=False, obs_format="image", episode_info=False,
                 obs_delta="auto", specialize=False, specialize_cache=None, level_edits=0, explore=False, memory=False, _dry=False):
        if grid_size is not None:
            assert width is None and height is None
            width, height = grid_size, grid_size
        self.respawn = respawn
        self.window = None
        self.width, self.height = int(width), int(height)
        self.max_steps = int(max_steps)
        self.reward_decay = reward_decay
        self.agent_spawn_kwargs = agent_spawn_kwargs
        self.ghost_mode = ghost_mode
        self.batch_size = int(batch_size)
        # auto_reset: False; True = "same_step" — an env whose episode ends is reset inside the same launch, `done` reports the
        # end and the observation returned is already the next episode's first —; "next_step" (what EnvPool and Gymnasium >= 1.0
        # do): the step that ends an episode returns the TERMINAL state's observation with done=True and does not reset; the
        # env's next step() ignores that env's action row and is its reset — the new episode's first observation, reward 0,
        # done=False.  One launch per step either way (mg_*_ep).
        if auto_reset is True or auto_reset is False or auto_reset is None:
            auto_reset = bool(auto_reset)
        if auto_reset not in (False, True, "same_step", "next_step"):
            raise ValueError("auto_reset must be False, True (= 'same_step'), 'same_step' or 'next_step' (got %r)" % (auto_reset,))
        self.auto_reset = bool(auto_reset)
        self.auto_reset_mode = None if not auto_reset else "next_step" if auto_reset == "next_step" else "same_step"
        # episode_info=True: step()'s fourth value is {"terminated", "truncated", "reset": (B,) bool, "episode_return": (B, n)
        # float64, "episode_length": (B,) int32} — device tensors of the step's buffer set, like rewards and done — written by
        # the step's own launch: terminated = done and every agent is done, truncated = done by the time limit alone
        # (base.py:649), return / length of the running episode BEFORE any reset (where done: of the finished episode),
        # reset = this call was the env's reset ("next_step" only).  False: {} — and unless auto_reset="next_step" the plain
        # entry points are called, exactly as before.
        self.episode_info = bool(episode_info)
        self._use_ep = self.episode_info or self.auto_reset_mode == "next_step"
        # Per-env runtime errors (the reference's exceptions).  strict=True: raised without giving up the
        # asynchronous launch queue — the kernels raise a one-word flag in host-mapped memory that every
        # step()/reset() polls (no stream synchronize), so the exception surfaces at the next call into the env
        # after the GPU got there, at the latest at check_errors().  strict="sync": raised by the very step() that
        # caused it, as upstream does (one host synchronize per step).  strict=False: only check_errors() raises.
        if strict not in (True, False, "sync"):
            raise ValueError("strict must be True, False or 'sync'")
        self.strict = strict
        self.obs_buffers = max(1, int(obs_buffers))
        # Which library call a step is follows from the options below: step_launch.py has the kinds, the order they are tried
        # in, and what an MG_E_UNSUPPORTED does to it (`_plan`: chosen at the first step, remembered)
        self._plan = StepPlan()
        self._delta_launches = 0
        self.fused_step = bool(fused_step)     # step() = one launch instead of mg_step + one launch per view group
        # encode_in_step=True: every step() (and reset()) also leaves `grid.encode()` of the batch — (B, W, H, 3) uint8,
        # base.py:196-214 — in `self.grid_encoding`, written by the step's own launch where it can (+2.4 % bytes instead of a
        # second launch), by an mg_encode launch behind it otherwise
        self.encode_in_step = encode_in_step
        self.grid_encoding = None
        # obs_format="encoded": reset() / step() / gen_obs() return every agent's gen_obs_grid(agent) -> grid.encode(vis_mask)
        # (base.py:418-451, 196-214) — (B, n, V, V, 3) uint8, index [i, j] — instead of the (B, n, P, P, 3) pixels; the step's
        # launch writes them and nothing is rasterised
        if obs_format not in ("image", "encoded"):
            raise ValueError("obs_format must be 'image' or 'encoded' (got %r)" % (obs_format,))
        self.obs_format = obs_format
        self._encoded = obs_format == "encoded"
        # obs_delta: step() writes into a buffer set of the ring that still holds the observation of `obs_buffers` steps ago;
        # with it the step's launch compares, band by band — a tile row of an agent's image —, the tiles
        # it is about to draw with the ones that buffer was drawn from (a signature tensor kept per buffer set) and does not
        # store the bands that are the same: an agent that is blocked, done, or toggles / picks up / drops changes nothing.
        # The returned tensors are VIEWS of buffers the env owns: a caller that writes into them calls invalidate_obs() (or
        # constructs with obs_delta=False).  "auto": where the step is the one fused image launch without episode outputs or
        # encode_in_step and the library has an instantiation for the shape (view 7, 8-pixel tiles, <= 3 agents, none
        # 'prestige'); True: the same, but a configuration that cannot is an error — and ALSO with episode_info,
        # auto_reset="next_step", encode_in_step or any mix of them (the episode outputs, the grid encoding or both from the one
        # delta launch; "auto" leaves those steps as they are); False: every step stores every byte.
        if obs_delta not in ("auto", True, False):
            raise ValueError("obs_delta must be 'auto', True or False (got %r)" % (obs_delta,))
        self.obs_delta = obs_delta
        # specialize: the library ships ~100 instantiations of the observation kernel; a (view_size, view_tile_size) pair off
        # that table runs the fully run-time one (the RuntimeWarning of _warn_generic_kernel), 2-2.4x slower.  "auto" / True: the
        # instantiation this configuration would have on the table is compiled when the env is built (mg_render_specialize: hipRTC,
        # ~5 s per instantiation, once per process and — through `specialize_cache` — once per machine) and launched instead, per
        # view group; the variants with encode_in_step and with episode outputs are compiled when a step first needs them.  The
        # bytes written are the table kernel's.  Where the library has nothing to compile — 'prestige' agents, a grid or an atlas
        # read in place, no libhiprtc —, "auto" keeps the table's kernel (and its warning), True raises NotImplementedError with
        # the library's reason; a shape the table already has compiled in is no error.  False (the default): launches, kernel names
        # and warnings are exactly the table's.  specialize_cache: a directory for compiled code objects; None: $MARLGRID_AMD_CACHE,
        # else ~/.cache/marlgrid_amd; False: none.  Encoded views (obs_format="encoded") rasterise nothing: not specialised.
        if specialize not in ("auto", True, False):
            raise ValueError("specialize must be False, 'auto' or True (got %r)" % (specialize,))
        self.specialize = specialize
        if specialize_cache is None:
            specialize_cache = os.environ.get("MARLGRID_AMD_CACHE") or os.path.join(os.path.expanduser("~"), ".cache", "marlgrid_amd")
        self._spec_cache = os.fsencode(specialize_cache) if specialize and specialize_cache else None
        # where the observation buffers live: "search" (= True) picks the fastest of a bounded set of candidate
        # allocations by timing the raster itself into each (_place_obs_buffers -> mg_obs_place: <= 2 s, candidates <=
        # min(a quarter of the free memory, 32 GiB)); "thorough": the long search (a second pass, larger candidates, one
        # big allocate-and-free: for a process that owns the GPU); False = plain torch allocations
        if place_obs is True:
            place_obs = DEFAULT_PLACE_OBS
        # ... or a dict of the search's own knobs: {"budget": bytes of live candidates, "seconds": per pass, "thorough": bool,
        # "stir": bool, "reuse": bool, "share": processes that share this device's memory — each counts on 1 / share of what
        # is free} (what `_place_obs_buffers` takes)
        self._place_kw = {}
        if isinstance(place_obs, dict):
            unknown = set(place_obs) - {"budget", "seconds", "thorough", "stir", "reuse", "min_bytes", "share"}
            if unknown:
                raise ValueError("place_obs: unknown keys %s" % sorted(unknown))
            self._place_kw = dict(place_obs)
            place_obs = "thorough" if place_obs.get("thorough") else "search"
        if place_obs not in ("search", "thorough", False):
            raise ValueError("place_obs must be 'search' (= True), 'thorough', a dict of budgets, or False")
        self.place_obs = place_obs
        self._dry = bool(_dry)
        if self.batch_size < 1:
            raise ValueError("batch_size must be >= 1")
        if self.width > 255 or self.height > 255:
            raise ValueError("grid dimensions are limited to 255")
        self.cells_stride = (self.width * self.height + 15) // 16 * 16

        self.agents = []
        for agent in agents:
            self.add_agent(agent)
        self._check_agents()
        for k, agent in enumerate(self.agents):
            agent._bind(self, k)         # agent.pos / .dir / .done / ... become batched views of this env

        self.obj_reg = ObjectRegistry()
        self._tables_version = -1
        self._settings_seen = self._spawn_reject_key = None
        self._gen = GenRecorder(self)       # all `_gen_grid` recording state and logic (gen_recorder.py)
        self._prog_cache = {}
        self._params = ParamTable(self)     # the per-env parameters of `_gen_grid` (gen_params.py)
        self._levels = EnvLevels(self)      # replayable levels (levels.py): nothing is allocated or launched until set_levels
        self._goal = EnvGoal(self)          # goal distance (goal.py): nothing is allocated or launched until goal_distance
        self._look = EnvLookahead(self)     # lookahead (lookahead.py): nothing is allocated or launched until lookahead / fork
        # level_edits=K (0..64): every env holds a list of K cell edits (x, y, kind, on) that its every reset applies behind
        # what `_gen_grid` laid out and before the agents are placed (an EDITS op at the end of the reset program; set_edits).
        # 0: no table, no op — recordings, programs and launches are what they were
        self._edits = EditTable(self, level_edits)
        self.level_edits = self._edits.K
        # explore=True: per agent, the world cells its observations have covered this episode (`seen`) and how often it stood
        # on each cell (`visits`), with the two per-step scalars exploration bonuses are made of (`new_cells`, `visit_count`) —
        # kept on the device by one more launch behind every reset() and step() (explore.py).  False: nothing is allocated and
        # nothing is launched
        # memory=True: beside those, each agent's last view of every cell (`memory`) and when it had it (`seen_step`), written
        # by the same one launch (mg_memory_update instead of mg_explore_update).  It implies explore=True
        self._memory_on = bool(memory)
        self.explore = bool(explore) or self._memory_on
        self._explore = None
        self._spec_ctor = None
        self._spec_last = None
        self._probe = None
        self.grid = None

        if not self._dry:
            import torch
            if not torch.cuda.is_available():
                raise RuntimeError("marlgrid_amd needs an MI355X (HIP device): there is no CPU fallback")
            self.device = torch.device(device if device is not None else "cuda")
            if self.device.type != "cuda":
                raise RuntimeError("marlgrid_amd runs on HIP devices only (got %r)" % (device,))
            if self.device.index is None:
                self.device = torch.device("cuda", torch.cuda.current_device())
            self._lib = N.lib()
            self._alloc_state()
            if self.explore:
                self._explore = EnvExplore(self, memory=self._memory_on)
        self._edits.alloc()
        self._seeds_arg = seeds
        self.seed(seed=seed)
        self.reset()
        self.obs_placement = []
        # (encoded views are a few MB: plain allocations, nothing to place)
        if not self._dry and not self._encoded and self.place_obs in ("search", "thorough"):
            self._place_obs_buffers(**self._place_kw)
        self._spec_ctor = self._spec_last     # the constructor-time `_gen_grid` (base.py:369)
        self._retrace = True

    @classmethod
    def pipelined(cls, agents, parts=2, batch_size=1, seed=1337, device=None, streams=None, **kwargs):
        """The batch as `parts` envs of this class on `parts` streams (marlgrid_amd.sharding.ShardPipeline): what a
        double-buffered sampler steps in turn so that the launches of independent shards overlap.  Part 0 is built
        with `agents` themselves, the other parts with shallow copies (a learner's networks and buffers are shared,
        the binding to an env — agent.pos, .dir, ... — is per part)."""
        import copy
        from .sharding import ShardPipeline
        agents = list(agents)
        made = []

        def make_part(batch_size, seeds, device):
            team = agents if not made else [copy.copy(a) for a in agents]
            made.append(True)
            return cls(agents=team, batch_size=batch_size, seeds=seeds, device=device, **kwargs)
        return ShardPipeline(make_part, batch_size, parts=parts, seed=seed, device=device, streams=streams)

    @classmethod
    def sharded(cls, agents, devices, batch_size=1, seed=1337, streams=None, **kwargs):
        """The batch as one env of this class per entry of `devices`, in this process (marlgrid_amd.sharding.DeviceShards:
        shard k owns `shard_range(batch_size, k, len(devices))` on devices[k] and its own stream; entries may repeat).  Shard
        0 is built with `agents` themselves, the other shards with shallow copies (a learner's networks and buffers are
        shared, the binding to an env — agent.pos, .dir, ... — is per shard).  A device named m > 1 times gives its shards
        `share=m` in `place_obs`; every other kwarg reaches every shard unchanged."""
        import copy
        from .sharding import DeviceShards, merge_share
        if "seeds" in kwargs:
            raise ValueError("sharded(): per-env seeds come from `seed` + the env's index in the whole batch")
        if kwargs.pop("device", None) is not None:
            raise ValueError("sharded(): the shards' devices are `devices`; `device` has no meaning next to it")
        agents = list(agents)
        place_obs = kwargs.pop("place_obs", True)
        made = []

        def make_shard(batch_size, seeds, device, share=1):
            team = agents if not made else [copy.copy(a) for a in agents]
            made.append(True)
            return cls(agents=team, batch_size=batch_size, seeds=seeds, device=device, place_obs=merge_share(place_obs, share),
                       **kwargs)
        return DeviceShards(make_shard, batch_size, devices, seed=seed, streams=streams)

    # ---- configuration ----------------------------------------------------------------------------
    def add_agent(self, agent_interface):
        if isinstance(agent_interface, dict):
            self.agents.append(GridAgentInterface(**agent_interface))
        elif isinstance(agent_interface, GridAgentInterface):
            self.agents.append(agent_interface)
        else:
            raise ValueError(
                "To add an agent to a marlgrid environment, call add_agent with either a "
                "GridAgentInterface object or a dictionary that can be used to initialize one.")

    def _check_agents(self):
        n = len(self.agents)
        if n < 1 or n > N.MAX_AGENTS:
            raise ValueError("the batched engine supports 1..%d agents (got %d)" % (N.MAX_AGENTS, n))
        # Every agent carries its own view (agents.py:19-35).  Agents that share (view_size, view_tile_size,
        # view_offset, see_through_walls) form a VIEW GROUP: one (B, n_g, P, P, 3) observation tensor and one
        # raster launch per group.  One group — every shipped scenario — is the fast path (one tensor, the
        # env step fused into the raster launch); with several, reset()/step() return the per-agent list the
        # reference returns.
        self._groups = []
        for k, a in enumerate(self.agents):
            if a.allow_negative_prestige:
                raise NotImplementedError("allow_negative_prestige=True raises AttributeError upstream "
                                          "(agents.py:147-148) and is not supported")
            if a.view_size < 3:
                raise ValueError("Grid needs width, height >= 3")      # what upstream's first observation raises (base.py:97-99)
            if a.view_size > N.MAX_VIEW:
                raise NotImplementedError("view_size must be <= %d" % N.MAX_VIEW)
            if not (0 <= a.view_offset < a.view_size):
                raise ValueError("view_offset out of range")
            key = (a.view_size, a.view_tile_size, a.view_offset, bool(a.see_through_walls))
            for g in self._groups:
                # (encoded views: the tile size plays no part — a group's tile size is its first member's, used only by the
                # pixel views gen_obs_grid() and render() draw on demand)
                if g.key == key or (self._encoded and g.key[0] == key[0] and g.key[2:] == key[2:]):
                    g.members.append(k)
                    break
            else:
                self._groups.append(_ViewGroup(key, [k]))
        self._hetero = len(self._groups) > 1
        self._prestige = [a.color == "prestige" for a in self.agents]
        self._all_image = all(a.observation_style == "image" for a in self.agents)
        # the first group's view parameters double as "the env's" (what uniform envs have always exposed)
        self.view_size, self.tile_size, self.view_offset, self.see_through_walls = self._groups[0].key
        self.obs_pixels = self.view_size * self.tile_size
        if self._encoded:       # each agent's observation_space (and a rich agent's 'pov'): Box(0, 255, (V, V, 3), uint8)
            for a in self.agents:
                box = spaces.Box(low=0, high=255, shape=(a.view_size, a.view_size, 3), dtype="uint8")
                if a.observation_style == "image":
                    a.observation_space = box
                else:
                    a.observation_space = spaces.Dict(dict(a.observation_space.spaces, pov=box))

    @property
    def num_agents(self):
        return len(self.agents)

    @property
    def kernel_name(self):
        """the instantiation of the observation kernel a step launches (first view group), as the launcher names it
        (mg_render_kernel_name) and as rocprofv3 prints it"""
        self._sync_tables()
        return self._groups[0].kernel_name

    @property
    def specialization(self):
        """specialize: what mg_render_specialize made for this env so far — one MgSpecInfo dict (kernel_name, the five
        parameters, lds_bytes, scratch_bytes, code_bytes, compile_seconds, cache_hit; request_seconds: the whole call, load
        included) per handle, view group by view group, with `group` and `want` (0 plain, 1 with the encode, 2 with episode outputs)"""
        self._sync_tables()
        return [dict(g.spec_info[w], group=k, want=w) for k, g in enumerate(self._groups) for w in sorted(g.spec) if g.spec[w]]

    def _spec(self, g, want):
        """the group's handle for `want` (N.WANT_PLAIN / _ENCODE / _EPISODE), asked for on first use; None: the table's launch"""
        if not self.specialize or self._encoded:
            return None
        if want not in g.spec:
            import torch
            info, h = N.SpecInfo(), C.c_void_p()
            if self._spec_cache:
                try:
                    os.makedirs(self._spec_cache, exist_ok=True)
                except OSError:                  # (a home that cannot be written: compile without a cache)
                    self._spec_cache = None
            import time
            t0 = time.perf_counter()
            with torch.cuda.device(self.device):      # (a handle belongs to the device it is loaded on)
                rc = self._lib.mg_render_specialize(C.byref(g.cfg), want, 0, None, self._spec_cache, C.byref(h), C.byref(info))
            g.spec_info[want] = dict(info.as_dict(), request_seconds=time.perf_counter() - t0)      # (compile or cache read, and the load)
            if rc == N.E_UNSUPPORTED:
                g.spec[want] = None
                if self.specialize is True and not info.table_is_ideal:
                    raise NotImplementedError("specialize=True: view_size=%d, view_tile_size=%d: %s"
                                              % (g.view_size, g.tile_size, info.reason.decode()))
            else:
                N.check(rc)
                g.spec[want] = h
        return g.spec[want]

    def _release_spec(self):
        """unload every handle (the tables changed: the instantiations were compiled for the old ones' LDS layout; or the env goes)
        — and with them the step's remembered call, which may hold one"""
        self._plan.chosen = None
        for g in getattr(self, "_groups", ()):
            for h in g.spec.values():
                if h:
                    self._lib.mg_render_spec_release(h)
            g.spec, g.spec_info = {}, {}

    def __del__(self):
        try:
            self._release_spec()
        except Exception:      # (interpreter shutdown: the library or the device may be gone already)
            pass

    @property
    def action_space(self):
        return spaces.Tuple([agent.action_space for agent in self.agents])

    @property
    def observation_space(self):
        return spaces.Tuple([agent.observation_space for agent in self.agents])

    # ---- device state -------------------------------------------------------------------------------
    def _alloc_state(self):
        import torch
        B, n, dev = self.batch_size, self.num_agents, self.device
        P = self.obs_pixels
        with torch.cuda.device(dev):
            self.grid_state = torch.zeros((B, self.cells_stride), dtype=torch.uint8, device=dev)
            self.agent_state = torch.zeros((B, n), dtype=torch.int64, device=dev)
            self.mt_state = torch.zeros((B, N.MT_N), dtype=torch.int32, device=dev)
            self.mt_pos = torch.zeros((B,), dtype=torch.int32, device=dev)
            self.mt_head = torch.zeros((B, N.MT_HEAD), dtype=torch.int32, device=dev)
            self.step_count_t = torch.zeros((B,), dtype=torch.int32, device=dev)
            self.error_t = torch.zeros((B,), dtype=torch.int32, device=dev)
            # agent.prestige (agents.py:141-153): only needed when some agent's colour is 'prestige'
            self.prestige_t = torch.zeros((B, n), dtype=torch.float64, device=dev) if any(self._prestige) else None
            # step() outputs rotate through `obs_buffers` buffer sets (default 2), so what one step
            # returned stays intact while the next step is computed — the README loop
            # `save_step(obs, act, next_obs, rew, done)` sees two different observations.
            for g in self._groups:
                g.shape = (B, len(g.members), g.pixels, g.pixels, 3)
                if self._encoded:       # the encoded views; pixels only on demand (_pixel_views)
                    g.shape = (B, len(g.members), g.view_size, g.view_size, 3)
                g.pix = None
                g.ring = [torch.zeros(g.shape, dtype=torch.uint8, device=dev) for _ in range(self.obs_buffers)]
                g.obs = g.ring[0]
            self._ring = [dict(obs=self._groups[0].ring[i],
                               rewards=torch.zeros((B, n), dtype=torch.float32, device=dev),
                               done=torch.zeros((B,), dtype=torch.uint8, device=dev),
                               sig=None)       # (obs_delta: the signature of what `obs` holds, below)
                          for i in range(self.obs_buffers)]
            self._ring_i = 0
            # obs_delta: per buffer set the tile map its observation was drawn from (MG_DELTA_SIG_BYTES per env), in DEVICE memory
            # and invalidated there — filled with 0xFF: the entry 0xFFFF is no tile, every band compares unequal and is stored —,
            # so that a captured step (torch.cuda.graph) sees an invalidation as an eager one does.  Made with the ring: step()
            # allocates nothing.
            self.episode_level = torch.full((B,), -1, dtype=torch.int64, device=dev)     # set_levels: the running episode's seed
            if self._delta_wanted():
                for r in self._ring:
                    r["sig"] = torch.full((B * N.delta_sig_bytes(n, self.view_size),), 0xFF, dtype=torch.uint8, device=dev)
            self.obs, self.rewards, self.done_t = (self._ring[0][k] for k in ("obs", "rewards", "done"))
            self.done_b = self.done_t.view(torch.bool)      # the same bytes, as the bool tensor step() returns
            # episode boundaries (mg_*_ep): the persistent return accumulator; per buffer set the step's outputs and, made
            # from its flag byte by ONE small elementwise launch, the three bool tensors of the info dict (the three flags
            # exclude each other — truncated is "done and not terminated", a reset call is not done —: flag == 1 / 2 / 4)
            self.ep_return_t = None
            if self.episode_info:
                self.ep_return_t = torch.zeros((B, n), dtype=torch.float64, device=dev)
                self._ep_vals = torch.tensor([[N.EPF_TERMINATED], [N.EPF_TRUNCATED], [N.EPF_RESET]], dtype=torch.uint8, device=dev)
                for r in self._ring:
                    r["ep_return"] = torch.zeros((B, n), dtype=torch.float64, device=dev)
                    r["ep_length"] = torch.zeros((B,), dtype=torch.int32, device=dev)
                    r["ep_flags"] = torch.zeros((B,), dtype=torch.uint8, device=dev)
                    r["ep_bits"] = bits = torch.zeros((3, B), dtype=torch.bool, device=dev)
                    r["info"] = {"terminated": bits[0], "truncated": bits[1], "reset": bits[2], "episode_return": r["ep_return"],
                                 "episode_length": r["ep_length"]}
            if self._use_ep:
                for r in self._ring:
                    r["ep"] = N.Episode(N.RESET_NEXT_STEP if self.auto_reset_mode == "next_step" else N.RESET_SAME_STEP, 0,
                                        self.ep_return_t.data_ptr() if self.episode_info else None,
                                        r["ep_return"].data_ptr() if self.episode_info else None,
                                        r["ep_length"].data_ptr() if self.episode_info else None,
                                        r["ep_flags"].data_ptr() if self.episode_info else None)
            # one word of pinned host memory the kernels raise when they record an error in error_t: polled by
            # step()/reset() instead of a nonzero() + .item() round trip through the stream (mapped while the
            # env's device is current: the device pointer is this device's view of the word)
            self._flag = _HostFlag(self._lib)
        self._launch_streams = {}       # streams this env has launched on since the last check_errors()
        self._state = N.State(self.grid_state.data_ptr(), self.agent_state.data_ptr(), self.mt_state.data_ptr(),
                              self.mt_pos.data_ptr(), self.step_count_t.data_ptr(), self.done_t.data_ptr(),
                              self.error_t.data_ptr(),
                              self.prestige_t.data_ptr() if self.prestige_t is not None else None,
                              self.mt_head.data_ptr(), self._flag.dev)

    @_on_device
    def _place_obs_buffers(self, budget=0, seconds=0.0, thorough=None, stir=None, reuse=True, min_bytes=0, gain=0.0, max_candidates=0,
                           slow_alloc=0.0, stir_cap=0, iters=0, share=1, fast_rate=0.0):
        """place_obs="search" (default) / "thorough": choose WHERE in HBM the observation buffers live — mg_obs_place
        (include/marlgrid_hip.h; marlgrid_amd/csrc/mg_place_obs.hip) does the work, this is its caller.

        What is measured (MI355X, profiles/r04/README.md section 1, profiles/r05/README.md): the raster's write pattern —
        thousands of concurrent sequential streams — runs at 5.3 TB/s into a buffer that lies inside one of the driver's
        physical blocks and at the speed of a dense fill (6.9 TB/s) into one that straddles the boundary between two blocks:
        0.153 instead of 0.193 ms for the bench workload's 925 MB.  The library constructs candidates on such boundaries
        (one hipMalloc of 3 P bytes, P = the power of two >= half the buffer; the buffer = the window centred on the
        2 P | P junction), times the raster into each and keeps the fastest `obs_buffers` once they run 12 % under the median.

        What it costs (the defaults are meant to be survivable for whoever shares the GPU): candidates alive at any time
        <= min(a quarter of the free memory, 32 GiB) — for buffers of several GB raised to the kept buffers plus three
        candidates, while that is within half of the free memory (a 16 GB buffer's candidates are 24 GiB each: round 5's
        flat 32 GiB could not hold one) —; 2 s at most (0.33 s per GiB of candidate above 6 GiB, 12 s at most); a kept buffer
        pins its whole candidate — 1.5 .. 3 x its size, outside torch's allocator (`env.obs_placement[g]["pinned_bytes"]`);
        buffers under 256 MiB are plain torch allocations; at most MG_PLACE_MAX (8) buffers of a ring are placed (the
        rest stay torch allocations); `share` = k: k processes share this device, each counts on 1 / k of what is free.  "thorough" adds what round 4 found necessary on memory nobody had allocated before: larger block
        pairs (a kept buffer may then pin up to 12 x its size), a second pass, one big allocate-and-free (half of the
        free memory, 64 GiB at most) that mixes the driver's free lists, and larger budgets (candidates up to half of the
        free memory / 128 GiB, 6 s per pass).  A released buffer of the fast class is
        remembered by the library: the next env of the same size in this process takes it without a search
        (`release_obs_cache()` gives them back).  Without a candidate in the fast class the best seen is kept and
        `found` is False: try again later, or with place_obs="thorough"."""
        import torch
        if thorough is None:
            thorough = self.place_obs == "thorough"
        if stir is None:
            stir = thorough
        flags = (N.PLACE_THOROUGH if thorough else 0) | (N.PLACE_STIR if stir else 0) | (0 if reuse else N.PLACE_NO_REUSE)
        share = max(1, int(share))
        if thorough and not budget:         # the long search is for a process that owns its GPU: half of what is free, 6 s per pass
            budget = min(torch.cuda.mem_get_info(self.device)[0] // (2 * share), 128 << 30)
        if thorough and not seconds:
            seconds = 6.0
        tn = N.PlaceTuning(gain=gain, slow_alloc_s_per_gib=slow_alloc, min_bytes=min_bytes, stir_bytes=stir_cap,
                           max_candidates=max_candidates, iters=iters, share=share, fast_rate=fast_rate)
        threshold = min_bytes or (256 << 20)
        any_replaced = False
        previous = list(getattr(self, "obs_placement", None) or [])
        self.obs_placement = []
        for gi, g in enumerate(self._groups):
            nbytes = g.ring[0].numel()
            if nbytes < threshold:
                self.obs_placement.append(None)
                continue
            # (a call places at most MG_PLACE_MAX buffers: a longer ring keeps torch allocations for the rest — the ring
            # rotates through all of them, `kept` says which are placed)
            keep = min(len(g.ring), N.PLACE_MAX)
            out = (C.c_void_p * keep)()
            st = N.PlaceStats()
            rc = self._lib.mg_obs_place(C.byref(g.cfg), C.byref(self._state), keep, int(budget), float(seconds), flags, C.byref(tn),
                                        out, C.byref(st), self._stream())
            if rc == N.E_NOMEM:
                # nothing was handed out: the ring stays what it was — torch allocations, or the buffers an earlier call
                # placed (whose record then stays too: they are still pinned)
                was = previous[gi] if gi < len(previous) else None
                failed = {"found": False, "stopped": N.PLACE_STOP.get(st.stopped, str(st.stopped)) or "out of memory", "kept": [],
                          "candidates": st.candidates, "seconds": st.seconds, "buffer_bytes": nbytes, "pinned_bytes": 0}
                if was and was.get("pinned_bytes"):
                    g.placement_ms = dict(was, retry_failed=failed)
                else:
                    g.placement_ms = failed
                self.obs_placement.append(g.placement_ms)
                continue
            N.check(rc)
            g.ring = [_PlacedBuffer(self._lib, out[i], nbytes, self.device).tensor(g.shape) for i in range(keep)] + list(g.ring[keep:])
            for t in g.ring[:keep]:
                t.zero_()
            g.obs = g.ring[self._ring_i]
            any_replaced = True
            g.placement_ms = {"found": bool(st.found), "reused": st.reused, "kept": [st.kept_ms[i] for i in range(keep)],
                              "candidates": st.candidates, "windows_measured": st.windows, "passes": st.passes,
                              "stopped": N.PLACE_STOP.get(st.stopped, str(st.stopped)), "seconds": st.seconds,
                              "median_ms": st.median_ms, "all": [st.all_ms[i] for i in range(min(st.candidates, N.PLACE_ALL))],
                              "buffer_bytes": st.buffer_bytes, "candidate_bytes": st.candidate_bytes,
                              "window_offset": ((2 * (st.candidate_bytes // 3) - nbytes // 2) & ~4095) if st.candidate_bytes else None,
                              "kept_window_offsets": [st.window_offset[i] for i in range(keep)],
                              "pinned_bytes": st.pinned_bytes, "budget_bytes": st.budget_bytes, "block_pair_level": st.level,
                              "plain_stage": bool(st.plain_stage), "stirred": ({"bytes": st.stirred_bytes} if st.stirred_bytes else None),
                              "placed_buffers": keep, "ring_buffers": len(g.ring), "share": share,
                              "alloc_ms_per_GiB": 1e3 * st.alloc_seconds / max(st.alloc_bytes, 1) * (1 << 30)}
            self.obs_placement.append(g.placement_ms)
            if not st.found and not thorough and st.stopped != 7:       # (7: not bound by HBM writes — nothing to find, nothing to say)
                import warnings
                warnings.warn("marlgrid_amd: the bounded placement search found no observation buffer in the fast class for %d-byte "
                              "buffers (%d candidates, stopped: %s): if this configuration's raster is bound by HBM writes it may run up to "
                              "20 %% below its best — place_obs='thorough' searches with larger budgets (env.obs_placement has the "
                              "numbers; a configuration that is not HBM-bound has no fast class to find)"
                              % (nbytes, st.candidates, g.placement_ms["stopped"]), RuntimeWarning, stacklevel=3)
        for i, r in enumerate(self._ring):
            r["obs"] = self._groups[0].ring[i]
        self.obs = self._ring[self._ring_i]["obs"]
        self.invalidate_obs()               # (new buffers: no signature describes them)
        # (the torch-allocated ring tensors that were replaced are unreferenced now; their blocks stay in torch's caching
        # allocator for the caller's next allocations — this package does not empty a cache it does not own)
        if any_replaced:
            self._render()                  # the current observation, into the buffer that is current now

    def _stream(self):
        """torch's current stream of the env's device, as the C ABI takes it — and remembered: check_errors()
        has to wait for the launches on EVERY stream this env was driven on (a ShardPipeline part is stepped
        under its own stream and checked from wherever the caller happens to be)."""
        import torch
        s = torch.cuda.current_stream(self.device)
        self._launch_streams[s.cuda_stream] = s
        return C.c_void_p(s.cuda_stream)

    @_on_device
    def seed(self, seed=1337):
        """Seed every env's RNG (base.py:371-374).  Env b gets `seed + b` unless explicit per-env
        `seeds` were given to the constructor."""
        if self._seeds_arg is not None:
            sa = self._seeds_arg
            if hasattr(sa, "reshape"):                 # ndarray / tensor
                sa = sa.reshape(-1).tolist()
            seeds = [int(s) for s in sa]               # python ints: seeds may exceed int64
            if len(seeds) != self.batch_size:
                raise ValueError("seeds must have batch_size entries")
        else:
            seeds = [int(seed) + b for b in range(self.batch_size)]
        self.seeds = seeds
        if not self._dry:
            import torch
            keys, lens = seeding.batch_keys(seeds)
            k = torch.from_numpy(keys.view(np.int32)).to(self.device)
            kl = torch.from_numpy(lens).to(self.device)
            N.check(self._lib.mg_mt_seed(self.batch_size, k.data_ptr(), kl.data_ptr(), self.mt_state.data_ptr(),
                                         self.mt_pos.data_ptr(), self.mt_head.data_ptr(), self._stream()))
            torch.cuda.current_stream(self.device).synchronize()    # k / kl die here
        return [seed]

    # ---- `_gen_grid` recording ----------------------------------------------------------------------
    def _gen_grid(self, width, height):
        raise NotImplementedError("subclasses build self.grid here (see marlgrid_amd/envs)")

    def _rand_int(self, low, high):
        """gym-minigrid's `_rand_int`: `self.np_random.randint(low, high)`.  Inside `_gen_grid` the draw is recorded — every
        env makes it for itself on the device at every reset, from its own RNG, where upstream makes it — and what comes
        back is a `GenDraw`: usable as a coordinate or extent of later put_obj / grid.set / wall helpers, in place_obj's
        `top` / `size`, and as a bound of a later `_rand_int`.  Programs whose every possible draw cannot be shown to stay
        legal (hi > lo here, fills inside the grid, sampling rectangles non-empty) are refused with ValueError when they
        are recorded; upstream would fail for some seeds only."""
        return self._gen.rand_int(low, high)

    # ---- per-env parameters: a register whose value comes from device memory, not from the RNG ----------------------
    def _param(self, name, low, high, default=None):
        """A per-env PARAMETER of the layout: inside `_gen_grid` this returns what `_rand_int(low, high)` returns — a
        `GenDraw` over [low, high), within 0..255, usable wherever a draw is (`+- int`, coordinates and extents, place_obj's
        `top` / `size` / `count`, bounds of a later `_rand_int`, `_fork`) — but every env reads its value from its row of a
        byte table on the device (`env.params[name]`, `set_params`) when it resets, and no RNG word is consumed.  The
        recorder's proofs run over the whole interval and the device clamps what it loads to it.  One draw register and
        one table column per distinct name; naming a parameter again in the same `_gen_grid` returns the same register."""
        return self._gen.param(name, low, high, default)

    def _param_column(self, name, low, high, default):
        return self._params.column(name, low, high, default)

    params_t = property(lambda self: self._params.table)    # (B, MG_GEN_DRAWS) uint8; None until `_gen_grid` names a parameter

    @property
    def params(self):
        """name -> (B,) uint8: the column of the parameter table that `_gen_grid`'s `self._param(name, ...)` reads (a view:
        `set_params` validates what it writes, a direct write is clamped on the device when it is loaded)"""
        self._ensure_recorded()
        return {name: self.params_t[:, d["col"]] for name, d in self._params.decl.items()}

    @_on_device
    def _ensure_recorded(self):
        """the recording that follows the constructor (a subclass stores its settings after the base constructor's reset)"""
        if getattr(self, "_retrace", False):
            template, ops = self._record_gen_grid()
            if self._dry:
                self._dry_trace = (template, ops)
            else:
                self._sync_tables()
                self._reset_prog = self._program(template, ops)
            self._retrace = False

    @_on_device
    def set_params(self, env_mask=None, env_ids=None, **values):
        """Set per-env parameters of `_gen_grid` (`self._param`): `name=value` with an int, or an array / tensor of one value
        per env — (B,), or with `env_ids` (k,) — for every env, those of `env_mask` ((B,) bool) or those listed in `env_ids`.
        Host values are checked against the parameter's interval (ValueError); a device tensor is clamped to it in stream
        order, without a host synchronisation.  A value takes effect when its env next resets — reset(), the reset inside a
        step launch, a next-step reset —: the running episode is untouched."""
        self._params.set(env_mask, env_ids, **values)

    # ---- per-env cell edits: the last op of the reset program -------------------------------------------------------------
    edits_t = property(lambda self: self._edits.table)      # (B, K, 4) uint8 entries (x, y, kind, on); None at level_edits=0

    @_on_device
    def edit_key(self, obj):
        """the kind id of an object instance for an edit entry (None: 0, an empty cell).  A kind seen for the first time is
        registered and the device tables are brought up to date: the id is valid in the launch that next resets."""
        key = self.obj_reg.get_key(obj)
        self._sync_tables()
        return key

    @_on_device
    def set_edits(self, edits, env_mask=None, env_ids=None):
        """Set the edit lists of a `level_edits=K` env: `edits` is (K', 4) entries `(x, y, kind, on)` for every selected env —
        all, those of `env_mask` ((B,) bool) or those listed in `env_ids` — or one list per selected env, (B, K', 4) or with
        `env_ids` (k, K', 4); K' <= K, the slots from K' on are switched off.  An entry that is on writes `kind`
        (`env.edit_key(obj)`; 0 empties the cell) into cell (x, y) as `put_obj` / `grid.set` at the end of `_gen_grid` would,
        in list order.  Host values are checked (ValueError: x >= width, y >= height, a kind that is not registered, K' > K);
        a device tensor is written in stream order with nothing read back, and the device ignores an entry outside the grid
        or of an unknown kind.  A list takes effect when its env next resets — reset(), the reset inside a step launch, a
        next-step reset —: the running episode is untouched."""
        self._edits.set(edits, env_mask, env_ids)

    # ---- replayable levels ----------------------------------------------------------------------------------------------
    def level_bank(self, seeds_or_capacity, full=False):
        """a LevelBank on this env's device.  `full`: its slots also hold a row of this env's parameters (`bank.params`, at the
        declared defaults) and a list of `level_edits` cell edits (`bank.edits`, all off) — a level is (seed, parameters,
        edits), set with `bank.assign(slots, seeds, params=, edits=)` and taken whole by an env at its reset"""
        return LevelBank(seeds_or_capacity, None if self._dry else self.device, _dry=self._dry, env=self if full else None)

    @_on_device
    def set_levels(self, bank=None, ids=None, seeds=None, env_mask=None, env_ids=None):
        """Name the level each env plays from its NEXT reset on (the running episode is untouched, as with set_params) — for
        every env, those of `env_mask` ((B,) bool) or those listed in `env_ids`.  A level is a seed: the env's reset then is the
        reference's `env.seed(s); env.reset()`, and it plays that level at every reset until it is given another.

          * `set_levels(bank, ids)`: slots of a LevelBank of this env's device — an int, or one per env, (B,) or with `env_ids`
            (k,); -1: free-running (the env keeps its own running stream).  Envs may share a slot.
          * `set_levels(seeds=...)`: the seeds themselves, same shapes, -1: free-running.  The env keeps a bank of its own, row b
            for env b.

        Host values are checked (ValueError); device tensors are only range-guarded on the device, and with them the call reads
        nothing back.  Needs auto_reset=False or "next_step".  `env.episode_level` (B,) int64 is the seed of the level each
        env's running episode was started from (-1: free-running); with episode_info, info["level"] is the step's copy."""
        self._levels.set(bank, ids, seeds, env_mask, env_ids)

    @property
    def episode_level_t(self):      # (the name state_dict() saves it under)
        return self.episode_level

    _levels_on = property(lambda self: self._levels.on)                 # the names tests and tools read `env._levels` by
    _level_launches = property(lambda self: self._levels.launches)
    _level_bank = property(lambda self: self._levels.bank)
    _own_bank = property(lambda self: self._levels.own_bank)
    _level_of_env = property(lambda self: self._levels.level_of_env)

    # ---- goal distance: what an optimal agent would need, per env, from the env's own grid -----------------------------------
    @_on_device
    def goal_distance(self, env_mask=None, env_ids=None, field=False, _path=None):
        """The exact number of actions `left` / `right` / `forward` after which each agent's `forward` ENTERS a goal cell, on its
        env's grid as it is now: the env-owned (B, n) int32 tensor, -1 where no such sequence exists or the agent is in no cell
        (not yet spawned, done, evicted by put_obj).  With `field=True` the pair (dist, field): field (B, W, H, 4) int32 holds
        the same number for every state, field[b, x, y, dir], -1 where there is none and on cells no agent can stand on.  Both
        are updated for the selected envs only — all, those of `env_mask` ((B,) bool; step()'s `info["reset"]` as it is) or
        those listed in `env_ids` (host ids are checked, ValueError; a device tensor's ids outside the batch select nothing) — and
        start at -1; they are made at the first call.

        The analysis is static: other agents are ignored, nothing is toggled, picked up or dropped.  Free cells are empty ones
        and objects that can be overlapped without ending the episode (floor, bonus tiles, open doors); walls, keys, balls,
        boxes, closed and locked doors and lava block, and so does the outside of the grid (a border wall removed by an edit
        included).  Entering a goal ends the agent's episode, so goals are never passed through, and an agent standing on a
        goal has to leave and come back.  With `ghost_mode=False` other agents can stand in the way: the number is then a
        lower bound.

        One launch on the current stream (mg_goal_distance: a wave per selected env), nothing is read back, no host
        synchronisation; an env that never calls it allocates and launches nothing.  Derived values: no part of state_dict()."""
        return self._goal.distance(env_mask, env_ids, field, _path)

    @_on_device
    def solve_distance(self, env_mask=None, env_ids=None, max_doors=2, max_items=2, policy=False):
        """`goal_distance` with keys and doors in play: the exact number of actions out of `left` (0), `right` (1), `forward` (2),
        `pickup` (3) and `toggle` (5) after which each agent's `forward` ENTERS a goal cell — on its env's grid as it is now, the
        agent carrying what it carries now, other agents ignored, under step()'s own rules.  The env-owned (B, n) int32 tensor,
        -1 where no such sequence exists, the agent is in no cell, or it stands on a cell that is neither free nor a goal (a door
        shut on it included).  With `policy=True` the pair (dist, action): action (B, n) int64, ready for `env.step`, is the
        first action of such a path — the lowest action id that leads one action nearer (a locked door's first toggle: two) —
        and 6 (`done`) where there is no path; after stepping it, a fresh call gives exactly one less.  Selectors and tensors
        behave as `goal_distance`'s: updated for the selected envs only, -1 / 6 at the start, made at the first call.

        `drop` and `done` are never used, so an agent picks up at most ONE object: two locked doors of two colours in a row
        have no path — that is part of the definition.  A closed door costs one toggle, a locked one two (unlock, open) by an
        agent holding a key of its colour; a door counts only if it ends as a cell that can be walked on, and is never closed
        again; a box is never toggled; pickup empties the cell of anything that can be picked up.  Everything else is
        `goal_distance`'s: nothing wraps, lava blocks, goals are entered and never crossed.

        Per env the first `max_doors` (0 .. 4) shut doors and the first `max_items` (0 .. 3) items in grid order are tracked;
        those beyond block and are never touched, and an agent that already carries something tracks no item.
        `env.solve_exact` — (B,) bool, of the last call's envs — says where nothing was beyond the caps; elsewhere every value is
        -1 or not smaller than the uncapped one.  The search keeps 2^max_doors * (1 + max_items) layers in LDS; caps that do not
        fit for the grid's size raise NotImplementedError, naming the bytes and the caps that would fit, before anything is
        launched.

        One launch on the current stream (mg_solve_distance: a wave per selected env), nothing is read back; an env that never
        calls it allocates and launches nothing.  Derived values: no part of state_dict()."""
        return self._goal.solve(env_mask, env_ids, max_doors, max_items, policy)

    @property
    def solve_exact(self):
        """(B,) bool: where the last `solve_distance` call tracked every shut door and item (None before the first call)"""
        return self._goal.exact

    @_on_device
    def optimal_return(self, dist=None):
        """(B, n) float64: what an agent that takes a shortest path from here earns — R * (1 - 0.9 * (step_count + d) /
        max_steps), R without reward_decay, and 0 where d < 0 (no path) or step_count + d > max_steps (the episode is truncated
        first).  `dist`: a (B, n) tensor of distances, default `goal_distance()` of every env now; `solve_distance()`'s tensor gives
        the return of a shortest path through keys and doors.  R is the reward the
        registered Goal kinds share (ValueError if they differ or there is none).  Torch ops only."""
        return self._goal.optimal_return(dist)

    # ---- exploration maps (explore=True): None without the option ---------------------------------------------------------
    @property
    def seen(self):
        """(B, n, W, H) bool (uint8 storage), indexed [b, k, x, y] like `goal_distance`'s field: cell (x, y) was inside agent k's
        view AND VISIBLE in at least one observation returned to the caller since the env's running episode began.  "Visible" is
        exactly the `vis_mask` of the reference's `gen_obs_grid(agent)` (crop at `get_view_exts`, rotate `dir + 1` times,
        `process_vis`): all ones with `see_through_walls`, all zeros for a viewer that is not active, clipped to the grid, the
        transparency that of the grid's own object; `hide_item_types` plays no part; taken on the state the returned observation
        shows.  ONE OBSERVATION IS ONE UPDATE: every `reset()` and every `step()` updates each env it covers once, after the
        step's launch (one mg_explore_update launch per view group, on the env's stream, nothing read back) — `reset(env_mask=)`
        only the selected envs, `step()` every env, one whose episode has ended under `auto_reset=False` included.  A FRESH
        EPISODE CLEARS FIRST: an env whose step counter is 0 after the launch has just begun an episode (reset(), the same-step
        reset inside a step, the next-step reset call), and its `seen` and `visits` are cleared before the observation is
        accumulated — under `auto_reset=True` the values after a finishing step are those of the new episode's first
        observation; under `"next_step"` the terminal step still accumulates into the finished episode and the reset call
        clears.  The four tensors are rewritten in place by the next call; `state_dict()` carries `seen` and `visits` (a
        checkpoint without them loads with cleared maps), `fork` copies the four rows, `lookahead` leaves them alone.
        `obs_format`, `obs_delta`, `obs_buffers`, `encode_in_step`, `episode_info` and `specialize` do not interact with it."""
        return None if self._explore is None else self._explore.seen

    @property
    def visits(self):
        """(B, n, W, H) int32: the number of those observations (see `seen`) in which agent k was placed on (x, y)"""
        return None if self._explore is None else self._explore.visits

    @property
    def new_cells(self):
        """(B, n) int32: how many cells the last observation added to `seen[b, k]`"""
        return None if self._explore is None else self._explore.new_cells

    @property
    def visit_count(self):
        """(B, n) int32: `visits[b, k]` at agent k's own cell after the last observation's increment; 0 for an agent in no cell"""
        return None if self._explore is None else self._explore.visit_count

    # ---- memory maps (memory=True, which implies explore=True): None without the option -------------------------------------
    @property
    def memory(self):
        """(B, n, W, H, 4) uint8, indexed [b, k, x, y] = (type, colour, state, known): the triple cell (x, y) had in the most
        recent observation of agent k in which the cell was inside its view AND VISIBLE (see `seen`) — byte for byte the triple
        `obs_format="encoded"` shows at the view cell that maps to (x, y): the shadow cast applied, `hide_item_types` applied,
        an agent standing there encoded with its colour and heading.  `known` is 1 once the cell has been seen this episode: a
        seen empty cell is (0, 0, 0, 1), a cell never seen (0, 0, 0, 0); `memory[..., 3] == seen` after every call.  The rules
        are `seen`'s: one observation is one update (every `reset()` for the envs it selects, every `step()` for every env,
        ONE mg_memory_update launch per view group in place of mg_explore_update, nothing read back); an env whose step counter
        is 0 after the launch has just begun an episode and is cleared first (`memory` to 0, `seen_step` to -1); an inactive
        viewer sees nothing and changes nothing, and what it remembered earlier in the episode stays.  Rewritten in place by
        the next call; `state_dict()` carries `memory` and `seen_step` (a memory=True env that loads a checkpoint without them
        clears all six maps), `fork` copies the rows, `lookahead` leaves them alone.  An env WITHOUT the option does not take
        the two keys: `load_state_dict` raises KeyError for them, as an env without `explore` does for `seen` and `visits` — so
        an explore=True env cannot load a memory=True env's checkpoint unless the caller drops `memory` and `seen_step` first."""
        return None if self._explore is None else self._explore.memory

    @property
    def seen_step(self):
        """(B, n, W, H) int32: the env's `step_count` at that most recent observation (see `memory`), -1 where the cell was
        never seen this episode: `(seen_step >= 0) == seen`, every cell visible in the observation just returned has
        `seen_step == step_count[b]`, and `step_count[b] - seen_step` is how stale the memory of a cell is"""
        return None if self._explore is None else self._explore.seen_step

    # ---- lookahead: what T steps WOULD return, on a shadow copy of the state --------------------------------------------------
    @_on_device
    def lookahead(self, actions, env_ids=None):
        """What `T` successive `step()` calls of an `auto_reset=False` env in this env's present state would return for each of
        K action plans — without doing them.  `actions`: an integer tensor (K, T, m, n) or (T, m, n) (K = 1) on the env's device,
        of any dtype step() takes; m = len(env_ids), or B without `env_ids`; plan p of env j is `actions[p, :, j, :]`.  Returns
        the env-owned pair (rewards (K, T, m, n) float32, done (K, T, m) bool), rewritten by the next call of the same shape.
        `env_ids`: host ids are checked (ValueError); of a device tensor nothing is read back, and an id outside the batch makes
        that row inert — frozen, reward 0, done True.

        Every plan starts from a copy of the env's state, generator included: the shuffle orders are the ones the env itself
        would draw next, and the rewards are bit-identical to step()'s.  One difference: a rollout STOPS AT ITS EPISODE'S END —
        from the first step that reports `done` on, the row is frozen, its rewards are 0 and `done` stays True; an env whose
        episode has already ended (auto_reset="next_step": the terminal state) is frozen from the first row.  Nothing resets
        inside a lookahead: no reset program, level or parameter is read.

        The env is untouched: no byte of its state, error array, host error flag, observation buffers or episode accumulators
        changes.  Errors a simulated step records go to `env.lookahead_errors`, and `strict` never raises for a plan.

        Two launches on the current stream (mg_fork_rows: a wave per shadow row; mg_rollout: a lane per shadow row, all T steps),
        nothing is read back, no host synchronisation.  The shadow state — K * m rows of cells_stride + 8 n + 2 573 bytes — is
        made at the first call and re-made only when K * m grows.  Out of scope: observations of simulated states, lookahead
        through a reset, plans whose shuffles differ."""
        return self._look.lookahead(actions, env_ids)

    @property
    def lookahead_errors(self):
        """(K, m) int32 of the last `lookahead` call: the first error code (MG_ERR_*: 1 ValueError — an action outside 0..6 —, 2
        RecursionError, ...) a simulated step of the row recorded, 0 for none; None before the first call"""
        return self._look.errors

    @_on_device
    def fork(self, src_ids, dst_ids):
        """Branch the batch: env `dst_ids[i]` becomes a copy of env `src_ids[i]` — everything state_dict() carries: grid, agent
        records, generator and head, step count, done, error, 'prestige', the episode_info accumulators, the env's parameter and
        edit rows, and with set_levels the running level and the slot it resets to.  The copy goes through staging rows (gather,
        then scatter: two launches), so a row may be a source and a destination of one call.  Host ids are checked — a `dst`
        named twice is a ValueError —; of device tensors nothing is read back: a `dst` named twice is the caller's error, and a
        pair with an id outside the batch copies nothing.  With `set_levels(seeds=)` the env's own bank row — seed and
        generator — is copied, so `dst` can be re-seeded by its own id afterwards and re-seeding `src` leaves it alone; with a
        caller's bank `dst` takes `src`'s slot.

        Two copies given the same actions stay byte-identical for ever: they hold the same generator.  The observation tensors
        last returned are stale for the `dst` rows until `gen_obs()` or the next `step()`; the call ends with `invalidate_obs()`,
        so an obs_delta step redraws them."""
        self._look.fork(src_ids, dst_ids)

    # ---- branching on a draw: one recorded run of `_gen_grid` per path, merged into one guarded program --------------
    def _fork(self, d):
        """The value of `d` — an int, or a `_rand_int` result (`const +- draw[r]`) — as a plain Python int: `_gen_grid` may
        then do with it whatever Python does with an int (`if`, `range`, indexing, arithmetic).  The recorder runs
        `_gen_grid` once per value the draw can take here (at most 16; depth first over the forks met so far, at most 64
        paths) and merges the runs into one reset program: what was recorded before the fork once, then every branch's ops
        under a guard `draw[r] == value` (MgGenOp.obj, MG_GEN_GUARD) that each env evaluates for itself on the device.
        `_gen_grid` is therefore run SEVERAL TIMES and must be a function of its arguments and its draws alone."""
        if isinstance(d, (int, np.integer)) and not isinstance(d, bool):
            return int(d)
        if not isinstance(d, GenDraw):
            raise TypeError("_fork takes an int or a value of self._rand_int(...), not %s" % type(d).__name__)
        return self._gen.fork(d)

    def _rand_elem(self, iterable):
        """gym-minigrid's `_rand_elem`: one element of `iterable`, by a `_rand_int(0, len)` draw.  Inside `_gen_grid` the draw
        is recorded and forked on (`_fork`): the element that comes back is the concrete one of the path being recorded."""
        lst = list(iterable)
        return lst[self._fork(self._rand_int(0, len(lst)))]

    def _rand_bool(self):
        """gym-minigrid's `_rand_bool`: `self.np_random.randint(0, 2) == 0` — a draw of (0, 2) and a fork on it"""
        return self._fork(self._rand_int(0, 2)) == 0

    def _record_gen_grid(self):
        """run `_gen_grid` under the recorder (gen_recorder.GenRecorder.record): the template and the reset program's ops"""
        self._spec_last = rec = self._gen.record()
        return rec.template, list(rec.ops)

    @_on_device
    def put_obj(self, obj, i, j, env_mask=None):
        """Put an object at a specific position, replacing what is there (base.py:655-662) — an agent standing
        there included: as upstream it is in no cell afterwards (nobody sees it; it keeps its position, turns
        and looks), and its next successful forward move raises what upstream raises (MG_AF_EVICTED)."""
        if self._gen.active:
            self._gen.grid.set(i, j, obj)
            return True
        assert 0 <= i < self.width and 0 <= j < self.height
        key = self.obj_reg.get_key(obj)
        if not self._dry:
            self._sync_tables()
            N.check(self._lib.mg_put_obj(C.byref(self._cfg), C.byref(self._state), key, int(i), int(j),
                                         self._mask_ptr(env_mask), self._stream()))
        return True

    def _table_dev(self, table):
        """a (W, H) uint8 table as the device layout the kernels index (x*H + y, cells_stride bytes)"""
        import torch
        t = np.zeros(self.cells_stride, np.uint8)
        t[:self.width * self.height] = np.asarray(table, np.uint8).reshape(-1)
        return torch.from_numpy(t).to(self.device)

    def _place_region(self, top, size):
        # sampling rectangle, clamped exactly like base.py:692-695
        x0, y0 = (0, 0) if top is None else top[:2]
        w, h = (self.width, self.height) if size is None else size[:2]
        x0, y0 = max(int(x0), 0), max(int(y0), 0)
        x1, y1 = min(x0 + int(w), self.width), min(y0 + int(h), self.height)
        if x1 <= x0 or y1 <= y0:
            raise ValueError("place_obj: empty sampling rectangle")
        return x0, y0, x1, y1

    def _what(self, obj):
        if isinstance(obj, GridAgentInterface):
            return -(self.agents.index(obj) + 1)
        return self.obj_reg.get_key(obj)

    @_on_device
    def _place_live(self, obj, top, size, max_tries, env_mask, reject_fn=None):
        """place_obj on the live grids: per-env rejection sampling on each env's RNG.  Returns the
        chosen positions (B, 2) int32 (-1, -1 where it failed: RecursionError on check_errors())."""
        import torch
        what = self._what(obj)
        self._sync_tables()
        x0, y0, x1, y1 = self._place_region(top, size)
        pos = torch.empty((self.batch_size, 2), dtype=torch.int32, device=self.device)
        rej = self._reject_table(reject_fn, (x0, y0, x1, y1))
        rej_dev = None if rej is None else self._table_dev(rej)
        N.check(self._lib.mg_place(C.byref(self._cfg), C.byref(self._state), what, x0, y0, x1, y1,
                                   int(max(1, min(max_tries, 1e5))), None, self._mask_ptr(env_mask),
                                   None if rej_dev is None else C.c_void_p(rej_dev.data_ptr()),
                                   pos.data_ptr(), None, self._stream()))
        if self.strict:
            self.check_errors()
        return pos

    def _reject_table(self, reject_fn, region):
        """place_obj(reject_fn=) as data: the reference calls `reject_fn(pos)` with the drawn position and nothing
        else (base.py:700-701) — a function of the position alone is a table.  Evaluated once over the sampling
        rectangle (the only positions that can be drawn): (W, H) uint8, 1 = rejected; None without a callback.
        (A callback that looks at anything else — per-env state, a counter — cannot be batched and is not
        supported: it would see one call per cell here, not one per draw.)"""
        if reject_fn is None:
            return None
        x0, y0, x1, y1 = region
        t = np.zeros((self.width, self.height), np.uint8)
        for x in range(x0, x1):
            for y in range(y0, y1):
                t[x, y] = 1 if reject_fn(np.array([x, y])) else 0
        return t

    def place_obj(self, obj, top=None, size=None, reject_fn=None, max_tries=1e5, env_mask=None, count=1):
        """Rejection-sample a free cell for `obj` (base.py:690-708).  Inside `_gen_grid` this records
        one placement; the draw happens on the device, per env.  `reject_fn(pos)` is tabulated over the
        sampling rectangle once (see `_reject_table`).  `count` (not upstream's; inside `_gen_grid` only): that many
        placements in a row — an int is the same as so many calls, a `_rand_int` / `_param` value is a count that every env
        evaluates for itself at its reset (never below 0, proved when recorded)."""
        if not self._gen.active:
            if isinstance(count, GenDraw) or count != 1:
                raise NotImplementedError("place_obj(count=) is for the recorded placements of _gen_grid")
            return self._place_live(obj, top, size, max_tries, env_mask, reject_fn)
        return self._gen.place_obj(obj, top, size, reject_fn, max_tries, count)

    @_on_device
    def try_place_obj(self, obj, pos, env_mask=None):
        """Try to place `obj` (an object, or one of this env's agents) at `pos` — one (x, y) for every
        env or a (B, 2) tensor — and return a (B,) bool tensor saying where it worked (base.py:664-688)."""
        import torch
        if self._gen.active:
            raise NotImplementedError("inside _gen_grid use put_obj / place_obj")
        what = self._what(obj)
        self._sync_tables()
        p = torch.as_tensor(pos, dtype=torch.int32, device=self.device)
        if p.dim() == 1:
            p = p.expand(self.batch_size, 2)
        p = p.contiguous()
        ok = torch.zeros((self.batch_size,), dtype=torch.uint8, device=self.device)
        N.check(self._lib.mg_place(C.byref(self._cfg), C.byref(self._state), what, 0, 0, self.width, self.height, 1,
                                   p.data_ptr(), self._mask_ptr(env_mask), None, None, ok.data_ptr(), self._stream()))
        return ok.bool()

    def place_agents(self, top=None, size=None, rand_dir=True, max_tries=1000):
        pass    # deprecated no-op upstream as well (base.py:710-712)

    # ---- tables: object descriptors, atlas, settings — derived in launch_tables.py, uploaded here -------
    def _obj_table(self, tile_size=None):
        return LT.obj_table(self.obj_reg, self.tile_size if tile_size is None else tile_size)

    def _host_tables(self, group=None):
        """(cfg without pointers, object table bytes, atlas bytes, atlas) of a view group (default: the first); hide_by goes on the group"""
        grp = self._groups[0] if group is None else group
        *tables, grp.hide_by = LT.group_tables(self, grp)
        return tuple(tables)

    _spawn_reject = property(lambda self: LT.reject_table(self, LT.read_settings(self)))     # read-only: the spawn's reject_fn as a table

    def _refresh_cfg(self, cfg):
        LT.apply_settings(cfg, LT.read_settings(self), cfg.spawn_reject)

    def _sync_tables(self):
        """Make the launch configs current: rebuild and upload the object table / atlas of every view group when a new
        object kind was registered since the last launch, apply the scalar settings when their value (LT.read_settings) changed."""
        if self._dry:
            return
        settings = LT.read_settings(self)
        stale = self._tables_version != self.obj_reg.version
        if not stale and settings == self._settings_seen:
            return
        rej = LT.reject_table(self, settings)       # (tabulated once for the env; uploaded when the table changed)
        if rej is not None and self._spawn_reject_key != rej.tobytes():
            self._spawn_reject_dev, self._spawn_reject_key = self._table_dev(rej), rej.tobytes()
        if stale:
            import torch
            self.invalidate_obs()               # (a tile index means other pixels once the atlas or the object table changes)
            self._release_spec()                # (... and the `specialize` handles were compiled for the old tables)
            for g in self._groups:
                t = LT.group_tables(self, g)
                g.cfg, g.atlas, flat = t.cfg, t.atlas, t.atlas_flat
                fits = LT.raster_fits(g.cfg, self._encoded)
                # specialize: the group's plain instantiation is asked for now; the atlas follows the name of the kernel to be launched
                name, generic = N.render_kernel_name(g.cfg) if fits else ("", 0)
                if fits and self._spec(g, N.WANT_PLAIN):
                    name, generic = g.spec_info[N.WANT_PLAIN]["kernel_name"], 0
                if name.endswith(", 2>"):
                    flat, g.cfg.atlas_gather_off = LT.gather_atlas(flat, g.cfg.n_tiles, g.tile_size)
                g.obj_dev = torch.from_numpy(t.obj_raw).to(self.device)
                g.atlas_dev = torch.from_numpy(flat).to(self.device)
                g.hide_dev = None if t.hide_by is None else torch.from_numpy(t.hide_by.view(np.int32)).to(self.device)
                g.cfg.obj, g.cfg.atlas = g.obj_dev.data_ptr(), g.atlas_dev.data_ptr()
                g.cfg.hide_by_obj = None if g.hide_dev is None else g.hide_dev.data_ptr()
                # the launcher's pick for this group (what rocprofv3 will call the launch); a warning when it is the fully generic one
                if self._encoded:
                    name, generic = "mg::encode_views_kernel<%d>" % (g.view_size if g.view_size in (5, 7, 9) else 0), 0
                g.kernel_name = name
                _warn_generic_kernel(g, generic, bool(g.cfg.prestige_mask))
        for g in self._groups:
            LT.apply_settings(g.cfg, settings, None if rej is None else self._spawn_reject_dev.data_ptr())
        g0 = self._groups[0]
        self._cfg, self.atlas, self._obj_dev, self._atlas_dev = g0.cfg, g0.atlas, g0.obj_dev, g0.atlas_dev
        self._tables_version, self._settings_seen = self.obj_reg.version, settings

    def _program(self, template, ops):
        import torch
        key = (template.tobytes(), tuple(ops))
        # a program with a PARAM op reads the env's parameter table right behind its template: all such programs of this env
        # share ONE buffer — template, then table —, whose head is rewritten (in stream order) when the template changes
        has_param = any(op.is_param or op.is_edits for op in ops)      # (... or an EDITS op: the edit table behind that one)
        if has_param and self._params.tpl != key[0]:
            t = np.zeros(self.cells_stride, np.uint8)
            t[:self.width * self.height] = template.reshape(-1)
            self._params.buf[:self.cells_stride].copy_(torch.from_numpy(t).to(self.device))
            self._params.tpl = key[0]
        prog = self._prog_cache.get(key)
        if prog is not None:
            return prog
        prog = N.GenProgram()
        # the struct carries a raw device pointer: the tensor it points at is kept on the struct
        # itself, so it lives exactly as long as any holder of the program (cache, `_reset_prog`)
        if has_param:
            prog._template_dev = self._params.buf
        else:
            t = np.zeros(self.cells_stride, np.uint8)
            t[:self.width * self.height] = template.reshape(-1)
            prog._template_dev = torch.from_numpy(t).to(self.device)
        prog.template_grid = prog._template_dev.data_ptr()
        prog.n_ops = len(ops)
        host_ops, reject = pack_program(ops, self.width, self.height, self.cells_stride, len(self.obj_reg.objs))
        # the ops live in device memory (MgGenProgram::ops), kept alive on the struct like the template
        prog._ops_dev = torch.from_numpy(np.frombuffer(bytes(host_ops), np.uint8).copy()).to(self.device)
        prog.ops = prog._ops_dev.data_ptr()
        prog.n_reject = 0 if reject is None else len(reject)
        if reject is not None:
            prog._reject_dev = torch.from_numpy(reject).to(self.device)
            prog.reject = prog._reject_dev.data_ptr()
        self._prog_cache[key] = prog
        return prog

    def _mask_ptr(self, env_mask):
        if env_mask is None:
            return None
        import torch
        if per_env.on_device(env_mask, self.device) and env_mask.dtype == torch.uint8:
            # bytes as they are (the kernels test nonzero): handed `done_t` itself, mg_reset keeps the done flags readable
            per_env.check_selectors(self.batch_size, env_mask, None, "env_mask")
            self._mask_keep = env_mask.to(self.device).contiguous()
        else:
            self._mask_keep = per_env.select(self.batch_size, self.device, env_mask, None, "env_mask")[0]
            if self._mask_keep.data_ptr() == self.done_t.data_ptr():       # step()'s bool `done`: a copy, so that mg_reset
                self._mask_keep = self._mask_keep.clone()                   # clears the flags of the envs it resets
        return C.c_void_p(self._mask_keep.data_ptr())

    # ---- the gym surface -----------------------------------------------------------------------------
    @_on_device
    def reset(self, env_mask=None, **kwargs):
        """Start a new episode in every env (or those selected by `env_mask`) and return the
        observation tensor (B, n, P, P, 3) — base.py:402-416."""
        template, ops = self._record_gen_grid()
        if self._dry:
            self._dry_trace = (template, ops)     # host-only instance: the recorded layout, nothing runs
            return None
        import torch
        self._sync_tables()
        prog = self._program(template, ops)
        self._reset_prog, self._retrace = prog, False
        mask_ptr, stream = self._mask_ptr(env_mask), self._stream()
        self._levels.apply(N.LEVEL_MASK, mask_ptr, stream)       # (set_levels: the envs that reset take their level's generator first)
        N.check(self._lib.mg_reset(C.byref(self._cfg), C.byref(self._state), C.byref(prog), mask_ptr, stream))
        if self.ep_return_t is not None:       # (mg_reset knows nothing of the episode accumulators)
            if env_mask is None:
                self.ep_return_t.zero_()
            else:
                self.ep_return_t.masked_fill_((self._mask_keep != 0).unsqueeze(1), 0.0)
        self._render()
        if self._explore is not None:
            self._explore.update(mask_ptr, stream)
        if self.encode_in_step:
            self._encode_into(self._encoding_buffer())
        if self.strict:
            self.check_errors()
        return self._package_obs()

    @_on_device
    def step(self, actions):
        """actions: (B, n) integer tensor (device preferred) or array-like -> (obs, rewards, done, {})
        with obs (B, n, P, P, 3) uint8, rewards (B, n) float32, done (B,) bool — base.py:501-653."""
        import torch
        if not torch.is_tensor(actions):
            actions = torch.as_tensor(np.asarray(actions))
        if actions.dim() == 1 and self.batch_size == 1:
            actions = actions.unsqueeze(0)
        assert actions.dim() == 2 and actions.shape[1] == len(self.agents) and actions.shape[0] == self.batch_size, \
            "actions must have shape (batch_size, n_agents)"                            # base.py:508
        if actions.dtype not in (torch.int64, torch.int32, torch.uint8):
            actions = actions.to(torch.int64)
        if actions.device != self.device or not actions.is_contiguous():
            actions = actions.to(self.device).contiguous()
        if self.strict and self._flag.raised():
            self.check_errors()   # an earlier launch recorded an error: raise it now (this is the only host sync)
        self._sync_tables()       # re-derives the launch configs only if a setting or the object registry changed
        if self.obs_buffers > 1:
            self._ring_i = (self._ring_i + 1) % self.obs_buffers
            r = self._ring[self._ring_i]
            self.obs, self.rewards, self.done_t = r["obs"], r["rewards"], r["done"]
            for g in self._groups:
                g.obs = g.ring[self._ring_i]
            self.done_b = self.done_t.view(torch.bool)
            self._state.done = self.done_t.data_ptr()
        stream = self._stream()
        prog = None
        if self.auto_reset:
            # envs that finish in this step start their next episode inside the same launch, before the
            # obs is rendered (their returned obs is the first obs of the new episode; `done` still
            # reports the end): the lane that computes an env's done flag runs its reset — no host sync,
            # no second launch.
            # first step after construction: subclass constructors finish configuring the
            # scenario after the base constructor's reset (cluttered.py:13-20)
            self._ensure_recorded()
            prog = C.byref(self._reset_prog)
        probe = self._probe          # bench.py: records an event on the launch stream around each launch
        if probe is not None:
            probe(0)
        # obs / rewards / done are views of the current buffer set (see `obs_buffers`)
        done = self.done_b
        if self._levels.on:     # the same call every step: which envs are about to reset is decided on the device
            self._levels.apply(N.LEVEL_PENDING if self.auto_reset_mode == "next_step" else N.LEVEL_PUBLISH, None, stream)
        r = self._ring[self._ring_i] if self._use_ep else None
        self._launch_step(actions, prog, stream, probe, None if r is None else C.byref(r["ep"]))
        if self._explore is not None:
            self._explore.update(None, stream)
        info = {}
        if self.episode_info:
            torch.eq(r["ep_flags"].unsqueeze(0), self._ep_vals, out=r["ep_bits"])
            info = r["info"]        # the info dict of the current buffer set
        if probe is not None:
            probe(2)
        if self.strict == "sync":
            self.check_errors()
        return self._package_obs(), self.rewards, done, info

    def _launch_step(self, actions, prog, stream, probe, ep):
        """The step and the observations it returns, as whichever library call this env's step is (step_launch.py: chosen at
        the first step, remembered).  `ep`: None, or the buffer set's MgEpisode (episode_info and / or auto_reset="next_step")."""
        self._plan.launch(self, actions, prog, stream, probe, ep)

    def _delta_wanted(self):
        return self._plan.delta_wanted(self)

    # what the library has not refused this env (read-only: the refusals are StepPlan's)
    _enc_fused = property(lambda self: "enc" not in self._plan.refused)           # the fused render with the encode
    _ep_fused = property(lambda self: "ep" not in self._plan.refused)             # ... with episode outputs
    _delta_ok = property(lambda self: self.obs_delta is not False and "delta" not in self._plan.refused)

    @property
    def encode_in_step(self):
        return self._encode_in_step

    @encode_in_step.setter
    def encode_in_step(self, on):       # (the one option callers switch on a live env: its step may be another call from now on)
        self._encode_in_step, self._plan.chosen = bool(on), None

    def invalidate_obs(self, buffer_set=None):
        """The observation tensors reset() / step() return are views of buffers the env owns and writes again `obs_buffers`
        steps later — with obs_delta only where the observation changed.  Call this after writing into one of them: the next
        step into every buffer set (or into `buffer_set`, an index of the ring) stores every byte.  One small fill per set on
        the current stream: ordered like a launch, and capturable."""
        ring = getattr(self, "_ring", ())
        for r in (ring if buffer_set is None else [ring[buffer_set]]):
            if r.get("sig") is not None:
                r["sig"].fill_(0xFF)

    def _launch_views(self, pixels=False):
        """one launch per view group (one group unless the agents' views differ) of the current state into the groups'
        observation buffers — encoded views: mg_encode_views —, or, `pixels`, the raster into their pixel buffers"""
        st, stream = C.byref(self._state), self._stream()
        if not (self._encoded and pixels):
            self.invalidate_obs(self._ring_i)       # (mg_render_obs writes the CURRENT set behind its signature's back)
        for g in self._groups:
            if self._encoded and not pixels:
                N.check(self._lib.mg_encode_views(C.byref(g.cfg), st, g.obs.data_ptr(), stream))
            elif self._spec(g, N.WANT_PLAIN):
                N.check(self._lib.mg_render_obs_spec(g.spec[N.WANT_PLAIN], C.byref(g.cfg), st, self._pixel_buffer(g).data_ptr(), stream))
            else:
                N.check(self._lib.mg_render_obs(C.byref(g.cfg), st, self._pixel_buffer(g).data_ptr(), None, None, None, stream))

    def _render(self, debug=False, group=None):
        import torch
        self._sync_tables()
        if debug:
            self.invalidate_obs(self._ring_i)
            g = self._groups[0] if group is None else group
            B, nv, vs = self.batch_size, len(g.members), g.view_size
            cells = torch.zeros((B, nv, vs, vs), dtype=torch.uint8, device=self.device)
            shown = torch.zeros_like(cells)
            vis = torch.zeros_like(cells)
            N.check(self._lib.mg_render_obs(C.byref(g.cfg), C.byref(self._state), self._pixel_buffer(g).data_ptr(),
                                            cells.data_ptr(), shown.data_ptr(), vis.data_ptr(), self._stream()))
            return cells, shown, vis
        self._launch_views()
        return None

    def _pixel_buffer(self, g):
        """the group's pixel observations: its obs buffer, or — encoded views — a scratch tensor made on first use"""
        if not self._encoded:
            return g.obs
        if g.pix is None:
            import torch
            g.pix = torch.zeros((self.batch_size, len(g.members), g.pixels, g.pixels, 3), dtype=torch.uint8, device=self.device)
        return g.pix

    def _pixel_views(self):
        """rasterise every group's pixel views of the current state (render()'s side columns) -> {group: tensor}"""
        if self._encoded:
            self._launch_views(pixels=True)
        else:
            self._render()
        return {id(g): self._pixel_buffer(g) for g in self._groups}

    @_on_device
    def gen_obs(self):
        """(B, n, P, P, 3) uint8, or the per-agent list for 'rich' agents (base.py:473-474)"""
        self._render()
        return self._package_obs()

    def _package_obs(self):
        """What reset()/step() hand back: the (B, n, P, P, 3) tensor when every agent uses the 'image'
        style (the fast path), else — like the reference's list of per-agent observations — a list
        with one entry per agent: its (B, P, P, 3) view or, for 'rich' agents, a dict of batched
        fields (base.py:459-471)."""
        if self._all_image and not self._hetero:
            return self.obs
        return [self._agent_obs(k) for k in range(self.num_agents)]

    @_on_device
    def gen_agent_obs(self, agent):
        """agent: a GridAgentInterface of this env or its index -> (B, P, P, 3) (base.py:453-471)"""
        k = agent if isinstance(agent, int) else self.agents.index(agent)
        self._render()
        return self._agent_obs(k)

    def _view_slot(self, k):
        """(view group, index inside it) of agent k"""
        for g in self._groups:
            if k in g.members:
                return g, g.members.index(k)
        raise IndexError(k)

    def _agent_obs(self, k):
        a = self.agents[k]
        g, slot = self._view_slot(k)
        pov = g.obs[:, slot]
        if a.observation_style == "image":
            return pov
        import torch
        ret = {"pov": pov}
        if a.observe_rewards:
            ret["reward"] = torch.zeros(self.batch_size, device=self.device)   # always 0 upstream (base.py:464,519)
        if a.observe_position:
            # np.array(pos) / np.array([W, H], dtype=float), `pos is None -> (0, 0)`: float64 like upstream
            wh = torch.tensor([self.width, self.height], dtype=torch.float64, device=self.device)
            pos = self.agent_pos[:, k].to(torch.float64)
            placed = (self.agent_flags[:, k] & N.AF_PLACED) != 0
            ret["position"] = torch.where(placed[:, None], pos, torch.zeros_like(pos)) / wh
        if a.observe_orientation:
            ret["orientation"] = self.agent_dir[:, k]
        return ret

    @_on_device
    def gen_obs_grid(self, agent):
        """(view cells (B, vs, vs) object ids indexed [i, j], visibility mask (B, vs, vs) bool) for one
        agent — base.py:418-451"""
        k = agent if isinstance(agent, int) else self.agents.index(agent)
        g, slot = self._view_slot(k)
        cells, _shown, vis = self._render(debug=True, group=g)
        return cells[:, slot], vis[:, slot].bool()

    @_on_device
    def _encode(self, vis_mask=None):
        import torch
        self._sync_tables()
        out = torch.empty((self.batch_size, self.width, self.height, 3), dtype=torch.uint8, device=self.device)
        vm = None
        if vis_mask is not None:
            vm = torch.as_tensor(vis_mask, device=self.device).to(torch.uint8).expand(
                self.batch_size, self.width, self.height).contiguous()
        return self._encode_into(out, vm)

    def _encode_into(self, out, vm=None):
        N.check(self._lib.mg_encode(C.byref(self._cfg), C.byref(self._state),
                                    None if vm is None else C.c_void_p(vm.data_ptr()), out.data_ptr(), self._stream()))
        return out

    def _encoding_buffer(self):
        """`grid_encoding` (encode_in_step): ONE tensor for the env's life — every step overwrites it"""
        if self.grid_encoding is None:
            import torch
            self.grid_encoding = torch.empty((self.batch_size, self.width, self.height, 3), dtype=torch.uint8, device=self.device)
        return self.grid_encoding

    @_on_device
    def check_errors(self):
        """Raise the reference's exception for the first env that hit one.  Host sync: waits for the launches
        queued so far, then reads ONE word (the error flag the kernels raise); the per-env codes are only
        fetched when it is set."""
        import torch
        torch.cuda.current_stream(self.device).synchronize()
        for s in list(self._launch_streams.values()):      # every stream a launch of this env went to
            s.synchronize()
        self._launch_streams.clear()
        if not self._flag.raised():
            return
        self._flag.clear()
        bad = torch.nonzero(self.error_t)
        if bad.numel():
            b = int(bad[0].item())
            code = int(self.error_t[b].item())
            self.error_t.zero_()
            msgs = {N.ERR_VALUE: "Environment can't handle action (env %d)." % b,
                    N.ERR_RECURSION: "Rejection sampling failed in place_obj (env %d)." % b,
                    N.ERR_TYPE: "toggle() takes 1 positional argument but 3 were given (Box, env %d)" % b,
                    N.ERR_ASSERT: "grid access out of bounds, or an agent left a cell it is not in (env %d)" % b,
                    N.ERR_ATTRIBUTE: "'NoneType' object has no attribute 'can_overlap' (env %d)" % b}
            raise N.ERR_EXC[code](msgs[code])

    def check_agent_position_integrity(self, title=""):
        """base.py:479-499 checks that every agent is in the grid exactly once (stack handling is
        error-prone there).  The packed records cannot express an agent in two places; what can be
        checked is that they are consistent: placed agents are inside the grid on a cell that can
        hold agents (one they overlap, or a door that was shut on them), stack ranks are a permutation, active implies placed.  Raises AssertionError
        (the reference drops into pdb)."""
        import torch
        pos, fl, rk = self.agent_pos, self.agent_flags, self.agent_rank
        placed = (fl & N.AF_PLACED) != 0
        ok = ~placed | ((pos[..., 0] < self.width) & (pos[..., 1] < self.height))
        cell = (pos[..., 0] * self.height + pos[..., 1]).clamp(max=self.width * self.height - 1)
        base = torch.gather(self.grid_state[:, :self.width * self.height].long(), 1, cell)
        holds = torch.tensor([True] + [bool(o.can_hold_agents()) for o in self.obj_reg.objs[1:]], device=self.device)
        ok &= ~placed | holds[base]
        ok &= ((fl & N.AF_ACTIVE) == 0) | placed
        ok &= (rk.sort(dim=1).values == torch.arange(self.num_agents, device=self.device)).all(dim=1, keepdim=True)
        if not bool(ok.all()):
            bad = torch.nonzero(~ok.all(dim=1))[:8, 0].tolist()
            raise AssertionError("%s > Failed integrity test! envs %s" % (title, bad))

    # ---- agent state views (per-env state lives in HBM, not on the agent objects) -------------------------
    def _rec_byte(self, i):
        return ((self.agent_state >> (8 * i)) & 0xFF)

    @property
    def agent_pos(self):
        """(B, n, 2) int64"""
        import torch
        return torch.stack([self._rec_byte(N.AG_X), self._rec_byte(N.AG_Y)], dim=-1)

    @property
    def agent_dir(self):
        return self._rec_byte(N.AG_DIR)

    @property
    def agent_flags(self):
        return self._rec_byte(N.AG_FLAGS)

    @property
    def agent_active(self):
        return (self.agent_flags & N.AF_ACTIVE) != 0

    @property
    def agent_done(self):
        return (self.agent_flags & N.AF_DONE) != 0

    @property
    def agent_carrying(self):
        return self._rec_byte(N.AG_CARRY)

    @property
    def agent_rank(self):
        return self._rec_byte(N.AG_RANK)

    @property
    def step_count(self):
        return self.step_count_t

    def set_agent(self, k, x=None, y=None, dir=None, carrying=None, env_mask=None):
        """Test / scenario-building helper: overwrite fields of agent k's record in the selected envs.
        Moving an agent this way gives it the highest arrival rank (as a fresh placement would)."""
        import torch
        m = torch.ones(self.batch_size, dtype=torch.bool, device=self.device) if env_mask is None else \
            per_env.select(self.batch_size, self.device, env_mask, None, "set_agent")[0].view(torch.bool)
        rec = self.agent_state

        def setb(col, i, v):
            return (col & ~(0xFF << (8 * i))) | (int(v) << (8 * i))
        if x is not None or y is not None:
            n = self.num_agents
            old = self._rec_byte(N.AG_RANK)[:, k:k + 1]
            rk = self._rec_byte(N.AG_RANK)
            rk = torch.where(rk > old, rk - 1, rk)
            rk[:, k] = n - 1
            new = (rec & ~(0xFF << (8 * N.AG_RANK))) | (rk << (8 * N.AG_RANK))
            rec[m] = new[m]
        col = rec[:, k].clone()
        if x is not None:
            col = setb(col, N.AG_X, x)
        if y is not None:
            col = setb(col, N.AG_Y, y)
        if dir is not None:
            col = setb(col, N.AG_DIR, dir % 4)
        if carrying is not None:
            col = setb(col, N.AG_CARRY, self.obj_reg.get_key(carrying) if isinstance(carrying, WorldObj) else carrying)
        rec[:, k] = torch.where(m, col, rec[:, k])

    # ---- RNG state exchange with numpy (tests / checkpoints) -------------------------------------------
    def numpy_rng_state(self, b=0):
        """env b's generator as `np.random.RandomState.get_state()` would report it: (key[624], pos).
        The device keeps the *lazy* form plus a look-ahead head (see mg_core.h): words below `mt_pos`
        are already regenerated, the head holds the 16 outputs before it.  numpy regenerates whole
        blocks, so the not-yet-regenerated tail is advanced here; when the head reaches across a block
        boundary the words regenerated ahead of numpy's position are wound back (the twist is
        invertible except for the low 31 bits of word 0, which MT19937 never reads: reported as 0)."""
        mt = [int(v) for v in self.mt_state[b].cpu().numpy().view(np.uint32)]
        G = int(self.mt_pos[b].item())
        return seeding.numpy_form(mt, G, N.MT_HEAD)

    _STATE_KEYS = ("grid_state", "agent_state", "mt_state", "mt_pos", "mt_head", "step_count_t", "done_t", "error_t")

    def state_dict(self):
        """The env batch's whole state as tensors (a checkpoint).  `version` names the layout: the packed agent
        records and the RNG in its lazy form with the look-ahead head (mt_pos counts the words generated INTO the
        head, not the words consumed) — an older checkpoint is a different RNG stream position, not this one."""
        import torch
        sd = {k: getattr(self, k).clone() for k in self._STATE_KEYS}
        if self.prestige_t is not None:
            sd["prestige_t"] = self.prestige_t.clone()
        if self.ep_return_t is not None:        # episode_info: the running episodes' return accumulators
            sd["ep_return_t"] = self.ep_return_t.clone()
        if self._params.decl:             # `_gen_grid` names parameters: the table they are read from
            sd["params_t"] = self.params_t.clone()
        if self.level_edits:              # the envs' edit lists
            sd["edits_t"] = self.edits_t.clone()
        if self._explore is not None:     # explore=True: the maps of the running episodes
            sd.update(self._explore.state())
        if self._levels.on:                     # set_levels: the running episodes' levels, and the seed each env resets to next
            sd["episode_level_t"] = self.episode_level.clone()      # (resolved through the bank now: a bank is no part of a checkpoint)
            sd["level_next_t"] = self._levels.next()
        sd["version"] = torch.tensor(STATE_DICT_VERSION)
        return sd

    def load_state_dict(self, sd):
        want = set(self._STATE_KEYS) | {"version"} | ({"prestige_t"} if self.prestige_t is not None else set())
        want |= {"ep_return_t"} if self.ep_return_t is not None else set()
        want |= {"params_t"} if self._params.decl else set()
        want |= {"edits_t"} if self.level_edits else set()
        levels = {"episode_level_t", "level_next_t"} & set(sd.keys())       # (optional: a checkpoint without them loads as before)
        if levels and len(levels) != 2:
            raise KeyError("load_state_dict: 'episode_level_t' and 'level_next_t' come together")
        if levels:
            if tuple(sd["level_next_t"].shape) != (self.batch_size,):
                raise ValueError("load_state_dict: level_next_t has shape %s, expected %s" % (tuple(sd["level_next_t"].shape), (self.batch_size,)))
            self._levels.enable()
        want |= levels
        maps = self._explore.keys_of(sd) if self._explore is not None else set()
        want |= maps
        if set(sd.keys()) != want:
            raise KeyError("load_state_dict: expected exactly the keys %s, got %s (a checkpoint without "
                           "'version' / 'mt_head' predates the look-ahead RNG form and cannot be resumed)"
                           % (sorted(want), sorted(sd.keys())))
        if int(sd["version"]) != STATE_DICT_VERSION:
            raise ValueError("load_state_dict: checkpoint version %d, this engine reads %d"
                             % (int(sd["version"]), STATE_DICT_VERSION))
        for k in want - {"version", "level_next_t"}:
            if tuple(sd[k].shape) != tuple(getattr(self, k).shape):
                raise ValueError("load_state_dict: %s has shape %s, expected %s" % (k, tuple(sd[k].shape),
                                                                                    tuple(getattr(self, k).shape)))
        for k in want - {"version", "level_next_t"}:
            getattr(self, k).copy_(sd[k])
        if levels:      # in the seeds form: the env's own bank, row b seeded with env b's next level
            self.set_levels(seeds=sd["level_next_t"].to(self.device))
        if self._explore is not None and not self._explore.complete(maps):      # (all of them: the invariants between them hold)
            self._explore.clear()
        self.invalidate_obs()
        if bool((self.error_t != 0).any()):
            self._flag._host[0] = 1          # the restored batch carries recorded errors (whatever `strict` is:
                                             # check_errors() looks at the flag first)

    # ---- plain-data description (parity tests hand this to the oracle) -----------------------------------
    def scenario_spec(self):
        def ospec(o):
            if o is None:
                return None
            d = dict(type=o.__class__.__name__, color=o.color, state=o.state)
            if isinstance(o, Goal):
                d["reward"] = o.reward
            if isinstance(o, BonusTile):
                d.update(reward=o.reward, penalty=o.penalty, bonus_id=o.bonus_id, n_bonus=o.n_bonus,
                         initial_reward=o.initial_reward, reset_on_mistake=o.reset_on_mistake)
            return d


        def aspec(a):
            d = dict(color=a.color)
            if a.spawn_delay:
                d["spawn_delay"] = a.spawn_delay
            if a.hide_item_types:
                d["hide_item_types"] = list(a.hide_item_types)
            if a.color == "prestige":
                d.update(prestige_beta=a.prestige_beta, prestige_scale=a.prestige_scale)
            if self._hetero:
                d["view"] = dict(view_size=a.view_size, tile_size=a.view_tile_size, view_offset=a.view_offset,
                                 see_through_walls=bool(a.see_through_walls))
            if a.observation_style == "rich":
                d["rich"] = {k: True for k in ("observe_rewards", "observe_position", "observe_orientation")
                             if getattr(a, k)}
            return d
        extra = {}
        if self.agent_spawn_kwargs:
            extra["agent_spawn"] = {k: (tuple(v) if k in ("top", "size") else v)
                                    for k, v in self.agent_spawn_kwargs.items() if k != "reject_fn"}
            if self.agent_spawn_kwargs.get("reject_fn") is not None:
                x0, y0, x1, y1 = self._place_region(self.agent_spawn_kwargs.get("top"), self.agent_spawn_kwargs.get("size"))
                t = self._reject_table(self.agent_spawn_kwargs["reject_fn"], (x0, y0, x1, y1))
                extra["agent_spawn"]["reject"] = tuple((int(x), int(y)) for x, y in np.argwhere(t))
        return dict(W=self.width, H=self.height, agents=[aspec(a) for a in self.agents], **extra,
                    view_size=self.view_size, tile_size=self.tile_size, view_offset=self.view_offset,
                    see_through_walls=self.see_through_walls, max_steps=self.max_steps,
                    reward_decay=bool(self.reward_decay), ghost_mode=self.ghost_mode,
                    respawn=bool(self.respawn), objects=[ospec(o) for o in self.obj_reg.objs],
                    wall_obj=self.obj_reg.find(Wall()), gen_ctor=decode_program(self._spec_ctor or self._spec_last, self.width, self.height),
                    gen_reset=decode_program(self._spec_last, self.width, self.height))

    @_on_device
    def render(self, mode="rgb_array", close=False, highlight=True, tile_size=TILE_PIXELS, show_agent_views=True,
               max_agents_per_col=3, agent_col_width_frac=0.3, agent_col_padding_px=2, pad_grey=100, env_ids=None):
        """Whole-grid human view (base.py:714-795): every cell at `tile_size` pixels, cells visible to
        some active agent highlighted, and (show_agent_views) the agents' own observations stacked in
        side columns.  Returns a uint8 tensor (H_px, W_px, 3) for env 0, or (K, H_px, W_px, 3) for
        `env_ids`.  There is no window: mode='human' returns the image as well."""
        import torch
        if close:
            return None
        if tile_size % 4 != 0 or not (4 <= tile_size <= 64):
            raise NotImplementedError("render(tile_size=) must be a multiple of 4 in [4, 64]")
        single = env_ids is None
        ids = torch.as_tensor([0] if single else env_ids, dtype=torch.int32).reshape(-1)
        K = int(ids.numel())
        if K and (int(ids.min()) < 0 or int(ids.max()) >= self.batch_size):
            raise IndexError("render(env_ids=): env index out of range [0, %d)" % self.batch_size)
        ids = ids.to(self.device)
        self._sync_tables()
        key = (self.obj_reg.version, tile_size)
        if getattr(self, "_frame_atlas_key", None) != key:
            fa, _, _ = rendering.build_atlas(self.obj_reg.objs, [a.color for a in self.agents], tile_size,
                                             prestige_sprites=any(self._prestige))
            self._frame_atlas = torch.from_numpy(np.ascontiguousarray(fa[0])).to(self.device)
            self._frame_atlas_key = key
            self._frame_amax = 0
            if any(self._prestige):
                for d in range(4):
                    self._frame_amax |= int(fa[0, fa.shape[1] - 4 + d][..., 0].max()) << (8 * d)
        Hp, Wp = self.height * tile_size, self.width * tile_size
        # (the frame kernel keeps two bytes per cell in one workgroup's LDS — the cell's tile index and its highlight bit; the grid
        # is read where it lives —: every grid up to 255 x 255 fits, next to the recoloured sprites of up to ~10 'prestige' agents)
        lds = 2 * ((self.width * self.height + 7) // 8 * 8) + 1024 + 4 * self.num_agents * self.view_size + (
            self.num_agents * tile_size * tile_size * 3 if any(self._prestige) else 0)
        if lds > 160 * 1024:
            raise NotImplementedError("render(): the whole-grid image of a %d x %d grid with %d 'prestige' agents at %d-pixel tiles "
                                      "needs more than the 160 KiB of LDS of a workgroup; use a smaller tile_size"
                                      % (self.width, self.height, self.num_agents, tile_size))
        img = torch.empty((K, Hp, Wp, 3), dtype=torch.uint8, device=self.device)
        N.check(self._lib.mg_render_frame(C.byref(self._cfg), C.byref(self._state), ids.data_ptr(), K,
                                          self._frame_atlas.data_ptr(), tile_size, int(bool(highlight)),
                                          self._frame_amax, img.data_ptr(), self._stream()))
        if show_agent_views:
            # side columns (base.py:764-786): views enlarged by an integer factor, max_agents_per_col
            # per column, centred on a grey background.  (The reference mixes shape[0] / shape[1]
            # here; kept as written — images are square in every shipped scenario.)
            tpw = int(Hp * agent_col_width_frac - 2 * agent_col_padding_px)
            tph = (Wp - 2 * agent_col_padding_px) // max_agents_per_col
            pix = self._pixel_views()
            cols = []
            for c0 in range(0, self.num_agents, max_agents_per_col):
                col = torch.full((K, Hp, tpw + 2 * agent_col_padding_px, 3), pad_grey, dtype=torch.uint8,
                                 device=self.device)
                for j, k in enumerate(range(c0, min(c0 + max_agents_per_col, self.num_agents))):
                    g, slot = self._view_slot(k)                            # each view at its own integer zoom
                    P = g.pixels
                    f = int(min(tpw / P, tph / P))
                    view = pix[id(g)][ids.long(), slot]                     # (K, P, P, 3)
                    view = view.repeat_interleave(f, dim=1).repeat_interleave(f, dim=2) if f > 0 else view[:, :0, :0]
                    vh = vw = P * f
                    o0 = (tph - vw) // 2 + agent_col_padding_px + j * tph
                    o1 = (tpw - vh) // 2 + agent_col_padding_px
                    col[:, o0:o0 + vh, o1:o1 + vw] = view
                cols.append(col)
            img = torch.cat([img] + cols, dim=2)
        return img[0] if single else img

    def __str__(self):
        return "<%s B=%d %dx%d n_agents=%d>" % (self.__class__.__name__, self.batch_size, self.width,
                                                self.height, self.num_agents)
