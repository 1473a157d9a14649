"""What every launch reads, derived on the host: per view group the launch config (MgConfig without device pointers), the
object-descriptor table, the sprite atlas (`group_tables`) and its copy in the raster's LDS layout (`gather_atlas`); per env
the scalar settings the reference reads on every step (`read_settings`: ONE immutable value — what step() compares, what
`apply_settings` writes, what names the tabulated `reject_fn` of the agents' spawn).  numpy and ctypes only: nothing here
touches a device or writes on the env; the uploads are MultiGridEnv._sync_tables."""
import ctypes as C
import os
import warnings
from collections import namedtuple

import numpy as np

from . import _native as N
from . import rendering
from .agents import GridAgentInterface
from .objects import COLOR_TO_IDX, OBJECT_TYPES, BonusTile, Box, Door, Goal, Key

GroupTables = namedtuple("GroupTables", "cfg obj_raw atlas_flat atlas hide_by")
# spawn: (x0, y0, x1, y1, max_tries) as clamped; reject: None, or (id(fn), fn) of agent_spawn_kwargs['reject_fn'] — compared by
# identity, and the id stays that function's while the value lives; agents: (spawn_delay, prestige_beta, prestige_scale) of each
Settings = namedtuple("Settings", "max_steps reward_decay ghost_mode respawn spawn reject agents")
_new = tuple.__new__


def read_settings(env):
    """The scalar settings the reference reads on every step (max_steps, reward_decay, ghost_mode, respawn,
    agent_spawn_kwargs, the agents' spawn_delay / prestige parameters) as ONE value that is equal exactly when the launch
    config it makes is: changing an attribute between steps changes this value, and the next launch sees it, as upstream.
    Every step pays for this call: an agent's numbers stay as they are (3 and 3.0 are one value; apply_settings converts them)."""
    spawn, reject = (0, 0, env.width, env.height, 100000), None     # (no keyword: what the lines below make of {})
    kw = env.agent_spawn_kwargs
    if kw:      # place_obj(agent, **agent_spawn_kwargs) (base.py:411, 505, 643)
        kw = dict(kw)
        reject_fn, top, size, max_tries = kw.pop("reject_fn", None), kw.pop("top", None), kw.pop("size", None), kw.pop("max_tries", 1e5)
        if kw:
            raise TypeError("place_obj() got an unexpected keyword argument %r" % sorted(kw)[0])
        spawn = (*env._place_region(top, size), int(max(1, min(max_tries, 1e5))))
        reject = None if reject_fn is None else (id(reject_fn), reject_fn)
    # upstream tests `ghost_mode is False` when moving (base.py:541) but `not ghost_mode` when placing
    # (base.py:683): they differ for falsy non-False values such as 0 or None
    ghost = env.ghost_mode
    return _new(Settings, (int(env.max_steps), 1 if env.reward_decay else 0, (1 if ghost is not False else 0) | (2 if ghost else 0),
                           1 if env.respawn else 0, spawn, reject,
                           tuple([(a.spawn_delay, a.prestige_beta, a.prestige_scale) for a in env.agents])))


def apply_settings(cfg, settings, reject_ptr):
    """write a settings value into one launch config; reject_ptr: where `reject_table(env, settings)` lies for the launch, or None"""
    cfg.max_steps, cfg.reward_decay, cfg.ghost_mode, cfg.respawn = settings[:4]
    cfg.spawn_x0, cfg.spawn_y0, cfg.spawn_x1, cfg.spawn_y1, cfg.spawn_max_tries = settings.spawn
    cfg.spawn_reject = reject_ptr
    for k, (delay, beta, scale) in enumerate(settings.agents):
        if delay < 0:
            raise ValueError("spawn_delay must be >= 0")
        cfg.spawn_delay[k], cfg.prestige_beta[k], cfg.prestige_scale[k] = int(delay), float(beta), float(scale)
    cfg.any_spawn_delay = int(any(a[0] != 0 for a in settings.agents))


def reject_table(env, settings):
    """agent_spawn_kwargs['reject_fn'] (base.py:411, 505, 643 -> :700-701), tabulated like place_obj's: (W, H) uint8, or None"""
    return None if settings.reject is None else env._reject_table(settings.reject[1], settings.spawn[:4])


def obj_table(obj_reg, tile_size):
    objs = obj_reg.objs
    tab = (N.ObjDesc * len(objs))()
    for i, o in enumerate(objs):
        if o is None:
            continue
        d = tab[i]
        d.type_idx, d.color_idx, d.state = o.encode()
        f = 0
        f |= N.OF_CAN_OVERLAP if o.can_overlap() else 0
        f |= N.OF_CAN_PICKUP if o.can_pickup() else 0
        f |= N.OF_SEE_BEHIND if o.see_behind() else 0
        f |= N.OF_ENDS_EPISODE if o.ends_episode else 0
        f |= N.OF_IS_KEY if isinstance(o, Key) else 0
        f |= N.OF_IS_BOX if isinstance(o, Box) else 0
        if isinstance(o, Door):
            f |= N.OF_IS_DOOR
            if o.state == Door.LOCKED:
                f |= N.OF_DOOR_LOCKED
            d.unlock_next = obj_reg.find(Door(o.color, Door.CLOSED))
            d.toggle_next = obj_reg.find(Door(o.color, Door.OPEN if o.state == Door.CLOSED else Door.CLOSED))
        d.flags = f
        try:    # "a corner of the plain tile is black" (the border rule of render_tile, base.py:296-298)
            plain = rendering.render_sprite(o.sprite_ops(), tile_size)
        except NotImplementedError:
            plain = np.zeros((tile_size, tile_size, 3), np.uint8)
        d.flags2 = int((plain[[0, 0, -1, -1], [0, -1, 0, -1]] == 0).all(axis=-1).any())
        if isinstance(o, Goal):
            d.reward_kind, d.reward = 1, float(o.reward)
        elif isinstance(o, BonusTile):
            d.reward_kind, d.reward, d.penalty = 2, float(o.reward), float(o.penalty)
            d.bonus_id, d.n_bonus = o.bonus_id, o.n_bonus
            d.bonus_flags = (1 if o.initial_reward else 0) | (2 if o.reset_on_mistake else 0)
    return tab


def group_tables(env, group):
    """Everything the kernels need that is derived on the host from the object registry, the agent interfaces and the
    settings, for one view group: (cfg without device pointers, object table bytes, atlas bytes, atlas array, hide_by —
    per object id the agents that hide its type, None when nobody hides anything)."""
    objs = env.obj_reg.objs
    atlas, ovl_slot, n_slots = rendering.build_atlas(objs, [a.color for a in env.agents], group.tile_size,
                                                     prestige_sprites=any(env._prestige))
    tab = obj_table(env.obj_reg, group.tile_size)
    for i in range(len(objs)):
        tab[i].ovl_slot = ovl_slot[i]
    raw = np.frombuffer(bytes(tab), dtype=np.uint8).copy()
    flat = atlas.reshape(-1)
    flat = np.concatenate([flat, np.zeros((-flat.size) % 16 + 16, np.uint8)])
    cfg = N.Config()
    cfg.B, cfg.W, cfg.H, cfg.n_agents = env.batch_size, env.width, env.height, env.num_agents
    cfg.view_size, cfg.tile_size = group.view_size, group.tile_size
    cfg.view_offset, cfg.see_through_walls = group.view_offset, int(group.see_through_walls)
    if env._hetero:                       # this group's agents only are rendered with this geometry
        cfg.n_view = len(group.members)
        for i, k in enumerate(group.members):
            cfg.view_agent[i] = k
    cfg.cells_stride = env.cells_stride
    cfg.n_obj, cfg.n_ovl_slots, cfg.n_tiles = len(objs), n_slots, atlas.shape[1]
    cfg.agent_type_idx = OBJECT_TYPES.index(GridAgentInterface)
    for k, a in enumerate(env.agents):
        cfg.agent_color_idx[k] = COLOR_TO_IDX[a.color]
        cfg.prestige_mask |= int(env._prestige[k]) << k     # 'prestige' agents (agents.py:92-119, 141-153): per-env recoloured sprites
    if cfg.prestige_mask:
        cfg.prestige_sprite_tile = atlas.shape[1] - 4
        for d in range(4):      # max alpha of the (white) sprite per dir = max of blend_tiles' alpha map
            cfg.prestige_amax[d] = int(atlas[0, atlas.shape[1] - 4 + d][..., 0].max())
    # hide_item_types (base.py:441-449): per object id the agents that hide its type (bit k = agent k; a device table),
    # and the agents that hide 'Agent'
    hide_by = np.zeros(len(objs), np.uint32)
    for k, a in enumerate(env.agents):
        for i, o in enumerate(objs):
            if o is not None and o.type in a.hide_item_types:
                hide_by[i] |= np.uint32(1 << k)
        if "Agent" in a.hide_item_types:
            cfg.hide_agent_mask |= 1 << k
    cfg.any_hide = int(cfg.hide_agent_mask != 0 or bool(hide_by.any()))
    apply_settings(cfg, read_settings(env), None)
    return GroupTables(cfg, raw, flat, atlas, hide_by if hide_by.any() else None)


def raster_fits(cfg, encoded):
    """the obs kernel keeps 4 waves of per-env scratch (and the atlas, when it fits) in one workgroup's LDS: ask the library,
    which owns that layout, before anything is uploaded"""
    need = N.lib().mg_render_obs_lds_bytes(C.byref(cfg))
    fits = 0 <= need <= 160 * 1024
    if not fits and not encoded:      # (encoded views have no per-env pixel scratch)
        raise NotImplementedError(
            "this configuration needs %d KiB of LDS per workgroup for 4 waves of per-env scratch; the obs "
            "kernel has 160 KiB — with 'prestige' agents reduce their number or the tile size (every one of them has "
            "its four recoloured sprites there); otherwise the number of agents / the view size" % (need // 1024))
    return fits


def gather_atlas(atlas_flat, n_tiles, tile_size):
    """The gather instantiations (raster 2: 5-, 6-, 7-, 9- ... 12-pixel tiles; examples/human_player.py's shape) take the atlas
    in the raster's own LDS layout when the host has it ready — behind the plain one, `atlas_gather_off` bytes on —: building
    it per workgroup was 5 us of human_player's 130 us launch (20 instructions per dword, 45 dwords per thread), 1 - 1.6 % of
    the others'.  Every pixel row of every tile at 16 + row * stride, 32 zero bytes behind the last, offset and length multiples
    of 16.  Returns (atlas_flat with the copy behind it, the offset); (atlas_flat, 0) with MG_NO_GATHER_ATLAS set."""
    if os.environ.get("MG_NO_GATHER_ATLAS"):
        return atlas_flat, 0
    seg = 3 * tile_size
    stride = (16 + seg + 3) // 4 * 4
    rows = np.ascontiguousarray(atlas_flat[:4 * n_tiles * tile_size * seg]).reshape(-1, seg)
    padded = np.zeros((rows.shape[0], stride), np.uint8)
    padded[:, 16:16 + seg] = rows
    off = (atlas_flat.size + 15) // 16 * 16
    tail = 32 + (-(padded.size + 32)) % 16
    return np.concatenate([atlas_flat, np.zeros(off - atlas_flat.size, np.uint8), padded.reshape(-1), np.zeros(tail, np.uint8)]), off


_GENERIC_WARNED = set()


def _warn_generic_kernel(g, generic, prestige):
    """mg_render_kernel_name's bits 1 | 2: view size AND tile size are run-time values of the launch — the fully generic
    instantiation of the observation kernel (assemble-and-stream raster, run-time dividers, a 15-row shadow cast, 8- / 4-wave
    workgroups), measured 2-2.4x slower than a specialised one (profiles/r05: view 9 at 5-pixel tiles 0.3136 -> 0.1360 ms
    when it got its own).  Said once per configuration and process, naming what is specialised nearby."""
    if generic != 3:
        return
    key = (g.view_size, g.tile_size, prestige, g.kernel_name)
    if key in _GENERIC_WARNED:
        return
    _GENERIC_WARNED.add(key)
    if g.kernel_name.endswith(", 3>"):      # the grid-in-place variant: nothing about the view or the tiles would change it
        warnings.warn("marlgrid_amd: this grid does not fit the observation kernel's LDS next to its per-cell agent maps (grids up "
                      "to ~140 x 140, ~110 x 110 with hide_item_types, are staged there): it is read in place by the fully run-time "
                      "instantiation (%s) — correct, every size up to 255 x 255, but slower per observation byte than a staged grid"
                      % g.kernel_name, RuntimeWarning, stacklevel=4)
        return
    near = []
    if prestige:
        near.append("'prestige' agents: view_size 7 with any view_tile_size (5, 8 and 11 fastest), or view_tile_size 8 / 16 / 32 with any view")
    else:
        if g.view_size > 9:
            near.append("view_size %d with view_tile_size 8, 16 or 32%s" % (g.view_size, ", or 5" if g.view_size in (11, 13, 15) else ""))
        near.append("view_size 3 ... 9 with this view_tile_size (%d)" % g.tile_size)
        if g.view_size not in (11, 13, 15):
            near.append("view_size 11 / 13 / 15 with view_tile_size 5")
    warnings.warn("marlgrid_amd: view_size=%d, view_tile_size=%d%s takes the fully run-time instantiation of the observation "
                  "kernel (%s): correct, but 2-2.4x slower than a specialised one.  Specialised nearby: %s."
                  % (g.view_size, g.tile_size, " with 'prestige' agents" if prestige else "", g.kernel_name, "; ".join(near)),
                  RuntimeWarning, stacklevel=4)
