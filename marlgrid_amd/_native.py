"""ctypes binding of libmarlgrid_hip.so (C ABI: include/marlgrid_hip.h).

The product path has NO CPU fallback: if the HIP library is missing or does not load, importing
this module raises.  Build it with `python -c "import __graft_entry__ as g; g.build()"` or
`marlgrid_amd/csrc/build.sh`.
"""
import ctypes as C
import os

MAX_AGENTS, MAX_OBJ, MAX_GEN, MAX_VIEW, KEY_WORDS, MT_N, MT_HEAD = 32, 256, 1024, 31, 2, 624, 16
ABI_VERSION = 6
# `_rand_int` draws of a reset program (MG_GEN_* in the C header): an operand with GEN_SYM is `const +- draw[r]`
GEN_DRAWS, GEN_SYM, GEN_NEG, GEN_DRAW_SHIFT = 8, 0x40000000, 0x20000000, 16
GEN_PARAM = -2              # GenOp.max_tries of a PARAM op (MG_GEN_PARAM): draw[obj] = clamp(params[env][y0], x0, x1 - 1), no RNG word
GEN_EDITS = -3              # GenOp.max_tries of an EDITS op (MG_GEN_EDITS): `count` entries (x, y, obj, on) of the env's edit list
GEN_MAX_EDITS = 64          # ... at most (MG_GEN_MAX_EDITS)
# ... and the guard of an op, in the upper bits of GenOp.obj (MG_GEN_GUARD*): the op runs only where lo <= draw[r] <= hi
GEN_GUARD, GEN_GUARD_DRAW_SHIFT, GEN_GUARD_HI_SHIFT, GEN_GUARD_LO_SHIFT = 0x40000000, 24, 16, 8

OK = 0
ERR_VALUE, ERR_RECURSION, ERR_TYPE, ERR_ASSERT, ERR_ATTRIBUTE = 1, 2, 3, 4, 5
ERR_EXC = {ERR_VALUE: ValueError, ERR_RECURSION: RecursionError, ERR_TYPE: TypeError,
           ERR_ASSERT: AssertionError, ERR_ATTRIBUTE: AttributeError}

AG_X, AG_Y, AG_DIR, AG_FLAGS, AG_CARRY, AG_RANK, AG_BONUS = range(7)
AF_ACTIVE, AF_DONE, AF_PLACED, AF_EVICTED = 1, 2, 4, 8
OF_CAN_OVERLAP, OF_CAN_PICKUP, OF_SEE_BEHIND, OF_ENDS_EPISODE = 1, 2, 4, 8
OF_IS_KEY, OF_IS_DOOR, OF_IS_BOX, OF_DOOR_LOCKED = 16, 32, 64, 128


class ObjDesc(C.Structure):
    _fields_ = [("type_idx", C.c_uint8), ("color_idx", C.c_uint8), ("state", C.c_uint8), ("flags", C.c_uint8),
                ("reward_kind", C.c_uint8), ("toggle_next", C.c_uint8), ("unlock_next", C.c_uint8),
                ("ovl_slot", C.c_uint8),
                ("bonus_id", C.c_uint8), ("n_bonus", C.c_uint8), ("bonus_flags", C.c_uint8), ("flags2", C.c_uint8),
                ("pad1", C.c_uint32), ("reward", C.c_double), ("penalty", C.c_double)]


assert C.sizeof(ObjDesc) == 32


class Config(C.Structure):
    _fields_ = [("B", C.c_int32), ("W", C.c_int32), ("H", C.c_int32), ("n_agents", C.c_int32),
                ("view_size", C.c_int32), ("tile_size", C.c_int32), ("view_offset", C.c_int32),
                ("see_through_walls", C.c_int32),
                ("max_steps", C.c_int32), ("reward_decay", C.c_int32), ("ghost_mode", C.c_int32),
                ("respawn", C.c_int32),
                ("cells_stride", C.c_int32), ("n_obj", C.c_int32), ("n_ovl_slots", C.c_int32),
                ("n_tiles", C.c_int32), ("agent_type_idx", C.c_int32), ("atlas_gather_off", C.c_int32),
                ("spawn_x0", C.c_int32), ("spawn_y0", C.c_int32), ("spawn_x1", C.c_int32), ("spawn_y1", C.c_int32),
                ("spawn_max_tries", C.c_int32),
                ("n_view", C.c_int32), ("view_agent", C.c_uint8 * MAX_AGENTS),
                ("agent_color_idx", C.c_uint8 * MAX_AGENTS),
                ("any_spawn_delay", C.c_int32), ("spawn_delay", C.c_int32 * MAX_AGENTS),
                ("prestige_mask", C.c_uint32), ("prestige_amax", C.c_uint8 * 4), ("prestige_sprite_tile", C.c_int32),
                ("prestige_beta", C.c_double * MAX_AGENTS), ("prestige_scale", C.c_double * MAX_AGENTS),
                ("any_hide", C.c_int32), ("hide_agent_mask", C.c_uint32), ("hide_by_obj", C.c_void_p),
                ("obj", C.c_void_p), ("atlas", C.c_void_p), ("spawn_reject", C.c_void_p)]


class State(C.Structure):
    _fields_ = [("grid", C.c_void_p), ("agents", C.c_void_p), ("mt", C.c_void_p), ("mt_pos", C.c_void_p),
                ("step_count", C.c_void_p), ("done", C.c_void_p), ("error", C.c_void_p), ("prestige", C.c_void_p),
                ("mt_head", C.c_void_p), ("error_flag", C.c_void_p)]


class GenOp(C.Structure):
    _fields_ = [("obj", C.c_int32), ("count", C.c_int32), ("max_tries", C.c_int32),
                ("x0", C.c_int32), ("y0", C.c_int32), ("x1", C.c_int32), ("y1", C.c_int32), ("reject", C.c_int32)]


class GenProgram(C.Structure):
    _fields_ = [("template_grid", C.c_void_p), ("n_ops", C.c_int32), ("ops", C.c_void_p),      # ops: DEVICE memory, GenOp [n_ops]
                ("reject", C.c_void_p), ("n_reject", C.c_int32)]


class Episode(C.Structure):
    """MgEpisode: the extra argument of the mg_*_ep calls (episode boundaries under auto-reset); device pointers or None"""
    _fields_ = [("reset_mode", C.c_int32), ("reserved0", C.c_int32), ("ep_return", C.c_void_p), ("out_return", C.c_void_p),
                ("out_length", C.c_void_p), ("out_flags", C.c_void_p)]


EPF_TERMINATED, EPF_TRUNCATED, EPF_RESET = 1, 2, 4
RESET_SAME_STEP, RESET_NEXT_STEP = 0, 1

PLACE_MAX, PLACE_ALL = 8, 136
PLACE_STIR, PLACE_THOROUGH, PLACE_NO_REUSE = 1, 2, 4
PLACE_STOP = {0: "", 1: "found", 2: "cap", 3: "time", 4: "memory", 5: "out of memory", 6: "small", 7: "not HBM-bound"}
E_ARG, E_UNSUPPORTED, E_LAUNCH = -100, -101, -102
E_NOMEM = -103


class PlaceTuning(C.Structure):
    _fields_ = [("gain", C.c_double), ("slow_alloc_s_per_gib", C.c_double), ("min_bytes", C.c_uint64),
                ("stir_bytes", C.c_uint64), ("max_candidates", C.c_int32), ("iters", C.c_int32),
                ("share", C.c_int32), ("reserved1", C.c_int32), ("fast_rate", C.c_double)]


class PlaceStats(C.Structure):
    _fields_ = [("found", C.c_int32), ("reused", C.c_int32), ("candidates", C.c_int32), ("windows", C.c_int32),
                ("passes", C.c_int32), ("level", C.c_int32), ("plain_stage", C.c_int32), ("stopped", C.c_int32),
                ("kept_ms", C.c_float * PLACE_MAX), ("median_ms", C.c_float), ("reserved0", C.c_float),
                ("seconds", C.c_double), ("alloc_seconds", C.c_double),
                ("buffer_bytes", C.c_uint64), ("candidate_bytes", C.c_uint64), ("alloc_bytes", C.c_uint64),
                ("pinned_bytes", C.c_uint64), ("stirred_bytes", C.c_uint64), ("budget_bytes", C.c_uint64),
                ("window_offset", C.c_uint64 * PLACE_MAX), ("arena_bytes", C.c_uint64 * PLACE_MAX),
                ("all_ms", C.c_float * PLACE_ALL)]


LEVEL_PUBLISH, LEVEL_PENDING, LEVEL_MASK = 0, 1, 2      # MG_LEVEL_* (mg_level_apply's rule)
GOAL_PATH_AUTO, GOAL_PATH_REG, GOAL_PATH_LDS = 0, 1, 2  # mg_goal_distance_path's path
SOLVE_MAX_DOORS, SOLVE_MAX_ITEMS, SOLVE_LDS_LIMIT = 4, 3, 160 * 1024   # mg_solve_distance's caps and the LDS it may ask for

DELTA_FORCE = 1            # MG_DELTA_FORCE (mg_step_render_delta)

SPEC_COMPILE_ONLY = 1      # MG_SPEC_COMPILE_ONLY (mg_render_specialize)
WANT_PLAIN, WANT_ENCODE, WANT_EPISODE = 0, 1, 2


class SpecInfo(C.Structure):
    """MgSpecInfo: what mg_render_specialize says about the instantiation it compiled (or why it did not)"""
    _fields_ = [("kernel_name", C.c_char * 96), ("vs", C.c_int32), ("ts", C.c_int32), ("wpb", C.c_int32), ("v", C.c_int32),
                ("rm", C.c_int32), ("lds_bytes", C.c_int32), ("lds_static", C.c_int32), ("scratch_bytes", C.c_int32),
                ("code_bytes", C.c_int32), ("cache_hit", C.c_int32), ("table_is_ideal", C.c_int32), ("reserved0", C.c_int32),
                ("compile_seconds", C.c_double), ("reason", C.c_char * 256)]

    def as_dict(self):
        d = {f: getattr(self, f) for f, _ in self._fields_ if f != "reserved0"}
        d["kernel_name"], d["reason"] = self.kernel_name.decode(), self.reason.decode()
        return d


def delta_sig_bytes(n_agents, view_size):
    """MG_DELTA_SIG_BYTES: bytes per env of an observation buffer's signature"""
    return (n_agents * view_size * view_size * 2 + 15) // 16 * 16


LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "libmarlgrid_hip.so")

# every symbol include/marlgrid_hip.h declares
SYMBOLS = ["mg_abi_version", "mg_struct_sizes", "mg_host_flag_alloc", "mg_host_flag_free", "mg_obs_alloc", "mg_obs_free", "mg_obs_place", "mg_obs_release", "mg_obs_trim", "mg_build_info", "mg_error_string", "mg_mt_seed", "mg_reset", "mg_step", "mg_step_render", "mg_step_render_encode",
           "mg_render_obs",
           "mg_encode", "mg_put_obj", "mg_place", "mg_render_frame", "mg_time_render_obs",
           "mg_render_obs_lds_bytes", "mg_render_kernel_name", "mg_step_encode_views", "mg_encode_views",
           "mg_episode_struct_size", "mg_step_ep", "mg_step_render_ep", "mg_step_encode_views_ep",
           "mg_step_render_delta", "mg_step_render_delta_ex",
           "mg_spec_info_struct_size", "mg_render_specialize", "mg_step_render_spec", "mg_render_obs_spec",
           "mg_render_spec_release", "mg_rtc_source",
           "mg_level_seed", "mg_level_apply", "mg_level_apply_rows",
           "mg_goal_distance", "mg_goal_distance_path",
           "mg_solve_distance", "mg_solve_distance_lds_bytes",
           "mg_fork_rows", "mg_rollout",
           "mg_explore_update", "mg_memory_update"]

_lib = None
_path = LIB_PATH


def use_library(path):
    """tools/ only: bind another build of the same ABI (the measurement build libmarlgrid_hip_ab.so) instead of
    the product library — by an explicit call before the first lib(), never through the environment: the
    package loads exactly one library, the one next to it, unless a measurement script says otherwise in code."""
    global _path
    if _lib is not None:
        raise RuntimeError("marlgrid_amd: the library is already loaded (%s)" % _path)
    _path = os.path.abspath(path)


def lib():
    """Load the HIP library (after torch, so that the HIP runtime torch ships is the one bound).  Reads no
    environment variable."""
    global _lib
    if _lib is not None:
        return _lib
    import torch  # noqa: F401  — loads libamdhip64 first; our .so resolves against the same runtime
    path = _path
    if path == LIB_PATH and not os.path.exists(LIB_PATH):
        # not a fallback: build the one and only implementation if the toolchain is at hand
        import shutil
        import subprocess
        if shutil.which(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")):
            rc = subprocess.call(["bash", os.path.join(os.path.dirname(LIB_PATH), "build.sh")])
            if rc != 0:
                raise ImportError("marlgrid_amd: building %s failed (build.sh exit code %d)" % (LIB_PATH, rc))
    if not os.path.exists(path):
        raise ImportError("marlgrid_amd: %s is missing — build it (marlgrid_amd/csrc/build.sh); there is "
                          "no CPU fallback" % path)
    L = C.CDLL(path)
    vp, i32 = C.c_void_p, C.c_int32
    L.mg_abi_version.restype = i32
    if L.mg_abi_version() != ABI_VERSION:
        raise ImportError("marlgrid_amd: %s has ABI version %d, this package needs %d — rebuild it"
                          % (path, L.mg_abi_version(), ABI_VERSION))
    # the struct mirrors above against the library's own sizeof: a layout change that forgot this file (or
    # the ABI version) fails here, at load time, instead of shifting every later field of a launch config
    sizes = (i32 * 7)()
    L.mg_struct_sizes.argtypes = [C.POINTER(i32)]
    L.mg_struct_sizes.restype = i32
    if L.mg_struct_sizes(sizes) != 7:
        raise ImportError("marlgrid_amd: %s: mg_struct_sizes failed" % path)
    mine = [C.sizeof(t) for t in (Config, State, ObjDesc, GenOp, GenProgram, PlaceTuning, PlaceStats)]
    if list(sizes) != mine:
        raise ImportError("marlgrid_amd: struct layouts differ between %s %r and marlgrid_amd/_native.py %r "
                          "(MgConfig, MgState, MgObjDesc, MgGenOp, MgGenProgram, MgPlaceTuning, MgPlaceStats)" % (path, list(sizes), mine))
    L.mg_host_flag_alloc.argtypes = [C.POINTER(C.POINTER(i32)), C.POINTER(C.POINTER(i32))]
    L.mg_host_flag_free.argtypes = [C.POINTER(i32)]
    L.mg_obs_alloc.argtypes = [C.c_uint64, i32]
    L.mg_obs_alloc.restype = vp
    L.mg_obs_free.argtypes = [vp]
    L.mg_obs_place.argtypes = [C.POINTER(Config), C.POINTER(State), i32, C.c_uint64, C.c_double, i32, C.POINTER(PlaceTuning),
                               C.POINTER(vp), C.POINTER(PlaceStats), vp]
    L.mg_obs_release.argtypes = [vp]
    L.mg_obs_trim.argtypes = [i32]
    L.mg_error_string.restype = C.c_char_p
    L.mg_error_string.argtypes = [i32]
    L.mg_build_info.restype = C.c_char_p
    L.mg_mt_seed.argtypes = [i32, vp, vp, vp, vp, vp, vp]
    # (n, seeds, slots, row_mask, n_slots, bank_mt, bank_pos, bank_head, bank_seed, stream)
    L.mg_level_seed.argtypes = [i32, vp, vp, vp, i32, vp, vp, vp, vp, vp]
    # (cfg, st, rule, env_mask, level_of_env, n_slots, bank_mt, bank_pos, bank_head, bank_seed, episode_level, out_level, stream)
    L.mg_level_apply.argtypes = [C.POINTER(Config), C.POINTER(State), i32, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp]
    # (... out_level, bank_params, bank_edits, K, env_params, env_edits, stream)
    L.mg_level_apply_rows.argtypes = [C.POINTER(Config), C.POINTER(State), i32, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp]
    # (cfg, st, env_mask, agent_dist, field, stream) / (..., field, path, stream)
    L.mg_goal_distance.argtypes = [C.POINTER(Config), C.POINTER(State), vp, vp, vp, vp]
    L.mg_goal_distance_path.argtypes = [C.POINTER(Config), C.POINTER(State), vp, vp, vp, i32, vp]
    # (cfg, st, env_mask, max_doors, max_items, agent_dist, agent_action, env_exact, stream) / (W, H, max_doors, max_items)
    L.mg_solve_distance.argtypes = [C.POINTER(Config), C.POINTER(State), vp, i32, i32, vp, vp, vp, vp]
    L.mg_solve_distance_lds_bytes.argtypes = [i32, i32, i32, i32]
    # (cfg, src, dst, src_of_dst, dst_of_row, dst_B, R, m, stream) / (cfg, st, actions, action_bytes, T, m, rewards, done, errors, stream)
    L.mg_fork_rows.argtypes = [C.POINTER(Config), C.POINTER(State), C.POINTER(State), vp, vp, i32, i32, i32, vp]
    L.mg_rollout.argtypes = [C.POINTER(Config), C.POINTER(State), vp, i32, i32, i32, vp, vp, vp, vp]
    # (cfg, st, env_mask, seen, visits, new_cells, visit_count, stream)
    L.mg_explore_update.argtypes = [C.POINTER(Config), C.POINTER(State), vp, vp, vp, vp, vp, vp]
    # (cfg, st, env_mask, seen, visits, new_cells, visit_count, memory, seen_step, stream)
    L.mg_memory_update.argtypes = [C.POINTER(Config), C.POINTER(State), vp, vp, vp, vp, vp, vp, vp, vp]
    L.mg_reset.argtypes = [C.POINTER(Config), C.POINTER(State), C.POINTER(GenProgram), vp, vp]
    L.mg_step.argtypes = [C.POINTER(Config), C.POINTER(State), vp, i32, vp, C.POINTER(GenProgram), vp]
    L.mg_step_render.argtypes = [C.POINTER(Config), C.POINTER(State), vp, i32, vp, C.POINTER(GenProgram), vp, vp]
    L.mg_step_render_encode.argtypes = [C.POINTER(Config), C.POINTER(State), vp, i32, vp, C.POINTER(GenProgram), vp, vp, vp]
    # (cfg, st, actions, action_bytes, rewards, auto_reset, obs, signature, flags, stream)
    L.mg_step_render_delta.argtypes = [C.POINTER(Config), C.POINTER(State), vp, i32, vp, C.POINTER(GenProgram), vp, vp, C.c_uint32, vp]
    # (cfg, st, actions, action_bytes, rewards, auto_reset, obs, signature, flags, encode_out, ep, stream)
    L.mg_step_render_delta_ex.argtypes = [C.POINTER(Config), C.POINTER(State), vp, i32, vp, C.POINTER(GenProgram), vp, vp, C.c_uint32,
                                          vp, C.POINTER(Episode), vp]
    L.mg_step_encode_views.argtypes = [C.POINTER(Config), C.POINTER(State), vp, i32, vp, C.POINTER(GenProgram), vp, vp]
    L.mg_encode_views.argtypes = [C.POINTER(Config), C.POINTER(State), vp, vp]
    L.mg_episode_struct_size.argtypes = []
    L.mg_episode_struct_size.restype = i32
    if L.mg_episode_struct_size() != C.sizeof(Episode):
        raise ImportError("marlgrid_amd: MgEpisode is %d bytes in %s, %d in marlgrid_amd/_native.py"
                          % (L.mg_episode_struct_size(), path, C.sizeof(Episode)))
    L.mg_step_ep.argtypes = [C.POINTER(Config), C.POINTER(State), vp, i32, vp, C.POINTER(GenProgram), C.POINTER(Episode), vp]
    L.mg_step_render_ep.argtypes = [C.POINTER(Config), C.POINTER(State), vp, i32, vp, C.POINTER(GenProgram), vp,
                                    C.POINTER(Episode), vp]
    L.mg_step_encode_views_ep.argtypes = [C.POINTER(Config), C.POINTER(State), vp, i32, vp, C.POINTER(GenProgram), vp,
                                          C.POINTER(Episode), vp]
    L.mg_render_obs.argtypes = [C.POINTER(Config), C.POINTER(State), vp, vp, vp, vp, vp]
    L.mg_spec_info_struct_size.argtypes = []
    L.mg_spec_info_struct_size.restype = i32
    if L.mg_spec_info_struct_size() != C.sizeof(SpecInfo):
        raise ImportError("marlgrid_amd: MgSpecInfo is %d bytes in %s, %d in marlgrid_amd/_native.py"
                          % (L.mg_spec_info_struct_size(), path, C.sizeof(SpecInfo)))
    # (cfg, want, flags, arch, cache_dir, &handle, &info)
    L.mg_render_specialize.argtypes = [C.POINTER(Config), i32, C.c_uint32, C.c_char_p, C.c_char_p, C.POINTER(vp), C.POINTER(SpecInfo)]
    # (handle, cfg, st, actions, action_bytes, rewards, auto_reset, obs, encode_out, ep, stream)
    L.mg_step_render_spec.argtypes = [vp, C.POINTER(Config), C.POINTER(State), vp, i32, vp, C.POINTER(GenProgram), vp, vp,
                                      C.POINTER(Episode), vp]
    L.mg_render_obs_spec.argtypes = [vp, C.POINTER(Config), C.POINTER(State), vp, vp]
    L.mg_render_spec_release.argtypes = [vp]
    L.mg_rtc_source.argtypes = [i32, C.POINTER(C.c_char_p), C.POINTER(vp), C.POINTER(i32)]
    L.mg_encode.argtypes = [C.POINTER(Config), C.POINTER(State), vp, vp, vp]
    L.mg_put_obj.argtypes = [C.POINTER(Config), C.POINTER(State), i32, i32, i32, vp, vp]
    L.mg_place.argtypes = [C.POINTER(Config), C.POINTER(State), i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp]
    L.mg_render_frame.argtypes = [C.POINTER(Config), C.POINTER(State), vp, i32, vp, i32, i32, C.c_uint32, vp, vp]
    L.mg_render_kernel_name.argtypes = [C.POINTER(Config), C.c_char_p, i32]
    L.mg_time_render_obs.argtypes = [C.POINTER(Config), C.POINTER(State), vp, i32, C.POINTER(C.c_float), vp]
    for f in SYMBOLS:
        getattr(L, f)
        if f not in ("mg_error_string", "mg_build_info", "mg_obs_alloc"):
            getattr(L, f).restype = i32
    _lib = L
    return L


def check(rc):
    if rc != 0:
        raise RuntimeError("libmarlgrid_hip: %s (%d)" % (lib().mg_error_string(rc).decode(), rc))


def render_kernel_name(cfg):
    """(name, generic bits) of the observation-kernel instantiation the launcher picks for `cfg` (mg_render_kernel_name)"""
    buf = C.create_string_buffer(96)
    rc = lib().mg_render_kernel_name(C.byref(cfg), buf, len(buf))
    if rc < 0:
        check(rc)
    return buf.value.decode(), rc
