// mg_api.hip — the C ABI of libmarlgrid_hip.so (include/marlgrid_hip.h): argument checks and
// launches only; every buffer is caller-owned device memory, every call is asynchronous on the
// caller's stream.
#include <stdio.h>

#include "mg_device.h"
#include "mg_launch.h"
#include "mg_solve_core.h"

namespace {

int check_cfg(const MgConfig* c) {
    if (!c) return MG_E_ARG;
    if (c->B < 0 || c->W < 3 || c->H < 3 || c->W > 255 || c->H > 255) return MG_E_ARG;
    if (c->n_agents < 1 || c->n_agents > MG_MAX_AGENTS) return MG_E_UNSUPPORTED;
    if (c->view_size < 1 || c->view_size > MG_MAX_VIEW) return MG_E_UNSUPPORTED;   // (even sizes included: agents.py:233-266 is written with view_size // 2)
    if (c->tile_size < 1 || c->tile_size > 64) return MG_E_UNSUPPORTED;
    if (c->view_offset < 0 || c->view_offset >= c->view_size) return MG_E_ARG;
    if (c->cells_stride < c->W * c->H || (c->cells_stride & 15)) return MG_E_ARG;
    if (c->n_obj < 1 || c->n_obj > MG_MAX_OBJ) return MG_E_UNSUPPORTED;
    if (c->n_tiles < 1 + c->n_obj + c->n_ovl_slots * c->n_agents * 4) return MG_E_ARG;
    if (c->prestige_mask && (c->prestige_sprite_tile < 0 || c->prestige_sprite_tile + 4 > c->n_tiles)) return MG_E_ARG;
    if (!c->obj || !c->atlas) return MG_E_ARG;
    if (c->max_steps < 1) return MG_E_ARG;
    // the viewer subset of a launch (agents that differ in view geometry are rendered group by group)
    if (c->n_view < 0 || c->n_view > c->n_agents) return MG_E_ARG;
    for (int i = 0; i < c->n_view; i++)
        if (c->view_agent[i] >= c->n_agents) return MG_E_ARG;
    if (c->spawn_x0 < 0 || c->spawn_y0 < 0 || c->spawn_x1 > c->W || c->spawn_y1 > c->H || c->spawn_x1 <= c->spawn_x0 ||
        c->spawn_y1 <= c->spawn_y0 || c->spawn_max_tries < 1 || c->spawn_max_tries > 100000)
        return MG_E_ARG;
    return MG_OK;
}

int check_prog(const MgConfig* cfg, const MgGenProgram* prog) {
    // (the ops themselves are device memory — MgGenProgram::ops —: what they must satisfy is the caller's to guarantee)
    (void)cfg;
    if (!prog || !prog->template_grid || prog->n_ops < 0 || prog->n_ops > MG_MAX_GEN) return MG_E_ARG;
    if (prog->n_ops > 0 && !prog->ops) return MG_E_ARG;
    if (prog->n_reject < 0 || (prog->n_reject > 0 && !prog->reject)) return MG_E_ARG;
    return MG_OK;
}

int check_state(const MgState* s) {
    if (!s || !s->grid || !s->agents || !s->mt || !s->mt_pos || !s->mt_head || !s->step_count || !s->done || !s->error)
        return MG_E_ARG;
    return MG_OK;
}

int check_both(const MgConfig* c, const MgState* s) {
    int e = check_cfg(c);
    if (e) return e;
    e = check_state(s);
    if (e) return e;
    if (c->prestige_mask && !s->prestige) return MG_E_ARG;
    return MG_OK;
}

int rc(hipError_t e) { return e == hipSuccess ? MG_OK : MG_E_LAUNCH; }

// MgEpisode (mg_*_ep): what can be said without looking into device memory
int check_episode(const MgEpisode* ep, const MgGenProgram* auto_reset) {
    if (!ep) return MG_OK;
    if (ep->reset_mode != 0 && ep->reset_mode != 1) return MG_E_ARG;
    if (ep->reset_mode == 1 && !auto_reset) return MG_E_ARG;     // next-step reset resets: it needs the program
    if (ep->out_return && !ep->ep_return) return MG_E_ARG;
    return MG_OK;
}

// what every step entry point checks, in the order a caller can observe: the episode block first (answered without a valid
// config or a device), the config and the state, the buffers, the reset program.  `single_group`: the call steps AND writes
// every agent's observation in one launch — view groups (n_view != 0) take mg_step + one launch per group instead.
int check_step_args(const MgConfig* cfg, const MgState* st, const void* actions, int32_t action_bytes, const float* rewards,
                    const MgGenProgram* auto_reset, const MgEpisode* ep, bool single_group) {
    int e = check_episode(ep, auto_reset);
    if (e) return e;
    e = check_both(cfg, st);
    if (e) return e;
    if (!actions || !rewards) return MG_E_ARG;
    if (action_bytes != 1 && action_bytes != 4 && action_bytes != 8) return MG_E_ARG;
    if (single_group && cfg->n_view != 0) return MG_E_ARG;
    return auto_reset ? check_prog(cfg, auto_reset) : MG_OK;
}

}  // namespace

extern "C" {

int32_t mg_abi_version(void) { return MG_ABI_VERSION; }

int32_t mg_struct_sizes(int32_t out[7]) {
    if (!out) return MG_E_ARG;
    out[0] = (int32_t)sizeof(MgConfig);
    out[1] = (int32_t)sizeof(MgState);
    out[2] = (int32_t)sizeof(MgObjDesc);
    out[3] = (int32_t)sizeof(MgGenOp);
    out[4] = (int32_t)sizeof(MgGenProgram);
    out[5] = (int32_t)sizeof(MgPlaceTuning);
    out[6] = (int32_t)sizeof(MgPlaceStats);
    return 7;
}

#define MG_STR2(x) #x
#define MG_STR(x) MG_STR2(x)
#ifndef MG_BUILD_ID
#define MG_BUILD_ID "unknown"
#endif
const char* mg_build_info(void) {
#if defined(MG_AB_VARIANTS)
    return "libmarlgrid_hip_ab gfx950 abi" MG_STR(MG_ABI_VERSION) " " MG_BUILD_ID " (measurement variants: tools/ only)";
#else
    return "libmarlgrid_hip gfx950 abi" MG_STR(MG_ABI_VERSION) " " MG_BUILD_ID;
#endif
}

const char* mg_error_string(int32_t code) {
    switch (code) {
    case MG_OK: return "ok";
    case MG_E_ARG: return "invalid argument";
    case MG_E_UNSUPPORTED: return "unsupported configuration";
    case MG_E_LAUNCH: return "HIP launch failed";
    case MG_E_NOMEM: return "out of device memory";
    case MG_ERR_VALUE: return "ValueError: environment can't handle action";
    case MG_ERR_RECURSION: return "RecursionError: rejection sampling failed in place_obj";
    case MG_ERR_TYPE: return "TypeError: toggle() arity (Box)";
    case MG_ERR_ASSERT: return "AssertionError: grid access out of bounds";
    case MG_ERR_ATTRIBUTE: return "AttributeError: the cell under an agent was emptied by put_obj(None)";
    default: return "unknown";
    }
}

int32_t mg_mt_seed(int32_t B, const uint32_t* keys, const int32_t* key_len, uint32_t* mt, int32_t* mt_pos,
                   uint32_t* mt_head, void* stream) {
    if (B < 0 || !keys || !key_len || !mt || !mt_pos || !mt_head) return MG_E_ARG;
    return rc(mg::launch_mt_seed(B, keys, key_len, mt, mt_pos, mt_head, (hipStream_t)stream));
}

int32_t mg_reset(const MgConfig* cfg, const MgState* st, const MgGenProgram* prog, const uint8_t* env_mask,
                 void* stream) {
    int e = check_both(cfg, st);
    if (e) return e;
    e = check_prog(cfg, prog);
    if (e) return e;
    return rc(mg::launch_reset(*cfg, *st, *prog, env_mask, (hipStream_t)stream));
}

int32_t mg_level_seed(int32_t n, const int64_t* seeds, const int64_t* slots, const uint8_t* row_mask, int32_t n_slots,
                      uint32_t* bank_mt, int32_t* bank_pos, uint32_t* bank_head, int64_t* bank_seed, void* stream) {
    if (n < 0 || n_slots < 0 || !seeds || !bank_mt || !bank_pos || !bank_head || !bank_seed) return MG_E_ARG;
    return rc(mg::launch_level_seed(n, seeds, slots, row_mask, n_slots, bank_mt, bank_pos, bank_head, bank_seed, (hipStream_t)stream));
}

int32_t mg_level_apply(const MgConfig* cfg, const MgState* st, int32_t rule, const uint8_t* env_mask, const int64_t* level_of_env,
                       int32_t n_slots, const uint32_t* bank_mt, const int32_t* bank_pos, const uint32_t* bank_head,
                       const int64_t* bank_seed, int64_t* episode_level, int64_t* out_level, void* stream) {
    if (!cfg || cfg->B < 0 || cfg->n_agents < 1 || cfg->n_agents > MG_MAX_AGENTS) return MG_E_ARG;
    const int e = check_state(st);
    if (e) return e;
    if (rule != MG_LEVEL_PUBLISH && rule != MG_LEVEL_PENDING && rule != MG_LEVEL_MASK) return MG_E_ARG;
    if (n_slots < 0 || !episode_level) return MG_E_ARG;
    if (rule != MG_LEVEL_PUBLISH && (!level_of_env || (n_slots > 0 && (!bank_mt || !bank_pos || !bank_head || !bank_seed)))) return MG_E_ARG;
    // (the copy is 16-byte traffic: generator rows are 2 496 and 64 bytes, so aligned bases keep every row aligned)
    if ((reinterpret_cast<uintptr_t>(bank_mt) | reinterpret_cast<uintptr_t>(bank_head) | reinterpret_cast<uintptr_t>(st->mt) |
         reinterpret_cast<uintptr_t>(st->mt_head)) & 15)
        return MG_E_ARG;
    return rc(mg::launch_level_apply(*cfg, *st, rule, env_mask, level_of_env, n_slots, bank_mt, bank_pos, bank_head, bank_seed,
                                     episode_level, out_level, (hipStream_t)stream));
}

int32_t mg_level_apply_rows(const MgConfig* cfg, const MgState* st, int32_t rule, const uint8_t* env_mask, const int64_t* level_of_env,
                            int32_t n_slots, const uint32_t* bank_mt, const int32_t* bank_pos, const uint32_t* bank_head,
                            const int64_t* bank_seed, int64_t* episode_level, int64_t* out_level, const uint8_t* bank_params,
                            const uint8_t* bank_edits, int32_t K, uint8_t* env_params, uint8_t* env_edits, void* stream) {
    if (!cfg || cfg->B < 0 || cfg->n_agents < 1 || cfg->n_agents > MG_MAX_AGENTS) return MG_E_ARG;
    const int e = check_state(st);
    if (e) return e;
    if (rule != MG_LEVEL_PUBLISH && rule != MG_LEVEL_PENDING && rule != MG_LEVEL_MASK) return MG_E_ARG;
    if (n_slots < 0 || !episode_level) return MG_E_ARG;
    if (rule != MG_LEVEL_PUBLISH && (!level_of_env || (n_slots > 0 && (!bank_mt || !bank_pos || !bank_head || !bank_seed)))) return MG_E_ARG;
    if ((reinterpret_cast<uintptr_t>(bank_mt) | reinterpret_cast<uintptr_t>(bank_head) | reinterpret_cast<uintptr_t>(st->mt) |
         reinterpret_cast<uintptr_t>(st->mt_head)) & 15)
        return MG_E_ARG;
    // the rows: a pair comes whole or not at all; an edit pair with 1 <= K <= MG_GEN_MAX_EDITS; 32-bit traffic
    if (!bank_params != !env_params || !bank_edits != !env_edits) return MG_E_ARG;
    if (bank_edits ? (K < 1 || K > MG_GEN_MAX_EDITS) : K != 0) return MG_E_ARG;
    if ((reinterpret_cast<uintptr_t>(bank_params) | reinterpret_cast<uintptr_t>(env_params) | reinterpret_cast<uintptr_t>(bank_edits) |
         reinterpret_cast<uintptr_t>(env_edits)) & 3)
        return MG_E_ARG;
    return rc(mg::launch_level_apply_rows(*cfg, *st, rule, env_mask, level_of_env, n_slots, bank_mt, bank_pos, bank_head, bank_seed,
                                          episode_level, out_level, bank_params, bank_edits, K, env_params, env_edits,
                                          (hipStream_t)stream));
}

int32_t mg_goal_distance_path(const MgConfig* cfg, const MgState* st, const uint8_t* env_mask, int32_t* agent_dist, int32_t* field,
                              int32_t path, void* stream) {
    if (!cfg || !st || !agent_dist || !st->grid || !st->agents || !cfg->obj) return MG_E_ARG;
    if (cfg->B < 0 || cfg->W < 1 || cfg->H < 1 || cfg->W > 255 || cfg->H > 255 || cfg->n_agents < 1 || cfg->n_agents > MG_MAX_AGENTS)
        return MG_E_ARG;
    if (cfg->cells_stride < cfg->W * cfg->H || cfg->n_obj < 1 || cfg->n_obj > MG_MAX_OBJ) return MG_E_ARG;
    if (path < 0 || path > 2) return MG_E_ARG;
    int unsupported = 0;
    const hipError_t e = mg::launch_goal_distance(*cfg, *st, env_mask, agent_dist, field, path, (hipStream_t)stream, &unsupported);
    return unsupported ? MG_E_UNSUPPORTED : rc(e);
}

int32_t mg_goal_distance(const MgConfig* cfg, const MgState* st, const uint8_t* env_mask, int32_t* agent_dist, int32_t* field,
                         void* stream) {
    return mg_goal_distance_path(cfg, st, env_mask, agent_dist, field, 0, stream);
}

int32_t mg_solve_distance(const MgConfig* cfg, const MgState* st, const uint8_t* env_mask, int32_t max_doors, int32_t max_items,
                          int32_t* agent_dist, int8_t* agent_action, uint8_t* env_exact, void* stream) {
    if (!cfg || !st || !agent_dist || !st->grid || !st->agents || !cfg->obj) return MG_E_ARG;
    if (cfg->B < 0 || cfg->W < 1 || cfg->H < 1 || cfg->W > 255 || cfg->H > 255 || cfg->n_agents < 1 || cfg->n_agents > MG_MAX_AGENTS)
        return MG_E_ARG;
    if (cfg->cells_stride < cfg->W * cfg->H || cfg->n_obj < 1 || cfg->n_obj > MG_MAX_OBJ) return MG_E_ARG;
    if (max_doors < 0 || max_doors > 4 || max_items < 0 || max_items > 3) return MG_E_ARG;
    int unsupported = 0;
    const hipError_t e = mg::launch_solve_distance(*cfg, *st, env_mask, max_doors, max_items, agent_dist, agent_action, env_exact,
                                                   (hipStream_t)stream, &unsupported);
    return unsupported ? MG_E_UNSUPPORTED : rc(e);
}

int32_t mg_solve_distance_lds_bytes(int32_t W, int32_t H, int32_t max_doors, int32_t max_items) {
    if (W < 1 || H < 1 || W > 255 || H > 255 || max_doors < 0 || max_doors > 4 || max_items < 0 || max_items > 3) return MG_E_ARG;
    return (int32_t)mg::solve_scratch_bytes(W, H, max_doors, max_items);
}

int32_t mg_fork_rows(const MgConfig* cfg, const MgState* src, const MgState* dst, const int64_t* src_of_dst, const int64_t* dst_of_row,
                     int32_t dst_B, int32_t R, int32_t m, void* stream) {
    if (!cfg || cfg->B < 0 || cfg->n_agents < 1 || cfg->n_agents > MG_MAX_AGENTS || cfg->cells_stride < 1) return MG_E_ARG;
    int e = check_state(src);
    if (e) return e;
    e = check_state(dst);
    if (e) return e;
    if (cfg->prestige_mask && (!src->prestige || !dst->prestige)) return MG_E_ARG;
    if (R < 0 || dst_B < 0 || m < 1 || R % m != 0) return MG_E_ARG;
    // (generator rows are 2 496 and 64 bytes, copied as 16-byte vectors: aligned bases keep every row aligned)
    if ((reinterpret_cast<uintptr_t>(src->mt) | reinterpret_cast<uintptr_t>(src->mt_head) | reinterpret_cast<uintptr_t>(dst->mt) |
         reinterpret_cast<uintptr_t>(dst->mt_head)) & 15)
        return MG_E_ARG;
    return rc(mg::launch_fork_rows(*cfg, *src, *dst, src_of_dst, dst_of_row, dst_B, R, m, (hipStream_t)stream));
}

int32_t mg_rollout(const MgConfig* cfg, const MgState* st, const void* actions, int32_t action_bytes, int32_t T, int32_t m,
                   float* rewards, uint8_t* done, int32_t* errors, void* stream) {
    const int e = check_step_args(cfg, st, actions, action_bytes, rewards, nullptr, nullptr, false);
    if (e) return e;
    if (!done || T < 0 || m < 1 || cfg->B % m != 0) return MG_E_ARG;
    return rc(mg::launch_rollout(*cfg, *st, actions, action_bytes, T, m, rewards, done, errors, (hipStream_t)stream));
}

int32_t mg_explore_update(const MgConfig* cfg, const MgState* st, const uint8_t* env_mask, uint8_t* seen, int32_t* visits,
                          int32_t* new_cells, int32_t* visit_count, void* stream) {
    const int e = check_both(cfg, st);
    if (e) return e;
    if (!seen || !visits || !new_cells || !visit_count) return MG_E_ARG;
    return rc(mg::launch_explore_update(*cfg, *st, env_mask, seen, visits, new_cells, visit_count, (hipStream_t)stream));
}

int32_t mg_memory_update(const MgConfig* cfg, const MgState* st, const uint8_t* env_mask, uint8_t* seen, int32_t* visits,
                         int32_t* new_cells, int32_t* visit_count, uint8_t* memory, int32_t* seen_step, void* stream) {
    const int e = check_both(cfg, st);
    if (e) return e;
    if (!seen || !visits || !new_cells || !visit_count || !memory || !seen_step) return MG_E_ARG;
    return rc(mg::launch_memory_update(*cfg, *st, env_mask, seen, visits, new_cells, visit_count, memory, seen_step,
                                       (hipStream_t)stream));
}

int32_t mg_episode_struct_size(void) { return (int32_t)sizeof(MgEpisode); }

int32_t mg_step_ep(const MgConfig* cfg, const MgState* st, const void* actions, int32_t action_bytes, float* rewards,
                   const MgGenProgram* auto_reset, const MgEpisode* ep, void* stream) {
    const int e = check_step_args(cfg, st, actions, action_bytes, rewards, auto_reset, ep, false);
    if (e) return e;
    return rc(mg::launch_step(*cfg, *st, actions, action_bytes, rewards, auto_reset, (hipStream_t)stream, ep));
}

int32_t mg_step(const MgConfig* cfg, const MgState* st, const void* actions, int32_t action_bytes, float* rewards,
                const MgGenProgram* auto_reset, void* stream) {
    return mg_step_ep(cfg, st, actions, action_bytes, rewards, auto_reset, nullptr, stream);
}

int32_t mg_render_obs(const MgConfig* cfg, const MgState* st, uint8_t* obs, uint8_t* view_cells,
                      uint8_t* view_agent, uint8_t* vis_mask, void* stream) {
    int e = check_both(cfg, st);
    if (e) return e;
    if (!obs) return MG_E_ARG;
    return rc(mg::launch_render(*cfg, *st, obs, view_cells, view_agent, vis_mask, (hipStream_t)stream));
}

// what the obs kernel's fused step is told (the table's launcher and a specialised handle's alike)
static mg::FusedStep fused_step_of(const MgConfig* cfg, const void* actions, int32_t action_bytes, float* rewards,
                                   const MgGenProgram* auto_reset, uint8_t* encode_out, const MgEpisode* ep, uint16_t* sig,
                                   uint32_t sig_flags) {
    mg::FusedStep fs{};
    fs.actions = actions;
    fs.rewards = rewards;
    fs.action_bytes = action_bytes;
    fs.enabled = 1;
    fs.has_prog = auto_reset ? 1 : 0;
    if (auto_reset) fs.prog = *auto_reset;
    fs.encode_out = encode_out;
    const uint32_t cells = (uint32_t)(cfg->W * cfg->H), n = (uint32_t)cfg->n_agents;
    fs.enc_m_cells = (uint32_t)((0x100000000ull + cells - 1) / cells);
    fs.enc_m_n = (uint32_t)((0x100000000ull + n - 1) / n);
    fs.has_ep = ep ? 1 : 0;
    if (ep) fs.ep = *ep;
    fs.sig = sig;
    fs.sig_flags = ((sig_flags & MG_DELTA_FORCE) ? mg::kSigForce : 0) |
                   (mg::delta_sig_compact(cfg->n_tiles, cfg->n_agents, cfg->view_size) ? 0 : mg::kSigWide);
    return fs;
}

static int32_t step_render(const MgConfig* cfg, const MgState* st, const void* actions, int32_t action_bytes, float* rewards,
                           const MgGenProgram* auto_reset, uint8_t* obs, uint8_t* encode_out, void* stream,
                           const MgEpisode* ep = nullptr, uint16_t* sig = nullptr, uint32_t sig_flags = 0) {
    const int e = check_step_args(cfg, st, actions, action_bytes, rewards, auto_reset, ep, true);
    if (e) return e;
    if (!obs) return MG_E_ARG;      // (every check between the state's and this one answers MG_E_ARG too)
    // the one pick of the step: the launcher takes it as it is.  (A config without even a plain instantiation is the launcher's
    // to refuse, as for mg_render_obs.)
    const mg::RenderWant want = mg::render_want_of(sig != nullptr, encode_out != nullptr, ep != nullptr);
    mg::RenderPick pick;
    const bool picked = mg::render_pick(*cfg, want, &pick);
    if (!picked && want != mg::kPlain) return MG_E_UNSUPPORTED;
    const mg::FusedStep fs = fused_step_of(cfg, actions, action_bytes, rewards, auto_reset, encode_out, ep, sig, sig_flags);
    return rc(mg::launch_render(*cfg, *st, obs, nullptr, nullptr, nullptr, (hipStream_t)stream, &fs, picked ? &pick : nullptr));
}

// ... and through an instantiation compiled at run time (mg_rtc.hip: mg_render_specialize)
int32_t mg_step_render_spec(void* handle, const MgConfig* cfg, const MgState* st, const void* actions, int32_t action_bytes,
                            float* rewards, const MgGenProgram* auto_reset, uint8_t* obs, uint8_t* encode_out,
                            const MgEpisode* ep, void* stream) {
    if (!handle || (encode_out && ep)) return MG_E_ARG;
    const int e = check_step_args(cfg, st, actions, action_bytes, rewards, auto_reset, ep, true);
    if (e) return e;
    if (!obs) return MG_E_ARG;
    const mg::FusedStep fs = fused_step_of(cfg, actions, action_bytes, rewards, auto_reset, encode_out, ep, nullptr, 0);
    return mg::launch_render_spec(handle, *cfg, *st, obs, (hipStream_t)stream, &fs);
}

int32_t mg_render_obs_spec(void* handle, const MgConfig* cfg, const MgState* st, uint8_t* obs, void* stream) {
    if (!handle) return MG_E_ARG;
    const int e = check_both(cfg, st);
    if (e) return e;
    if (!obs) return MG_E_ARG;
    return mg::launch_render_spec(handle, *cfg, *st, obs, (hipStream_t)stream, nullptr);
}

int32_t mg_step_render(const MgConfig* cfg, const MgState* st, const void* actions, int32_t action_bytes, float* rewards,
                       const MgGenProgram* auto_reset, uint8_t* obs, void* stream) {
    return step_render(cfg, st, actions, action_bytes, rewards, auto_reset, obs, nullptr, stream);
}

int32_t mg_step_render_ep(const MgConfig* cfg, const MgState* st, const void* actions, int32_t action_bytes, float* rewards,
                          const MgGenProgram* auto_reset, uint8_t* obs, const MgEpisode* ep, void* stream) {
    return step_render(cfg, st, actions, action_bytes, rewards, auto_reset, obs, nullptr, stream, ep);
}

int32_t mg_step_render_encode(const MgConfig* cfg, const MgState* st, const void* actions, int32_t action_bytes, float* rewards,
                              const MgGenProgram* auto_reset, uint8_t* obs, uint8_t* encode_out, void* stream) {
    if (!encode_out) return MG_E_ARG;
    return step_render(cfg, st, actions, action_bytes, rewards, auto_reset, obs, encode_out, stream);
}

int32_t mg_step_render_delta(const MgConfig* cfg, const MgState* st, const void* actions, int32_t action_bytes, float* rewards,
                             const MgGenProgram* auto_reset, uint8_t* obs, uint16_t* signature, uint32_t flags, void* stream) {
    if (!signature || (flags & ~(uint32_t)MG_DELTA_FORCE) || (reinterpret_cast<uintptr_t>(signature) & 15)) return MG_E_ARG;
    return step_render(cfg, st, actions, action_bytes, rewards, auto_reset, obs, nullptr, stream, nullptr, signature, flags);
}

int32_t mg_step_render_delta_ex(const MgConfig* cfg, const MgState* st, const void* actions, int32_t action_bytes, float* rewards,
                                const MgGenProgram* auto_reset, uint8_t* obs, uint16_t* signature, uint32_t flags,
                                uint8_t* encode_out, const MgEpisode* ep, void* stream) {
    if (!signature || (flags & ~(uint32_t)MG_DELTA_FORCE) || (reinterpret_cast<uintptr_t>(signature) & 15)) return MG_E_ARG;
    if (!encode_out && !ep) return MG_E_ARG;      // (the plain call keeps its one spelling: mg_step_render_delta)
    return step_render(cfg, st, actions, action_bytes, rewards, auto_reset, obs, encode_out, stream, ep, signature, flags);
}

int32_t mg_encode(const MgConfig* cfg, const MgState* st, const uint8_t* vis_mask, uint8_t* out, void* stream) {
    int e = check_cfg(cfg);
    if (e) return e;
    e = check_state(st);
    if (e) return e;
    if (!out) return MG_E_ARG;
    return rc(mg::launch_encode(*cfg, *st, vis_mask, out, (hipStream_t)stream));
}

int32_t mg_encode_views(const MgConfig* cfg, const MgState* st, uint8_t* views, void* stream) {
    int e = check_both(cfg, st);
    if (e) return e;
    if (!views) return MG_E_ARG;
    return rc(mg::launch_encode_views(*cfg, *st, views, (hipStream_t)stream));
}

int32_t mg_step_encode_views_ep(const MgConfig* cfg, const MgState* st, const void* actions, int32_t action_bytes,
                                float* rewards, const MgGenProgram* auto_reset, uint8_t* views, const MgEpisode* ep,
                                void* stream) {
    const int e = check_step_args(cfg, st, actions, action_bytes, rewards, auto_reset, ep, true);
    if (e) return e;
    if (!views) return MG_E_ARG;
    return rc(mg::launch_step_encode_views(*cfg, *st, actions, action_bytes, rewards, auto_reset, views, (hipStream_t)stream, ep));
}

int32_t mg_step_encode_views(const MgConfig* cfg, const MgState* st, const void* actions, int32_t action_bytes, float* rewards,
                             const MgGenProgram* auto_reset, uint8_t* views, void* stream) {
    return mg_step_encode_views_ep(cfg, st, actions, action_bytes, rewards, auto_reset, views, nullptr, stream);
}

int32_t mg_put_obj(const MgConfig* cfg, const MgState* st, int32_t obj, int32_t x, int32_t y,
                   const uint8_t* env_mask, void* stream) {
    int e = check_cfg(cfg);
    if (e) return e;
    e = check_state(st);
    if (e) return e;
    if (obj < 0 || obj >= cfg->n_obj || x < 0 || x >= cfg->W || y < 0 || y >= cfg->H) return MG_E_ARG;
    return rc(mg::launch_put_obj(*cfg, *st, obj, x, y, env_mask, (hipStream_t)stream));
}

int32_t mg_place(const MgConfig* cfg, const MgState* st, int32_t what, int32_t x0, int32_t y0, int32_t x1, int32_t y1,
                 int32_t max_tries, const int32_t* fixed_pos, const uint8_t* env_mask, const uint8_t* reject,
                 int32_t* out_pos, uint8_t* out_ok, void* stream) {
    int e = check_cfg(cfg);
    if (e) return e;
    e = check_state(st);
    if (e) return e;
    if (what == 0 || what >= cfg->n_obj || -(what + 1) >= cfg->n_agents) return MG_E_ARG;
    if (!fixed_pos && (x0 < 0 || y0 < 0 || x1 > cfg->W || y1 > cfg->H || x1 <= x0 || y1 <= y0 || max_tries < 1))
        return MG_E_ARG;
    return rc(mg::launch_place(*cfg, *st, what, x0, y0, x1, y1, max_tries, fixed_pos, env_mask, reject, out_pos, out_ok,
                               (hipStream_t)stream));
}

int32_t mg_render_frame(const MgConfig* cfg, const MgState* st, const int32_t* env_ids, int32_t n_envs,
                        const uint8_t* frame_atlas, int32_t frame_tile_size, int32_t highlight, uint32_t frame_amax,
                        uint8_t* out, void* stream) {
    int e = check_cfg(cfg);
    if (e) return e;
    e = check_state(st);
    if (e) return e;
    if (!env_ids || n_envs < 0 || !frame_atlas || !out) return MG_E_ARG;
    if (frame_tile_size < 4 || frame_tile_size > 64 || (frame_tile_size & 3)) return MG_E_UNSUPPORTED;
    if (cfg->prestige_mask && !st->prestige) return MG_E_ARG;
    return rc(mg::launch_frame(*cfg, *st, env_ids, n_envs, frame_atlas, frame_tile_size, highlight, frame_amax, out,
                               (hipStream_t)stream));
}

int32_t mg_render_obs_lds_bytes(const MgConfig* cfg) {
    if (!cfg || cfg->n_agents < 1 || cfg->n_agents > MG_MAX_AGENTS || cfg->view_size < 1 || cfg->view_size > MG_MAX_VIEW ||
        cfg->tile_size < 1 || cfg->tile_size > 64 || cfg->cells_stride < 0 || cfg->n_tiles < 0)
        return MG_E_ARG;
    return mg::render_min_lds_bytes(*cfg);
}

int32_t mg_render_kernel_name(const MgConfig* cfg, char* out, int32_t cap) {
    if (!cfg || !out || cap < 1 || cfg->B < 1 || cfg->n_agents < 1 || cfg->n_agents > MG_MAX_AGENTS || cfg->view_size < 1 ||
        cfg->view_size > MG_MAX_VIEW || cfg->tile_size < 1 || cfg->tile_size > 64 || cfg->cells_stride < 0 || cfg->n_tiles < 0)
        return MG_E_ARG;
    mg::RenderPick pick;
    if (!mg::render_pick(*cfg, mg::kPlain, &pick)) { out[0] = 0; return MG_E_LAUNCH; }      // (the configuration does not fit LDS: mg_render_obs_lds_bytes)
    snprintf(out, (size_t)cap, "mg::render_kernel<%d, %d, %d, %d, %d>", pick.vs, pick.ts, pick.wpb, pick.v, pick.rm);
    return (pick.vs == 0 ? 1 : 0) | (pick.ts == 0 ? 2 : 0);
}

int32_t mg_time_render_obs(const MgConfig* cfg, const MgState* st, uint8_t* obs, int32_t iters, float* avg_ms,
                           void* stream) {
    int e = check_cfg(cfg);
    if (e) return e;
    e = check_state(st);
    if (e) return e;
    if (!obs || !avg_ms || iters < 1) return MG_E_ARG;
    hipStream_t s = (hipStream_t)stream;
    hipEvent_t t0, t1;
    if (hipEventCreate(&t0) != hipSuccess || hipEventCreate(&t1) != hipSuccess) return MG_E_LAUNCH;
    hipError_t err = mg::launch_render(*cfg, *st, obs, nullptr, nullptr, nullptr, s);   // warm
    (void)hipEventRecord(t0, s);
    for (int i = 0; i < iters && err == hipSuccess; i++) err = mg::launch_render(*cfg, *st, obs, nullptr, nullptr, nullptr, s);
    (void)hipEventRecord(t1, s);
    (void)hipEventSynchronize(t1);
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, t0, t1);
    *avg_ms = ms / (float)iters;
    (void)hipEventDestroy(t0);
    (void)hipEventDestroy(t1);
    return rc(err);
}

int32_t mg_host_flag_alloc(int32_t** host, int32_t** dev) {
    if (!host || !dev) return MG_E_ARG;
    void* h = nullptr;
    void* d = nullptr;
    if (hipHostMalloc(&h, 64, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) return MG_E_LAUNCH;
    if (hipHostGetDevicePointer(&d, h, 0) != hipSuccess) { (void)hipHostFree(h); return MG_E_LAUNCH; }
    *static_cast<volatile int32_t*>(h) = 0;
    *host = static_cast<int32_t*>(h);
    *dev = static_cast<int32_t*>(d);
    return MG_OK;
}

int32_t mg_host_flag_free(int32_t* host) {
    if (!host) return MG_OK;
    return rc(hipHostFree(host));
}

void* mg_obs_alloc(uint64_t bytes, int32_t device) {
    if (bytes == 0) return nullptr;
    int cur = 0;
    (void)hipGetDevice(&cur);
    if (cur != device && hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    void* p = nullptr;
    const hipError_t e = hipMalloc(&p, (size_t)bytes);
    if (cur != device) (void)hipSetDevice(cur);
    if (e != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return p;
}

int32_t mg_obs_free(void* ptr) { return ptr ? rc(hipFree(ptr)) : MG_OK; }

}  // extern "C"
