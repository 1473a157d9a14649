// mg_launch.h — host-side launchers implemented by the individual kernel translation units.
#pragma once
#include <hip/hip_runtime.h>

#include "marlgrid_hip.h"

namespace mg {
hipError_t launch_mt_seed(int B, const uint32_t* keys, const int32_t* key_len, uint32_t* mt, int32_t* mt_pos,
                          uint32_t* mt_head, hipStream_t s);
hipError_t launch_reset(const MgConfig& cfg, const MgState& st, const MgGenProgram& prog, const uint8_t* mask,
                        hipStream_t s);
hipError_t launch_step(const MgConfig& cfg, const MgState& st, const void* actions, int action_bytes,
                       float* rewards, const MgGenProgram* auto_reset, hipStream_t s, const MgEpisode* ep = nullptr);
struct FusedStep;
struct RenderPick;
// (which instantiation a configuration gets, whether it has one with the encode / the episode code, its LDS: mg_render_pick.h;
// `picked`: the caller's render_pick answer for this config and this step's want, where it has asked already)
hipError_t launch_render(const MgConfig& cfg, const MgState& st, uint8_t* obs, uint8_t* view_cells,
                         uint8_t* view_agent, uint8_t* vis_mask, hipStream_t s, const FusedStep* fused_step = nullptr,
                         const RenderPick* picked = nullptr);
// ... through a handle of mg_render_specialize (mg_rtc.hip); answers an MG_* code: MG_E_ARG when the handle was made for another shape
int32_t launch_render_spec(void* handle, const MgConfig& cfg, const MgState& st, uint8_t* obs, hipStream_t s,
                           const FusedStep* fused_step);
hipError_t launch_encode(const MgConfig& cfg, const MgState& st, const uint8_t* vis_mask, uint8_t* out,
                         hipStream_t s);
// every agent's gen_obs_grid -> encode (mg_encode_views.hip): out uint8 [B][nv][vs][vs][3]
struct EncViewsStep;
hipError_t launch_encode_views(const MgConfig& cfg, const MgState& st, uint8_t* out, hipStream_t s, const EncViewsStep* fs = nullptr);
// mg_step_encode_views: the step and the views in one launch where a workgroup of whole envs fits, else the two launches
hipError_t launch_step_encode_views(const MgConfig& cfg, const MgState& st, const void* actions, int action_bytes,
                                    float* rewards, const MgGenProgram* prog, uint8_t* out, hipStream_t s,
                                    const MgEpisode* ep = nullptr);
hipError_t launch_put_obj(const MgConfig& cfg, const MgState& st, int obj, int x, int y, const uint8_t* mask,
                          hipStream_t s);
hipError_t launch_place(const MgConfig& cfg, const MgState& st, int what, int x0, int y0, int x1, int y1, int max_tries,
                        const int32_t* fixed_pos, const uint8_t* mask, const uint8_t* reject, int32_t* out_pos,
                        uint8_t* out_ok, hipStream_t s);
hipError_t launch_frame(const MgConfig& cfg, const MgState& st, const int32_t* env_ids, int K, const uint8_t* atlas,
                        int ts, int highlight, uint32_t amax, uint8_t* out, hipStream_t s);
// replayable levels (mg_levels.hip): seed rows of a bank of generators; hand the envs that reset their level's generator
hipError_t launch_level_seed(int n, const int64_t* seeds, const int64_t* slots, const uint8_t* mask, int n_slots, uint32_t* bank_mt,
                             int32_t* bank_pos, uint32_t* bank_head, int64_t* bank_seed, hipStream_t s);
hipError_t launch_level_apply(const MgConfig& cfg, const MgState& st, int rule, const uint8_t* mask, const int64_t* level_of_env,
                              int n_slots, const uint32_t* bank_mt, const int32_t* bank_pos, const uint32_t* bank_head,
                              const int64_t* bank_seed, int64_t* episode_level, int64_t* out_level, hipStream_t s);
hipError_t launch_level_apply_rows(const MgConfig& cfg, const MgState& st, int rule, const uint8_t* mask, const int64_t* level_of_env,
                                   int n_slots, const uint32_t* bank_mt, const int32_t* bank_pos, const uint32_t* bank_head,
                                   const int64_t* bank_seed, int64_t* episode_level, int64_t* out_level, const uint8_t* bank_params,
                                   const uint8_t* bank_edits, int K, uint8_t* env_params, uint8_t* env_edits, hipStream_t s);
// goal distance (mg_goal_dist.hip): path 0 — the register-resident kernel where the grid fits a wave, else the LDS one —, 1 / 2
// force either; *unsupported = 1 and nothing launched when the forced or the only path cannot take the shape
hipError_t launch_goal_distance(const MgConfig& cfg, const MgState& st, const uint8_t* mask, int32_t* agent_dist, int32_t* field,
                                int path, hipStream_t s, int* unsupported);
// solve distance (mg_solve_dist.hip): *unsupported = 1 and nothing launched when the layers of (max_doors, max_items) do not fit LDS
hipError_t launch_solve_distance(const MgConfig& cfg, const MgState& st, const uint8_t* mask, int max_doors, int max_items,
                                 int32_t* agent_dist, int8_t* agent_action, uint8_t* env_exact, hipStream_t s, int* unsupported);
// lookahead (mg_lookahead.hip): rows of one state copied into another (one wave per row), and a shadow state's rows stepped T times
hipError_t launch_fork_rows(const MgConfig& cfg, const MgState& src, const MgState& dst, const int64_t* src_of_dst,
                            const int64_t* dst_of_row, int dst_B, int R, int m, hipStream_t s);
hipError_t launch_rollout(const MgConfig& cfg, const MgState& st, const void* actions, int action_bytes, int T, int m, float* rewards,
                          uint8_t* done, int32_t* errors, hipStream_t s);
// exploration maps (mg_explore.hip): the seen / visits planes of the config's viewers after one more observation
hipError_t launch_explore_update(const MgConfig& cfg, const MgState& st, const uint8_t* mask, uint8_t* seen, int32_t* visits,
                                 int32_t* new_cells, int32_t* visit_count, hipStream_t s);
// ... and with them the memory maps: memory u8 [B][n][W][H][4] (4-byte aligned), seen_step i32 [B][n][W][H]
hipError_t launch_memory_update(const MgConfig& cfg, const MgState& st, const uint8_t* mask, uint8_t* seen, int32_t* visits,
                                int32_t* new_cells, int32_t* visit_count, uint8_t* memory, int32_t* seen_step, hipStream_t s);
}  // namespace mg
