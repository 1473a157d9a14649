// mg_levels.hip — replayable levels (`env.seed(s); env.reset()`, marlgrid/base.py:371-374, 402-416): a bank of freshly
// seeded generators, and the launch in front of a reset or a step that hands an env which is about to reset its level's
// generator.  Bodies: mg_level_core.h.
//
// level_seed_kernel: one lane per row, as mt_seed_kernel — hashing a seed is a dependent chain of 80 rounds, init_by_array
// one of 1 247 steps; the parallelism is across rows.
// level_apply_kernel: one lane per env decides; the wave then copies for its selected lanes in turn, 64 lanes on one
// generator (2 496 + 64 + 4 bytes in three rounds of 16-byte accesses).  No LDS, no atomics, nothing the host has to read.
#include "mg_device.h"
#include "mg_launch.h"
#include "mg_level_core.h"

namespace mg {

__global__ __launch_bounds__(kBlock) void level_seed_kernel(int n, const int64_t* __restrict__ seeds, const int64_t* __restrict__ slots,
                                                            const uint8_t* __restrict__ mask, int n_slots, uint32_t* __restrict__ bank_mt,
                                                            int32_t* __restrict__ bank_pos, uint32_t* __restrict__ bank_head,
                                                            int64_t* __restrict__ bank_seed) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    level_seed_row(i, seeds, slots, mask, n_slots, bank_mt, bank_pos, bank_head, bank_seed);
}

__global__ __launch_bounds__(kBlock) void level_apply_kernel(MgConfig cfg, MgState st, int rule, const uint8_t* __restrict__ mask,
                                                             const int64_t* __restrict__ level_of_env, int n_slots,
                                                             const uint32_t* __restrict__ bank_mt, const int32_t* __restrict__ bank_pos,
                                                             const uint32_t* __restrict__ bank_head, const int64_t* __restrict__ bank_seed,
                                                             int64_t* __restrict__ episode_level, int64_t* __restrict__ out_level) {
    const int b = blockIdx.x * kBlock + threadIdx.x;
    const int lane = threadIdx.x & (kWave - 1);
    int what = kLevelKeep;
    if (b < cfg.B) what = level_select(cfg, st, b, rule, mask, level_of_env, n_slots, bank_seed);
    // the wave's selected lanes in turn, env and slot wave-uniform: every lane of the wave is here (no early return above)
    const int b0 = __builtin_amdgcn_readfirstlane(b - lane);
    unsigned long long todo = __ballot(what >= 0);
    while (todo) {
        const int l = __builtin_amdgcn_readfirstlane(__ffsll(todo) - 1);
        todo &= todo - 1;
        const int slot = __builtin_amdgcn_readlane(what, l);
        level_copy(st, b0 + l, slot, bank_mt, bank_pos, bank_head, lane, kWave);
    }
    if (b < cfg.B) level_publish(cfg, st, b, what, bank_seed, episode_level, out_level);
}

// ... the same launch for a bank whose levels carry their parameter row and edit list: the wave that copies a slot's generator
// copies the slot's rows over the env's, in the same lane loop
__global__ __launch_bounds__(kBlock) void level_apply_rows_kernel(MgConfig cfg, MgState st, int rule, const uint8_t* __restrict__ mask,
                                                                  const int64_t* __restrict__ level_of_env, int n_slots,
                                                                  const uint32_t* __restrict__ bank_mt, const int32_t* __restrict__ bank_pos,
                                                                  const uint32_t* __restrict__ bank_head, const int64_t* __restrict__ bank_seed,
                                                                  int64_t* __restrict__ episode_level, int64_t* __restrict__ out_level,
                                                                  LevelRows rows) {
    const int b = blockIdx.x * kBlock + threadIdx.x;
    const int lane = threadIdx.x & (kWave - 1);
    int what = kLevelKeep;
    if (b < cfg.B) what = level_select(cfg, st, b, rule, mask, level_of_env, n_slots, bank_seed);
    const int b0 = __builtin_amdgcn_readfirstlane(b - lane);
    unsigned long long todo = __ballot(what >= 0);
    while (todo) {
        const int l = __builtin_amdgcn_readfirstlane(__ffsll(todo) - 1);
        todo &= todo - 1;
        const int slot = __builtin_amdgcn_readlane(what, l);
        level_copy(st, b0 + l, slot, bank_mt, bank_pos, bank_head, lane, kWave, &rows);
    }
    if (b < cfg.B) level_publish(cfg, st, b, what, bank_seed, episode_level, out_level);
}

hipError_t launch_level_seed(int n, const int64_t* seeds, const int64_t* slots, const uint8_t* mask, int n_slots, uint32_t* bank_mt,
                             int32_t* bank_pos, uint32_t* bank_head, int64_t* bank_seed, hipStream_t s) {
    if (n <= 0 || n_slots <= 0) return hipSuccess;
    hipLaunchKernelGGL(level_seed_kernel, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, n, seeds, slots, mask, n_slots, bank_mt,
                       bank_pos, bank_head, bank_seed);
    return hipGetLastError();
}

hipError_t launch_level_apply(const MgConfig& cfg, const MgState& st, int rule, const uint8_t* mask, const int64_t* level_of_env,
                              int n_slots, const uint32_t* bank_mt, const int32_t* bank_pos, const uint32_t* bank_head,
                              const int64_t* bank_seed, int64_t* episode_level, int64_t* out_level, hipStream_t s) {
    if (cfg.B <= 0) return hipSuccess;
    hipLaunchKernelGGL(level_apply_kernel, dim3((cfg.B + kBlock - 1) / kBlock), dim3(kBlock), 0, s, cfg, st, rule, mask, level_of_env,
                       n_slots, bank_mt, bank_pos, bank_head, bank_seed, episode_level, out_level);
    return hipGetLastError();
}

hipError_t launch_level_apply_rows(const MgConfig& cfg, const MgState& st, int rule, const uint8_t* mask, const int64_t* level_of_env,
                                   int n_slots, const uint32_t* bank_mt, const int32_t* bank_pos, const uint32_t* bank_head,
                                   const int64_t* bank_seed, int64_t* episode_level, int64_t* out_level, const uint8_t* bank_params,
                                   const uint8_t* bank_edits, int K, uint8_t* env_params, uint8_t* env_edits, hipStream_t s) {
    if (cfg.B <= 0) return hipSuccess;
    LevelRows rows;
    rows.bank_params = reinterpret_cast<const uint32_t*>(bank_params);
    rows.env_params = reinterpret_cast<uint32_t*>(env_params);
    rows.bank_edits = reinterpret_cast<const uint32_t*>(bank_edits);
    rows.env_edits = reinterpret_cast<uint32_t*>(env_edits);
    rows.K = K;
    hipLaunchKernelGGL(level_apply_rows_kernel, dim3((cfg.B + kBlock - 1) / kBlock), dim3(kBlock), 0, s, cfg, st, rule, mask,
                       level_of_env, n_slots, bank_mt, bank_pos, bank_head, bank_seed, episode_level, out_level, rows);
    return hipGetLastError();
}

}  // namespace mg
