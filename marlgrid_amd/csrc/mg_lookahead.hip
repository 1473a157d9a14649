// mg_lookahead.hip — mg_fork_rows and mg_rollout: a second, shadow MgState is filled with copies of env rows and stepped
// through T actions per row in one launch, the env itself untouched.  Semantics: include/marlgrid_hip.h; bodies:
// mg_lookahead_core.h.
//
// fork_kernel: a bandwidth-bound gather of ~3 KB rows, one wave per destination row: the 2 496-byte generator, its 64-byte
// head and the grid slice as 16-byte vectors, the records and the four small words by the first lanes.  The K readers of one
// source row are neighbouring waves (fork_row_of_wave), so the source is read from HBM once.  Plain vector loads and stores.
// rollout_kernel: one lane per shadow row, mg_step's workgroup rule and LDS layout (step_lanes, lane_step_layout); the object
// tables are staged once, one barrier follows, and the T steps of a row run without another — a lane only ever touches its own
// LDS column and its own row.  No atomics (the shadow state has no error flag), nothing the host has to read.
#include "mg_device.h"
#include "mg_launch.h"
#include "mg_lookahead_core.h"

namespace mg {

__global__ __launch_bounds__(kBlock) void fork_kernel(MgConfig cfg, MgState src, MgState dst, const int64_t* __restrict__ src_of_dst,
                                                      const int64_t* __restrict__ dst_of_row, int dst_B, int R, int m) {
    const int w = blockIdx.x * (kBlock / kWave) + (int)(threadIdx.x / kWave);
    if (w >= R) return;
    fork_row(cfg, src, dst, src_of_dst, dst_of_row, dst_B, fork_row_of_wave(w, R, m), m, (int)(threadIdx.x & (kWave - 1)), kWave);
}

template <int BS>
__global__ __launch_bounds__(BS) void rollout_kernel(MgConfig cfg, MgState st, MgGenProgram none, const void* actions, int action_bytes,
                                                     int T, int m, float* rewards, uint8_t* done, int32_t* errors) {
    extern __shared__ __attribute__((aligned(16))) uint8_t s_mem[];      // lane_step_layout(n, BS)
    const int n = cfg.n_agents, tid = threadIdx.x;
    const StepScratch sc = lane_step_scratch(s_mem, n, BS, tid);
    const LaneStepLayout l = lane_step_layout(n, BS);
    stage_obj_tables(cfg, reinterpret_cast<MgObjDesc*>(s_mem + l.obj), s_mem + l.oflags, tid, BS);
    __syncthreads();
    const int r = blockIdx.x * BS + tid;
    if (r >= cfg.B) return;
    rollout_row(cfg, st, none, actions, action_bytes, T, m, rewards, done, errors, r, sc);
}

hipError_t launch_fork_rows(const MgConfig& cfg, const MgState& src, const MgState& dst, const int64_t* src_of_dst,
                            const int64_t* dst_of_row, int dst_B, int R, int m, hipStream_t s) {
    if (R <= 0) return hipSuccess;
    constexpr int per = kBlock / kWave;
    hipLaunchKernelGGL(fork_kernel, dim3((R + per - 1) / per), dim3(kBlock), 0, s, cfg, src, dst, src_of_dst, dst_of_row, dst_B, R, m);
    return hipGetLastError();
}

hipError_t launch_rollout(const MgConfig& cfg, const MgState& st, const void* actions, int action_bytes, int T, int m, float* rewards,
                          uint8_t* done, int32_t* errors, hipStream_t s) {
    if (cfg.B <= 0 || T <= 0) return hipSuccess;
    const int n = cfg.n_agents;
    const MgGenProgram none = {};       // (no reset program: nothing resets inside a rollout)
    if (step_lanes(n, cfg.B) == 256) {
        hipLaunchKernelGGL((rollout_kernel<256>), dim3((cfg.B + 255) / 256), dim3(256), lane_step_bytes(n, 256), s, cfg, st, none, actions,
                           action_bytes, T, m, rewards, done, errors);
    } else {
        hipLaunchKernelGGL((rollout_kernel<64>), dim3((cfg.B + 63) / 64), dim3(64), lane_step_bytes(n, 64), s, cfg, st, none, actions,
                           action_bytes, T, m, rewards, done, errors);
    }
    return hipGetLastError();
}

}  // namespace mg
