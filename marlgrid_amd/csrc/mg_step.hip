// mg_step.hip — batched MultiGridEnv.step action loop (marlgrid/base.py:501-649), with the reset of
// finished episodes (base.py:402-416) fused into its tail when the caller passes a reset program.
//
// Per env the reference is strictly sequential, so the only parallel axis is the env batch: one
// LANE per env (a wave-per-env mapping would idle 63 of 64 lanes through ~100 scalar instructions).
// The per-env body is mg::step_load / mg::step_run (mg_core.h).  What this file adds is the CDNA4
// shape of it:
//   * every per-env array the body indexes dynamically — agent records, the shuffled order, the
//     look-ahead RNG words — lives in LDS as [item][lane] columns (conflict-free), and the object
//     table is staged once per workgroup, so after the first memory round trip (all of it contiguous
//     across the batch: records, actions, RNG head, counters) the action loop only touches HBM for
//     the <= 2 grid cells an agent looks at;
//   * the RNG state proper (2.5 KB per env, three scattered words per draw) is only touched at the
//     very end, when the look-ahead head is topped up with all loads in flight at once;
//   * a finished env resets in the same lane right away (the done flag is computed by the lane that
//     would run the reset): no second launch, no second pass over the records.
#include "mg_device.h"
#include "mg_launch.h"

#if defined(MG_AB_VARIANTS)
#include <stdlib.h>
#endif

namespace mg {

template <int BS>
__global__ __launch_bounds__(BS) void step_kernel(MgConfig cfg, MgState st, StepArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t s_mem[];      // lane_step_layout(n, BS)
    const int n = cfg.n_agents, tid = threadIdx.x;
    StepScratch sc = lane_step_scratch(s_mem, n, BS, tid);
    if (a.has_ep) { sc.ep = &a.ep; sc.ep_rewards = a.rewards; }      // mg_step_ep (a launch-uniform branch)
    const int b = blockIdx.x * BS + tid;
    const bool live = b < cfg.B;

    const LaneStepLayout l = lane_step_layout(n, BS);
    stage_obj_tables(cfg, reinterpret_cast<MgObjDesc*>(s_mem + l.obj), s_mem + l.oflags, tid, BS);
    StepEnv env{0, 0};
    if (live) env = step_load(cfg, st, a.actions, a.action_bytes, b, sc);
    __syncthreads();
    if (!live) return;
    step_run(cfg, st, a.prog, a.has_prog != 0, a.rewards, b, env, sc, st.grid + (size_t)b * cfg.cells_stride);
}

template <int BS>
static hipError_t launch_step_bs(const MgConfig& cfg, const MgState& st, const StepArgs& a, hipStream_t s) {
    hipLaunchKernelGGL((step_kernel<BS>), dim3((cfg.B + BS - 1) / BS), dim3(BS), lane_step_bytes(cfg.n_agents, BS), s, cfg,
                       st, a);
    return hipGetLastError();
}

hipError_t launch_step(const MgConfig& cfg, const MgState& st, const void* actions, int action_bytes,
                       float* rewards, const MgGenProgram* prog, hipStream_t s, const MgEpisode* ep) {
    if (cfg.B <= 0) return hipSuccess;
    StepArgs a;
    if (!step_args(&a, actions, action_bytes, rewards, prog, ep)) return hipErrorInvalidValue;
    int bs = step_lanes(cfg.n_agents, cfg.B);
#if defined(MG_AB_VARIANTS)
    if (const char* f = getenv("MG_STEP_BLOCK")) { const int v = atoi(f); if (v == 64 || v == 256) bs = v; }
#endif
    if (bs == 256) return launch_step_bs<256>(cfg, st, a, s);
    return launch_step_bs<64>(cfg, st, a, s);
}

}  // namespace mg
