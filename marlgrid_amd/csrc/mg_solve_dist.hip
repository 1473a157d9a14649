// mg_solve_dist.hip — mg_solve_distance: per env, for every agent, the exact number of actions (left / right / forward / pickup /
// toggle) to the step that enters a goal cell, through keys and doors; the first action of such a path; whether the env's doors
// and items were all tracked.  Semantics, the layer model and the bodies: mg_solve_core.h.
//
// One wave per selected env; a wave whose env is not selected exits at once.  Everything lives in LDS: the base free and goal
// maps once, per layer `visited` and two frontiers (a layer's free words are the base words patched from the table of tracked
// objects), and a tail of small tables.  A level is three phases handed over by the wave's own LDS hand-off (mg_device.h:
// wave_lds_sync): the plane recurrence inside every layer that has a frontier, the edges between layers (one lane per (layer,
// dir): at most 7 objects each), and the agents' look-up in layer 0.  A 64-bit wave-uniform mask names the layers with a
// non-empty frontier; the others are skipped.  The loop stops when every agent of the class is labelled, or when no frontier
// is left and no cost-2 edge is due, or at solve_max_levels.  No atomics, no global scratch, nothing the host has to read.
#include "mg_device.h"
#include "mg_launch.h"
#include "mg_solve_core.h"

namespace mg {

namespace {

// the OR over the wave of the lanes' layer masks, as a wave-uniform (scalar) value: one ballot where there is one layer, a
// butterfly of cross-lane reads otherwise
__device__ __forceinline__ uint64_t wave_or_layers(uint64_t v, int layers) {
    if (layers == 1) return __ballot(v & 1ull) ? 1ull : 0ull;
#pragma unroll
    for (int o = 32; o; o >>= 1) v |= (uint64_t)__shfl_xor((unsigned long long)v, o, kWave);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}

}  // namespace

__global__ __launch_bounds__(kWave) void solve_lds_kernel(MgConfig cfg, MgState st, const uint8_t* __restrict__ mask, int max_doors,
                                                          int max_items, int32_t* __restrict__ agent_dist,
                                                          int8_t* __restrict__ agent_action, uint8_t* __restrict__ env_exact) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int lane = threadIdx.x;
    const int b = blockIdx.x;
    if (mask && !mask[b]) return;       // (block-uniform: the block is one wave)
    const int W = cfg.W, H = cfg.H, n = cfg.n_agents;
    const SolveScratch s0 = solve_scratch(smem, W, H, max_doors, max_items);
    const uint8_t* grid_b = st.grid + (size_t)b * cfg.cells_stride;
    const uint64_t* rec_b = st.agents + (size_t)b * n;

    solve_build(cfg, grid_b, s0, lane, kWave);
    wave_lds_sync();
    solve_count(s0, lane, kWave);
    wave_lds_sync();
    solve_table(cfg, grid_b, s0, max_doors, max_items, lane, kWave);
    wave_lds_sync();
    const int D = __builtin_amdgcn_readfirstlane(s0.t->D), K = __builtin_amdgcn_readfirstlane(s0.t->K);

    for (int cls = solve_next_class(cfg, rec_b, -1); cls >= 0; cls = solve_next_class(cfg, rec_b, cls)) {
        SolveScratch s = s0;
        const int Ke = cls ? 0 : K, pass_key = cls >= 2 ? cls - 2 : -1;
        const int layers = solve_layers(D, Ke);
        const uint64_t all = layers >= 64 ? ~0ull : (1ull << layers) - 1ull;
        solve_pass_init(s, lane, kWave);
        const bool edges = D + Ke > 0;      // (no tracked object: one layer, mg_goal_distance's search)
        uint64_t fm = wave_or_layers(solve_expand(s, nullptr, s.front, layers, D, all, lane, kWave), layers), stale = all;
        wave_lds_sync();
        bool pending = __ballot(solve_agents(cfg, rec_b, s, nullptr, s.front, cls, Ke, 1, lane, kWave)) != 0;
        bool due = false;
        const int max_levels = solve_max_levels(W, H, layers, D);
        int level = 1;
        while (pending && (fm || due) && level < max_levels) {
            level++;
            uint64_t found = solve_expand(s, s.front, s.next, layers, D, fm | stale, lane, kWave);
            wave_lds_sync();
            if (edges) {
                bool mine = false;
                found |= solve_edges(s, s.front, s.next, layers, D, Ke, pass_key, lane, kWave, &mine);
                wave_lds_sync();
                due = __ballot(mine) != 0;
            }
            pending = __ballot(solve_agents(cfg, rec_b, s, s.front, s.next, cls, Ke, level, lane, kWave)) != 0;
            wave_lds_sync();        // (the agents read `front` too, and the next level writes it)
            stale = fm;
            fm = wave_or_layers(found, layers);
            uint64_t* t = s.front;
            s.front = s.next;
            s.next = t;
        }
        wave_lds_sync();
    }
    solve_finish(cfg, s0, agent_dist + (size_t)b * n, agent_action ? agent_action + (size_t)b * n : nullptr,
                 env_exact ? env_exact + b : nullptr, lane, kWave);
}

hipError_t launch_solve_distance(const MgConfig& cfg, const MgState& st, const uint8_t* mask, int max_doors, int max_items,
                                 int32_t* agent_dist, int8_t* agent_action, uint8_t* env_exact, hipStream_t s, int* unsupported) {
    *unsupported = 0;
    const size_t lds = solve_scratch_bytes(cfg.W, cfg.H, max_doors, max_items);
    if (lds > 160 * 1024) { *unsupported = 1; return hipSuccess; }
    if (cfg.B <= 0) return hipSuccess;
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&solve_lds_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(solve_lds_kernel, dim3(cfg.B), dim3(kWave), lds, s, cfg, st, mask, max_doors, max_items, agent_dist, agent_action,
                       env_exact);
    return hipGetLastError();
}

}  // namespace mg
