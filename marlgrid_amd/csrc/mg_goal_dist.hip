// mg_goal_dist.hip — mg_goal_distance: per env, the exact number of actions (left / right / forward) from every agent's state —
// and, when asked, from every state of the grid — to the step that enters a goal cell.  Semantics and bodies: mg_goal_core.h.
//
// One wave per selected env; a wave whose env is not selected exits at once.  The search is a reverse breadth-first search by
// levels over bit planes (per direction and column, the cells along y as bits), so a level is a handful of 64-bit ANDs, ORs
// and shifts per column instead of a queue.
//   goal_reg_kernel   4 W <= 64 and H <= 64 (every registered scenario): lane dir * W + x keeps its column's plane in
//                     registers.  Turns and +-x steps are cross-lane reads, termination is a ballot, lanes 0 .. n-1 each follow
//                     one agent by fetching the owning lane's frontier word once per level.  No LDS, no barrier in the loop.
//   goal_lds_kernel   every W, H <= 255: free / goal / visited / two frontiers in LDS (14 * 8 * W * ceil(H / 64) bytes + 128:
//                     111.7 KiB at 255 x 255), lanes striding over (dir, x, word) items, the wave's own LDS hand-off between
//                     the two halves of a level.
// Both: at most 4 W H + 1 levels whatever the grid holds; without a field they stop as soon as every agent of the env is
// labelled or the frontier is empty.  No atomics, no global scratch, nothing the host has to read.
#include "mg_device.h"
#include "mg_goal_core.h"
#include "mg_launch.h"

namespace mg {

namespace {

__device__ __forceinline__ uint64_t lane_read(uint64_t v, int src) { return (uint64_t)__shfl((unsigned long long)v, src, kWave); }

}  // namespace

__global__ __launch_bounds__(kBlock) void goal_reg_kernel(MgConfig cfg, MgState st, const uint8_t* __restrict__ mask,
                                                          int32_t* __restrict__ agent_dist, int32_t* __restrict__ field) {
    const int lane = threadIdx.x & (kWave - 1);
    const int b = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6)));
    if (b >= cfg.B || (mask && !mask[b])) return;       // (wave-uniform: every lane of the wave is here or none)
    const int W = cfg.W, H = cfg.H, n = cfg.n_agents;
    const bool has = lane < 4 * W;
    const int d = has ? lane / W : 0, x = has ? lane - d * W : 0;
    const uint8_t* grid_b = st.grid + (size_t)b * cfg.cells_stride;
    int32_t* field_b = field ? field + (size_t)b * W * H * 4 : nullptr;

    // the column's free and goal words: the four lanes of a column classify every fourth row each, and read the others' parts
    uint64_t free_w = 0, goal_w = 0;
    if (has) goal_column_bits(cfg, grid_b, x, 0, d, 4, H, &free_w, &goal_w);
    {       // (three reads of the PARTS, then the sum)
        const uint64_t pf = free_w, pg = goal_w;
        const int s1 = goal_reg_turn_lane(W, d, x, 1), s2 = goal_reg_turn_lane(W, d, x, 2), s3 = goal_reg_turn_lane(W, d, x, 3);
        free_w = pf | lane_read(pf, s1) | lane_read(pf, s2) | lane_read(pf, s3);
        goal_w = pg | lane_read(pg, s1) | lane_read(pg, s2) | lane_read(pg, s3);
    }
    if (!has) free_w = goal_w = 0;
    const uint64_t open_w = free_w | goal_w;

    // the agent this lane follows
    GoalAgent ag{0, 0, 0, 0};
    if (lane < n) ag = goal_agent(cfg, st.agents[(size_t)b * n + lane]);
    const int owner = ag.in_cell ? ag.d * W + ag.x : 0;
    int32_t my_dist = -1;

    const int ta = goal_reg_turn_lane(W, d, x, 1), tb = goal_reg_turn_lane(W, d, x, 3);
    int ok = 0;
    int ahead = lane;
    if (has) ahead = goal_reg_ahead_lane(W, d, x, &ok);
    const int max_levels = goal_max_levels(W, H);

    // level 1: the states that look at a goal
    uint64_t front = goal_reg_word(d, open_w, 0ull, 0ull, 0ull, goal_w, lane_read(goal_w, ahead), ok);
    uint64_t visited = front;
    int level = 1;
    for (;;) {
        if (field_b && front) goal_field_store(field_b, H, x, 0, d, front, level);
        const uint64_t at_owner = lane_read(front, owner);
        if (ag.in_cell && my_dist < 0 && ((at_owner >> ag.y) & 1ull)) my_dist = level;
        const bool any = __ballot(front != 0) != 0;
        const bool pending = __ballot(ag.in_cell && my_dist < 0) != 0;
        if (!any || (!field_b && !pending) || level >= max_levels) break;
        level++;
        const uint64_t walk = front & free_w;       // (a goal cell is entered, never crossed)
        const uint64_t nw = goal_reg_word(d, open_w, visited, lane_read(front, ta), lane_read(front, tb), walk, lane_read(walk, ahead), ok);
        visited |= nw;
        front = nw;
    }
    if (lane < n) agent_dist[(size_t)b * n + lane] = my_dist;
    if (field_b && has) goal_field_store(field_b, H, x, 0, d, ~visited & goal_row_mask(H, 0), -1);
}

__global__ __launch_bounds__(kWave) void goal_lds_kernel(MgConfig cfg, MgState st, const uint8_t* __restrict__ mask,
                                                         int32_t* __restrict__ agent_dist, int32_t* __restrict__ field) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int lane = threadIdx.x;
    const int b = blockIdx.x;
    if (mask && !mask[b]) return;       // (block-uniform: the block is one wave)
    const int W = cfg.W, H = cfg.H, n = cfg.n_agents;
    GoalScratch s = goal_scratch(smem, W, H);
    const uint8_t* grid_b = st.grid + (size_t)b * cfg.cells_stride;
    const uint64_t* rec_b = st.agents + (size_t)b * n;
    int32_t* field_b = field ? field + (size_t)b * W * H * 4 : nullptr;

    goal_gen_build(cfg, grid_b, s, lane, kWave);
    wave_lds_sync();
    bool any = __ballot(goal_gen_expand(s, nullptr, s.front, 1, field_b, lane, kWave)) != 0;
    wave_lds_sync();
    bool pending = __ballot(goal_gen_agents(cfg, rec_b, s, s.front, 1, lane, kWave)) != 0;
    const int max_levels = goal_max_levels(W, H);
    int level = 1;
    while (any && (field_b || pending) && level < max_levels) {
        level++;
        any = __ballot(goal_gen_expand(s, s.front, s.next, level, field_b, lane, kWave)) != 0;
        wave_lds_sync();
        pending = __ballot(goal_gen_agents(cfg, rec_b, s, s.next, level, lane, kWave)) != 0;
        uint64_t* t = s.front;
        s.front = s.next;
        s.next = t;       // (the next level writes the buffer nobody reads any more: no second hand-off)
    }
    wave_lds_sync();
    goal_gen_finish(cfg, s, agent_dist + (size_t)b * n, field_b, lane, kWave);
}

hipError_t launch_goal_distance(const MgConfig& cfg, const MgState& st, const uint8_t* mask, int32_t* agent_dist, int32_t* field,
                                int path, hipStream_t s, int* unsupported) {
    *unsupported = 0;
    if (cfg.B <= 0) return hipSuccess;
    const bool reg = path == kGoalPathAuto ? goal_reg_fits(cfg.W, cfg.H) : path == kGoalPathReg;
    if (reg) {
        if (!goal_reg_fits(cfg.W, cfg.H)) { *unsupported = 1; return hipSuccess; }
        constexpr int per_block = kBlock / kWave;
        hipLaunchKernelGGL(goal_reg_kernel, dim3((cfg.B + per_block - 1) / per_block), dim3(kBlock), 0, s, cfg, st, mask, agent_dist, field);
        return hipGetLastError();
    }
    const size_t lds = goal_scratch_bytes(cfg.W, cfg.H);
    if (lds > 160 * 1024) { *unsupported = 1; return hipSuccess; }
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&goal_lds_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(goal_lds_kernel, dim3(cfg.B), dim3(kWave), lds, s, cfg, st, mask, agent_dist, field);
    return hipGetLastError();
}

}  // namespace mg
