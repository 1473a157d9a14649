// mg_lookahead_core.h — the bodies of mg_fork_rows and mg_rollout (semantics: include/marlgrid_hip.h) as plain inline
// functions, like mg_core.h: the kernels of mg_lookahead.hip call them per wave / per lane, and the same text compiles with
// g++ for the host harness under tests/native.
//
//   fork_row     one destination row: a copy of one source row of another (or the same) MgState — generator, head, grid slice,
//                records, 'prestige', the four small words —, items lane, lane + lanes, ...: a wave calls it with its 64 lanes,
//                the host with (0, 1).  A source id outside the source batch leaves an INERT row: an ended episode that no
//                step ever touches.
//   rollout_row  one shadow row through T steps: mg::step_load / mg::step_run (mg_core.h, the bodies mg_step runs) with no
//                reset program and no MgEpisode, stopped at the episode's end.
#pragma once

#include "mg_core.h"

namespace mg {

typedef uint32_t LookVec __attribute__((vector_size(16)));       // one 16-byte load / store (hipcc and g++ alike)
constexpr int kLookMtVecs = MG_MT_N * 4 / 16;        // 156: a generator row is 2 496 bytes
constexpr int kLookHeadVecs = MG_MT_HEAD * 4 / 16;   // 4
static_assert(MG_MT_N * 4 % 16 == 0 && MG_MT_HEAD * 4 % 16 == 0, "generator rows are whole 16-byte vectors");
constexpr int kLookInertSteps = 0x7FFFFFFF;          // step_count of an inert row: past every max_steps
constexpr uint64_t kLookInertRecord = (uint64_t)MG_AF_DONE << (8 * MG_AG_FLAGS);     // ... and each of its agent records: done, in no cell

// which shadow row the w-th wave of a fork launch copies: the K = R / m rows that read one source row are neighbours in the
// launch (they meet in L2), while the rows themselves stay plan-major, r = p * m + j
MG_HD int fork_row_of_wave(int w, int R, int m) {
    const int K = R / m;
    return (w % K) * m + w / K;
}

// dst row (dst_of_row ? dst_of_row[r] : r) <- src row (src_of_dst ? src_of_dst[r % m] : r % m); cfg.B = rows of `src`.
// mt / mt_head of both states 16-byte aligned (the entry point checks).  The grid slice goes as 16-byte vectors where both
// slices are aligned, the rest of it as bytes.
MG_HD void fork_row(const MgConfig& cfg, const MgState& src, const MgState& dst, const int64_t* src_of_dst, const int64_t* dst_of_row,
                    int dst_B, int r, int m, int lane, int lanes) {
    const int n = cfg.n_agents, stride = cfg.cells_stride;
    const int64_t s64 = src_of_dst ? src_of_dst[r % m] : (int64_t)(r % m);
    const int64_t d64 = dst_of_row ? dst_of_row[r] : (int64_t)r;
    if (d64 < 0 || d64 >= (int64_t)dst_B) return;       // (no such destination: nothing is written)
    const bool inert = s64 < 0 || s64 >= (int64_t)cfg.B;
    const size_t s = inert ? 0 : (size_t)s64, d = (size_t)d64;
    const uint8_t* sg = src.grid + s * stride;
    uint8_t* dg = dst.grid + d * stride;
    const bool vec_ok = ((reinterpret_cast<uintptr_t>(sg) | reinterpret_cast<uintptr_t>(dg)) & 15) == 0;
    const int gv = vec_ok ? stride / 16 : 0, gb = stride - gv * 16;
    const bool pre = cfg.prestige_mask != 0;
    const LookVec zero = {0u, 0u, 0u, 0u};
    const LookVec* s_mt = reinterpret_cast<const LookVec*>(src.mt + s * MG_MT_N);
    const LookVec* s_head = reinterpret_cast<const LookVec*>(src.mt_head + s * MG_MT_HEAD);
    LookVec* d_mt = reinterpret_cast<LookVec*>(dst.mt + d * MG_MT_N);
    LookVec* d_head = reinterpret_cast<LookVec*>(dst.mt_head + d * MG_MT_HEAD);
    // the small words first (the first lanes), then the vectors, then the grid's byte tail
    const int o_rec = 4, o_pre = o_rec + n, o_mt = o_pre + (pre ? n : 0), o_head = o_mt + kLookMtVecs, o_gv = o_head + kLookHeadVecs,
              o_gb = o_gv + gv, items = o_gb + gb;
    for (int i = lane; i < items; i += lanes) {
        if (i == 0) dst.mt_pos[d] = inert ? MG_MT_HEAD : src.mt_pos[s];
        else if (i == 1) dst.step_count[d] = inert ? kLookInertSteps : src.step_count[s];
        else if (i == 2) dst.done[d] = inert ? (uint8_t)1 : src.done[s];
        else if (i == 3) dst.error[d] = inert ? 0 : src.error[s];
        else if (i < o_pre) dst.agents[d * n + (i - o_rec)] = inert ? kLookInertRecord : src.agents[s * n + (i - o_rec)];
        else if (i < o_mt) dst.prestige[d * n + (i - o_pre)] = inert ? 0.0 : src.prestige[s * n + (i - o_pre)];
        else if (i < o_head) d_mt[i - o_mt] = inert ? zero : s_mt[i - o_mt];
        else if (i < o_gv) d_head[i - o_head] = inert ? zero : s_head[i - o_head];
        else if (i < o_gb) reinterpret_cast<LookVec*>(dg)[i - o_gv] = inert ? zero : reinterpret_cast<const LookVec*>(sg)[i - o_gv];
        else dg[gv * 16 + (i - o_gb)] = inert ? (uint8_t)0 : sg[gv * 16 + (i - o_gb)];
    }
}

// Row r of the shadow state `st` (cfg.B = R rows, plan-major: r = p * m + j) through the T steps of its plan.  actions:
// [K][T][m][n] integers of `action_bytes` bytes; rewards: float32 [K][T][m][n]; done: uint8 [K][T][m]; errors: int32 [R] or
// null.  `sc`: the lane's step scratch (lane_step_scratch; the tables staged).  A step whose row's episode has ended —
// mg::episode_ended on the state, which an inert row satisfies from the start — writes zeros and done = 1 and touches nothing.
// `none`: an all-zero reset program (never read: nothing resets; a kernel hands in one of its arguments, so that none is built
// in scratch memory).
MG_HD void rollout_row(const MgConfig& cfg, const MgState& st, const MgGenProgram& none, const void* actions, int action_bytes, int T,
                       int m, float* rewards, uint8_t* done, int32_t* errors, int r, const StepScratch& sc) {
    const int n = cfg.n_agents, S = sc.S, col = sc.col;
    const int p = r / m, j = r - p * m;
    st.error[r] = 0;        // (the copied env's own error, if any, is the env's: the row reports what ITS steps record)
    uint8_t* g = st.grid + (size_t)r * cfg.cells_stride;
    bool frozen = false;
    for (int t = 0; t < T; t++) {
        // step_load and step_run index actions and rewards by the row: the base that puts row r at [p][t][j]
        const size_t at = ((size_t)p * T + t) * m + j;
        const size_t shift = (at - (size_t)r) * n;      // (at >= r: p T + t >= p)
        const void* a_t = static_cast<const uint8_t*>(actions) + shift * (size_t)action_bytes;
        float* r_t = rewards + shift;
        if (!frozen) {      // (an ended episode stays ended: nothing loads or steps it again)
            const StepEnv e = step_load(cfg, st, a_t, action_bytes, r, sc);
            frozen = episode_ended(cfg, sc.rec, S, col, e.sc0);
            if (!frozen) {
                step_run(cfg, st, none, false, r_t, r, e, sc, g);
                done[at] = st.done[r];
                continue;
            }
        }
        for (int k = 0; k < n; k++) rewards[at * n + k] = 0.0f;
        done[at] = 1;
    }
    if (errors) errors[r] = st.error[r];
}

}  // namespace mg
