// mg_step_layout.h — where the env step's scratch (mg::StepScratch, mg_core.h) lies in a workgroup's LDS: byte offsets and
// byte counts, written once for the kernels that carve it, the launchers that ask for it and the host harness under
// tests/native, which runs the step bodies on buffers of exactly these sizes.  Plain C++17 behind marlgrid_hip.h.
#pragma once

#if !defined(__HIPCC_RTC__)   // (a run-time compile — mg_rtc.hip — has no system headers: its source supplies these names)
#include <stddef.h>
#include <stdint.h>
#endif

#include "marlgrid_hip.h"

#if defined(__HIPCC__)
#define MG_LAYOUT_FN __host__ __device__ inline
#else
#define MG_LAYOUT_FN inline
#endif

namespace mg {

// Lane per env (step_kernel, the step phase of encode_views_kernel; S = 1 on the host): [item][S] columns, this env is
// column `col`.  The object table comes first, so that it is 16-byte aligned whatever n * S is and is staged in 16-byte
// pieces (stage_obj_tables, mg_core.h); `rec` follows on a multiple of 8, `head` on a multiple of 4.
struct LaneStepLayout { int obj, rec, head, act, fb, ord, oflags, total; };
MG_LAYOUT_FN LaneStepLayout lane_step_layout(int n, int S) {
    LaneStepLayout l;
    int o = 0;
    l.obj = o;    o += MG_MAX_OBJ * (int)sizeof(MgObjDesc);   // MgObjDesc [MG_MAX_OBJ] (shared by the lanes)
    l.rec = o;    o += n * S * 8;                             // u64 [n][S] agent records
    l.head = o;   o += MG_MT_HEAD * S * 4;                    // u32 [MG_MT_HEAD][S] look-ahead RNG words
    l.act = o;    o += n * S;                                 // u8 [n][S] actions
    l.fb = o;     o += n * S;                                 // u8 [n][S] pre-loaded front cells
    l.ord = o;    o += n * S;                                 // u8 [n][S] iter_order (more than 16 agents)
    l.oflags = o; o += MG_MAX_OBJ;                            // u8 [MG_MAX_OBJ] object flags (shared)
    l.total = o;
    return l;
}
MG_LAYOUT_FN size_t lane_step_bytes(int n, int S) { return (size_t)lane_step_layout(n, S).total; }

// Workgroup size of mg_step.  One lane per env: single-wave workgroups spread the envs over as many CUs as possible until
// the batch alone fills the chip several times over; then 256 lanes, where their columns fit the 64 KiB of LDS a launch
// gets without asking and the env has at most kStepWideAgents agents.  (The layout alone would admit 14; 13 is the bound
// every configuration has always launched with — worked out with one byte per agent and lane more than the layout has.)
constexpr int kStepWideAgents = 13;
MG_LAYOUT_FN int step_lanes(int n_agents, int B) {
    const bool wide = B > 256 * 8 * 64 && n_agents <= kStepWideAgents && lane_step_bytes(n_agents, 256) <= 64 * 1024;
    return wide ? 256 : 64;
}

// reset_kernel / place_kernel: u64 [n][S] records | u8 [MG_MAX_OBJ] object flags
MG_LAYOUT_FN size_t reset_scratch_bytes(int n, int S) { return (size_t)n * S * 8 + MG_MAX_OBJ; }

// The obs kernel's fused step (S = 8: lane j steps staged env j): records, RNG look-ahead, actions, the agent-parallel
// resolution's flags and turns (step_par_*; an env of more than 16 agents keeps its iter_order in `ordp`), the envs' step
// counts.  The object table and the flags are the workgroup's own (render_shared_layout).
struct FusedStepLayout { int rec, head, act, pflag, ordp, psc, total; };
MG_LAYOUT_FN FusedStepLayout fused_step_layout(int n) {
    FusedStepLayout l;
    int o = 0;
    l.rec = o;   o += n * 8 * 8;                // u64 [n][8]
    l.head = o;  o += MG_MT_HEAD * 8 * 4;       // u32 [MG_MT_HEAD][8]
    l.act = o;   o += n * 8;                    // u8 [n][8]
    l.pflag = o; o += n * 8;                    // u8 [n][8]
    l.ordp = o;  o += n * 8;                    // u8 [n][8]
    l.psc = o;   o += 8 * 4;                    // i32 [8]
    l.total = o;
    return l;
}
MG_LAYOUT_FN size_t fused_step_bytes(int n) { return (size_t)fused_step_layout(n).total; }

// mg_step_render_delta: the issue priority (s_setprio, 0 .. 3) of a wave that has finished `groups_done` of the `groups_total`
// view groups of its WHOLE run of envs (all its staged batches, not one batch).  A SIMD arbitrates between its waves by
// priority, then age: with every wave at 0 the oldest wave of a SIMD runs unimpeded and the youngest takes what is left.
// Ordered by progress, the wave that is behind out-ranks the wave that is ahead.  3 with nothing done, never rising, four
// levels spread evenly over the run: 3 - min(3, 4 * done / total) — 3, 2, 1, 0 for the bench shape's four groups.
MG_LAYOUT_FN int delta_wave_prio(int groups_done, int groups_total) {
    if (groups_done <= 0 || groups_total <= 0) return 3;
    if (groups_done >= groups_total) return 0;           // (below: done < total, the groups of ONE wave's run)
    const int q = 4 * groups_done / groups_total;          // 0 .. 3
    return 3 - q;
}

// mg_step_render_delta: the COMPACT signature.  A tmap entry of the delta instantiations is the tile's dword offset in the
// atlas — (orientation * n_tiles + tile) * tile_dwords —, so the 16 bits of an entry say what the quotient says: its CODE,
// one byte per view cell where the 4 * n_tiles codes leave 0xFF free (a host's 0xFF fill is then "no tile" in every cell).
// Layout inside the allocation of MG_DELTA_SIG_BYTES per env, which stays: every agent image has a slot of
// kDeltaSigSlot bytes of its own — vs * vs codes, [view row][view column], the rest padding —, env e begins at
// e * n * kDeltaSigSlot and the tail of the allocation is unused.  Whole slots are what a launch reads (16 bytes a lane) and
// what it writes back, and it writes back only the images with a changed band.  A configuration with more codes than a
// byte holds keeps the 16-bit entries, MG_DELTA_SIG_BYTES per env, all of it rewritten by every launch.
constexpr int kDeltaSigSlot = 64;
constexpr uint32_t kDeltaSigNone = 0xFFu;
MG_LAYOUT_FN bool delta_sig_compact(int n_tiles, int n_agents, int view_size) {
    return 4 * n_tiles <= (int)kDeltaSigNone && view_size * view_size <= kDeltaSigSlot &&
           n_agents * kDeltaSigSlot <= MG_DELTA_SIG_BYTES(n_agents, view_size);
}
MG_LAYOUT_FN uint32_t delta_sig_code(uint32_t entry, uint32_t tile_dwords) { return entry / tile_dwords; }
MG_LAYOUT_FN uint32_t delta_sig_entry(uint32_t code, uint32_t tile_dwords) { return code * tile_dwords; }
MG_LAYOUT_FN size_t delta_sig_env_bytes(int n_agents) { return (size_t)n_agents * kDeltaSigSlot; }
// byte offset of the slot of env e's agent image v
MG_LAYOUT_FN size_t delta_sig_slot(size_t e, int v, int n_agents) { return (e * (size_t)n_agents + (size_t)v) * kDeltaSigSlot; }

}  // namespace mg
