// mg_render_pick.h — which instantiation of mg::render_kernel<VS, TS, WPB, V, RM> (mg_render_kernel.h) a configuration gets,
// and the LDS layouts that decide it.  Plain C++17 with nothing but marlgrid_hip.h behind it: the HIP library's launcher
// (mg_render.hip), its kernels (the layout functions: host and device agree by sharing the text) and a g++ build for the
// tests (tests/native) read the same rules.  No environment, no globals, no HIP call.
#pragma once

#if !defined(__HIPCC_RTC__)   // (a run-time compile — mg_rtc.hip — has no system headers: its source supplies these names)
#include <stddef.h>
#include <stdint.h>
#endif

#include "marlgrid_hip.h"
#include "mg_step_layout.h"   // MG_LAYOUT_FN (the layout functions: the kernels call them too) and the fused step's columns

namespace mg {

MG_LAYOUT_FN int round_up(int v, int m) { return (v + m - 1) / m * m; }

// Block-shared LDS of the obs-render kernel behind the atlas, sized by the configuration (object kinds in sixteens): per
// object kind its flags, overlap slot, flags2 and — with hide_item_types — the mask of the agents that hide it; per agent
// its prestige scale and the viewer map; for the fused step the object table (32 B per kind) and the first kOpsLds ops of
// the reset program (the rest, if any, is read in place).  Offsets in bytes from the end of the atlas.
constexpr int kOpsLds = 32;
struct RenderShared { int no, oflags, oslot, oflags2, hideby, pscale, vmap, obj, ops, total; };
MG_LAYOUT_FN RenderShared render_shared_layout(const MgConfig& cfg) {
    RenderShared h;
    h.no = ((cfg.n_obj < 1 ? 1 : cfg.n_obj) + 15) & ~15;
    int o = 0;
    h.oflags = o;  o += h.no;
    h.oslot = o;   o += h.no;
    h.oflags2 = o; o += h.no;
    h.hideby = o;  o += cfg.any_hide ? h.no * 4 : 0;          // uint32 [no]
    h.pscale = o;  o += MG_MAX_AGENTS * 8;                    // double [MG_MAX_AGENTS]
    h.vmap = o;    o += MG_MAX_AGENTS;                        // uint8 [MG_MAX_AGENTS]
    o = (o + 15) & ~15;
    h.obj = o;     o += h.no * 32;                            // MgObjDesc [no]
    h.ops = o;     o += kOpsLds * 32;                         // MgGenOp [kOpsLds]
    h.total = o;
    return h;
}

// per-wave LDS scratch of the obs-render kernel (bytes), shared by host launch code and kernel
struct RenderScratch {
    int grid, rec, pres, pcol, vaff, first, second, trow, trow2, tmap, dyn, out, step, total;
    int stage_envs;    // envs whose inputs (grid + agent records) are staged per batch: 1..8
    int tmap_slots;    // tmaps a wave can hold at once (= stage_envs): the look-ahead depth of its env loop
    int tmap_stride;   // bytes per tmap slot
    int rec_stride;    // u64 records per staged env
    int piece_rows;    // assemble-and-stream raster: pixel rows assembled in LDS per piece (0: chunk raster)
    int out_chunks;    // ... and the size of its piece buffer in 16-byte chunks
    int view_slots;    // envs whose views are derived together: slots of first / second / trow (1, or stage_envs)
    int cell_stride;   // bytes per slot of first / second
    int trow_stride;   // dwords per slot of trow
};
// The atlas in LDS.  As it is in HBM ([4 orientations][n_tiles][ts][ts][3], rounded up to 16 bytes) — except for the
// GATHER raster (mg_gather.h; the kernel's RM_ == 2, `mode` 2 below), which is instantiated for the reference's default
// view with its default 5-pixel tiles (agents.py:21-22), for 6-, 7-, 9-, 10-, 11- and 12-pixel tiles (the tile sizes
// under 16 that the 16-byte-chunk raster does not take) and for views 3, 5, 9 at 5-pixel tiles: there every tile ROW gets 16 zero bytes in
// front (GatherGeom::RS bytes per row, 32 zero bytes behind the last), so that a 16-byte window anywhere around a row is
// whole aligned dwords with zeros outside the row — no edge masks, no conditional reads.
MG_LAYOUT_FN bool render_gather(const MgConfig& cfg) {
    const int vs = cfg.view_size, ts = cfg.tile_size;
    // ('prestige' agents — per-env recoloured tiles next to the atlas's —: the reference's example, 11-pixel tiles, and the default 5)
    if (vs == 7) return (ts == 5 || ts == 6 || ts == 7 || ts == 9 || ts == 10 || ts == 11 || ts == 12) && (cfg.prestige_mask == 0 || ts == 11 || ts == 5);
    // the other view sizes the 16-byte-chunk raster is instantiated for (3 .. 9, even ones included) and the large odd views
    // (11, 13, 15: 8-wave workgroups — their shadow-cast arrays need more than 128 VGPRs), at GridAgentInterface's default tile size
    return (vs == 3 || vs == 4 || vs == 5 || vs == 6 || vs == 8 || vs == 9 || vs == 11 || vs == 13 || vs == 15) && ts == 5 && cfg.prestige_mask == 0;
}
MG_LAYOUT_FN int render_gather_row_bytes(int ts) { return (16 + 3 * ts + 3) / 4 * 4; }
// The gather raster's cycle (mg_gather.h: GatherGeom takes its C and NT from here; render_pick_ideal asks at run time whether a
// (view, tile) pair has one).  A pixel row is RB = 3 * vs * ts bytes; the pattern of 16-byte chunks over rows repeats every
// PC = RB / gcd(16, RB) chunks = PR = 16 / gcd(16, RB) rows.  A CYCLE of C periods = NT <= 4 trips (= sets of lane constants):
// the C whose trips are best filled, whole bands of tiles (C * PR a multiple of TS: the tile row of a lane's segment is then a
// constant of the set — a quarter fewer instructions per window) counting for 1.3; ties: the smaller C.
constexpr int gather_gcd(int a, int b) { return b ? gather_gcd(b, a % b) : a; }
constexpr int gather_pick_c(int pc, int pr, int ts) {
    int best = 1, best_score = 0;
    for (int c = 1; c <= 8; c++) {
        const int cc = c * pc, nt = (cc + 63) / 64;
        if (nt > 4) continue;
        const int score = cc * 1000 / (nt * 64) * (((c * pr) % ts == 0) ? 13 : 10);
        if (score > best_score) { best = c; best_score = score; }
    }
    return best;
}
// trips per cycle (GatherGeom::NT); more than 4 — a period of more than 256 chunks — is a shape the gather raster does not take
constexpr int gather_trips(int vs, int ts) {
    const int rb = 3 * vs * ts, g = gather_gcd(16, rb);
    return (gather_pick_c(rb / g, 16 / g, ts) * (rb / g) + 63) / 64;
}
MG_LAYOUT_FN int render_atlas_raw_bytes(const MgConfig& cfg) {
    return (4 * cfg.n_tiles * cfg.tile_size * cfg.tile_size * 3 + 15) / 16 * 16;
}
// `mode`: the kernel's RM_ (0: by tile size, 1: assemble-and-stream forced — measurement builds —, 2: gather, 3: assemble-and-
// stream with the grid AND the atlas read in place — grids that do not fit LDS)
MG_LAYOUT_FN int render_atlas_lds_bytes(const MgConfig& cfg, int mode) {
    if (mode == 3) return 0;
    if (mode == 2) return (4 * cfg.n_tiles * cfg.tile_size * render_gather_row_bytes(cfg.tile_size) + 32 + 15) / 16 * 16;
    return render_atlas_raw_bytes(cfg);
}

// n: the env's agents (records, who stands where); nv: the viewers this launch renders (view-sized arrays)
MG_LAYOUT_FN RenderScratch render_scratch_layout(int cells_stride, int n, int nv, int vs, int stage_envs = 1,
                                                               int dyn_bytes = 0, int out_bytes = 0, int piece_rows = 0,
                                                               bool any_hide = true, int max_view_slots = 0, bool gather = false,
                                                               bool big = false) {
    RenderScratch s;
    int o = 0;
    s.stage_envs = stage_envs;
    s.rec_stride = round_up(n * 8, 16) / 8;
    // (big: a grid too large for LDS — the kernel's RM_ == 3 — is read in place, and who stands on a view cell is searched among
    // the env's agents instead of looked up in per-cell maps: no `grid`, `first`, `second`)
    s.grid = o;  o += big ? 0 : stage_envs * round_up(cells_stride, 16);
    s.rec = o;   o += stage_envs * s.rec_stride * 8;
    s.pres = o;  o += dyn_bytes ? stage_envs * s.rec_stride * 8 : 0;   // agent.prestige of the staged envs
    s.pcol = o;  o += dyn_bytes ? round_up(stage_envs * s.rec_stride * 4, 16) : 0;   // ... and the sprite colours it gives them (fused step)
    // Views of a GROUP of envs at once: a slot of first (second: only with hide_item_types — the agents of a cell) and
    // of trow (transparency rows; visibility replaces them in place) per env of the group; a view cell's (object,
    // agent) pair waits in the env's tmap slot.
    // (chunk raster — out_bytes == 0 —: up to 4 envs of views at a time; it is HBM-bound and a wave's first store
    // should not wait for eight envs of views; the assemble-and-stream rasters take the whole staged batch)
    // (the gather raster: no piece buffer either, but a group's raster is ONE stream over all its envs: the whole batch)
    s.view_slots = out_bytes == 0 && !gather && stage_envs > 4 ? 4 : stage_envs;
    if (max_view_slots > 0 && s.view_slots > max_view_slots) s.view_slots = max_view_slots;
    s.cell_stride = round_up(cells_stride, 16);
    // (trow doubles as the per-agent colour words of the 'prestige' recolouring: at least n dwords)
    s.trow_stride = round_up((nv * vs > n ? nv * vs : n) * 4, 16) / 4;
    s.vaff = o;  o += round_up(s.view_slots * nv * 8, 16);   // per viewer: its view's affine map and identity (phase 2b)
    s.first = o; o += big ? 0 : s.view_slots * s.cell_stride;
    s.second = o; o += any_hide && !big ? s.view_slots * s.cell_stride : 0;
    s.trow = o;  o += s.view_slots * s.trow_stride * 4;
    // (views of more than 15 rows: the shadow cast walks its rows in memory — mg_occlude.h —, the result next to the transparency)
    s.trow2 = o; o += vs > 15 ? s.view_slots * s.trow_stride * 4 : 0;
    s.tmap_slots = stage_envs;
    s.tmap_stride = gather ? nv * vs * vs * 2 : round_up(nv * vs * vs * 2, 16);   // (gather: DENSE — band g of a group is entry g * vs)
    s.tmap = o;  o += round_up(s.tmap_slots * s.tmap_stride, 16);
    s.dyn = o;   o += round_up(dyn_bytes, 16);   // per-env recoloured ('prestige') agent tiles
    s.out = o;   o += round_up(out_bytes, 16);   // assemble-and-stream raster: the piece being assembled
    s.piece_rows = piece_rows;
    s.out_chunks = round_up(out_bytes, 16) / 16;
    // fused step (mg_step_render): lane j < stage_envs steps staged env j; its [item][8] columns (fused_step_layout)
    s.step = o;  o += round_up((int)fused_step_bytes(n), 16);
    s.total = o;
    return s;
}
// the tile sizes the 16-byte-chunk raster is instantiated for (whole pairs of dwords per tile row);
// everything else — and `mode` 1, measurement builds — takes the assemble-and-stream raster
MG_LAYOUT_FN bool render_chunk_raster(const MgConfig& cfg, int mode) {
    return (cfg.tile_size == 8 || cfg.tile_size == 16 || cfg.tile_size == 32) && mode == 0;
}
// The layout a launch of the obs kernel uses, from the config and the workgroup size alone (kernel and
// launcher agree): recoloured-tile space when some agent is 'prestige'; for the assemble-and-stream raster
// (tile sizes off the 16-byte-chunk path; `mode` 1 forces it — measurement builds) the piece buffer: as
// many whole pixel rows as fit ~4 KiB (at least one) plus 32 bytes for the carried-over partial chunk;
// and as many staged envs per batch (8, 4, 2 or 1) as `wpb` waves of scratch leave room for.
MG_LAYOUT_FN RenderScratch render_scratch_for(const MgConfig& cfg, int wpb, int mode = 0) {
    const int n = cfg.n_agents, vs = cfg.view_size, ts = cfg.tile_size;
    const int nv = cfg.n_view ? cfg.n_view : n;
    // (the recoloured tiles of a 'prestige' env: as the atlas's — gather raster: in padded rows)
    const int dyn = cfg.prestige_mask ? (cfg.any_hide ? 2 : 1) * n * 4 * ts * (mode == 2 ? render_gather_row_bytes(ts) : ts * 3) + (mode == 2 ? 32 : 0) : 0;
    // (`fixed`: what a workgroup holds besides its waves' scratch — exactly the launcher's sum, launch_render_t)
    const int atlas_b = render_atlas_lds_bytes(cfg, mode), fixed = render_shared_layout(cfg).total;
    const bool gather = mode == 2, big = mode == 3;
    int rows = 0, out = 0;
    if (!gather && !render_chunk_raster(cfg, mode)) {
        const int rb = 3 * vs * ts;
        rows = 4096 / rb;
        if (rows < 1) rows = 1;
        if (rows > nv * vs * ts) rows = nv * vs * ts;
        out = 32 + rows * rb;
    }
    // the views of several envs are derived together — one lane per viewer in the shadow cast (its ~420 instructions
    // run once per group instead of once per env), full trips in the per-cell phases — with one slot of view scratch per
    // env of the group (see the kernel's pass 0); the recoloured tiles of a 'prestige' env keep their one slot (they are
    // made right before the env's raster)
    const RenderScratch b = render_scratch_layout(cfg.cells_stride, n, nv, vs, 1, dyn, out, rows, true, 0, gather, big);
    const int resident = (atlas_b + 4 * b.total + fixed <= 160 * 1024) ? atlas_b : 0;   // else the atlas is read in place
    // (a wave stages its batch's records with two per lane — mg_render_kernel.h, step_load_issue —: up to 8 envs of up to
    // 16 agents, 4 envs of more)
    const int kmax = n > 16 ? 4 : 8;
    // ('prestige' — 12-wave workgroups next to a large atlas —: fewer view slots before fewer staged envs or fewer waves)
    for (int slots = dyn ? kmax : 0; dyn && slots >= 1; slots >>= 1) {
        const RenderScratch t = render_scratch_layout(cfg.cells_stride, n, nv, vs, kmax, dyn, out, rows, cfg.any_hide != 0, slots, gather, big);
        if (resident + wpb * t.total + fixed <= 160 * 1024) return t;
    }
    int k = kmax;
    while (k > 1 && resident + wpb * render_scratch_layout(cfg.cells_stride, n, nv, vs, k, dyn, out, rows, cfg.any_hide != 0, dyn ? 1 : 0, gather, big).total + fixed > 160 * 1024) k >>= 1;
    return render_scratch_layout(cfg.cells_stride, n, nv, vs, k, dyn, out, rows, cfg.any_hide != 0, dyn ? 1 : 0, gather, big);
}

// ---- the pick (host only) --------------------------------------------------------------------------------------------------

constexpr size_t kRenderLdsMax = 160 * 1024;

// which instantiation (0 = the value is read from the config at run time) and the LDS bytes of one of its workgroups
struct RenderPick { int vs, ts, wpb, v, rm, lds; };
// what the launch has to do besides the raster: nothing (mg_render_obs, mg_step_render), MultiGrid.encode of the stepped batch
// (mg_step_render_encode: the instantiations V + 16, MG_RENDER_GROUP_N), the episode outputs (mg_step_render_ep: V + 32, group P)
// ... or the band-wise comparison against the signature of what the output buffer already holds (mg_step_render_delta: V + 64,
// MG_RENDER_DELTA — a list of its own, not part of MG_RENDER_ALL) ... or that comparison TOGETHER with the encode, the episode
// outputs or both (mg_step_render_delta_ex: V + 64 + 16 | 32 | 48, MG_RENDER_DELTA_X — a second list of its own)
enum RenderWant { kPlain, kEncode, kEpisode, kDelta, kDeltaEncode, kDeltaEpisode, kDeltaEncodeEpisode };
constexpr bool render_want_delta(RenderWant w) { return w >= kDelta; }
constexpr bool render_want_encode(RenderWant w) { return w == kEncode || w == kDeltaEncode || w == kDeltaEncodeEpisode; }
constexpr bool render_want_episode(RenderWant w) { return w == kEpisode || w == kDeltaEpisode || w == kDeltaEncodeEpisode; }
// ... from what a launch was handed: a signature (the delta), an encode output, an MgEpisode.  (The encode AND the episode
// outputs: under the delta alone — there is no non-delta instantiation with both, the launcher refuses that pair.)
inline RenderWant render_want_of(bool sig, bool encode, bool episode) {
    return sig ? (episode && encode ? kDeltaEncodeEpisode : episode ? kDeltaEpisode : encode ? kDeltaEncode : kDelta)
               : episode ? kEpisode : encode ? kEncode : kPlain;
}

// dwords of the fused encode's LDS table — one per grid byte value, (n_obj + 4 n) rounded up to 16 —, 0: object ids and
// agent marks do not share a byte, no fused encode
inline int render_enc_entries(const MgConfig& cfg) { return cfg.n_obj + 4 * cfg.n_agents <= 256 ? ((cfg.n_obj + 4 * cfg.n_agents + 15) & ~15) : 0; }

// LDS of one workgroup: the atlas (variants 8 and 12 leave it in global memory), the block-shared tables, the fused encode's
// table, `wpb` waves of scratch.  What the pick reports and what the launch asks for.
inline size_t render_lds_bytes(const MgConfig& cfg, int wpb, int mode, int v = 0, int enc_ne = 0) {
    const size_t atlas = ((v & 15) == 8 || (v & 15) == 12) ? 0 : (size_t)render_atlas_lds_bytes(cfg, mode);
    return atlas + (size_t)render_shared_layout(cfg).total + (size_t)enc_ne * 4 + (size_t)wpb * render_scratch_for(cfg, wpb, mode).total;
}
inline bool render_fits(const MgConfig& cfg, int wpb, int mode) { return render_lds_bytes(cfg, wpb, mode) <= kRenderLdsMax; }

// The raster a configuration gets (the kernel's RM_): 2 = gather (mg_gather.h) where it is instantiated and its padded
// atlas fits LDS next to 4 waves of scratch, else 0 = by tile size (16-byte chunks / assemble-and-stream).
inline int render_mode_for(const MgConfig& cfg) { return render_gather(cfg) && render_fits(cfg, 4, 2) ? 2 : 0; }

// LDS of the smallest shape of the ordinary variants (4 waves, one staged env, the atlas read in place when it does not fit)
inline int render_small_lds_bytes(const MgConfig& cfg) {
    const int mode = render_mode_for(cfg);
    const size_t all = render_lds_bytes(cfg, 4, mode);
    return (int)(all <= kRenderLdsMax ? all : all - render_atlas_lds_bytes(cfg, mode));   // else the atlas is read in place
}
// A grid whose staged copy (and the per-cell first-agent maps beside it) does not fit LDS even then — beyond ~140 x 140, ~110 x
// 110 with hide_item_types — takes the variant that reads the grid in place (RM_ == 3; with 'prestige' agents: their recoloured tiles in LDS beside it).
inline bool render_big_grid(const MgConfig& cfg) { return (size_t)render_small_lds_bytes(cfg) > kRenderLdsMax; }

// mg_render_obs_lds_bytes
inline int render_min_lds_bytes(const MgConfig& cfg) {
    return render_big_grid(cfg) ? (int)render_lds_bytes(cfg, 4, 3) : render_small_lds_bytes(cfg);
}

// Workgroup shape.  16 waves per workgroup walk 16 *adjacent* envs at a time (a 450 KB contiguous
// output window per workgroup, one atlas copy per 16 waves): measured +7..13 % HBM write throughput
// over 4-wave workgroups at the bench batch.  Small batches keep 4-wave workgroups so that they
// still spread over all CUs.
inline int choose_wpb(const MgConfig& cfg, int mode) { return cfg.B >= 4096 && render_fits(cfg, 16, mode) ? 16 : 4; }

// mg_step_render_delta (V + 64), what its instantiations take from a wave's scratch WITHOUT growing it: the old signatures of a
// staged batch land in the envs' own tmap slots with the staging loads (16-bit entries: a tmap slot per env, three 16-byte requests
// per lane, 3 KiB at most; the compact codes of mg_step_layout.h — 64 bytes per agent image — take the front of the same area); the tmaps
// of the view group being derived — two envs at 8-pixel tiles — and the group's two band-mask words live in the fused step's
// columns (free once the batch is stepped); a band mask is one word (nv * vs bands).  At most three agents — whatever the grid
// leaves of the batch size — is what all of it holds for.
MG_LAYOUT_FN bool render_delta_fits(const MgConfig& cfg, const RenderScratch& L) {
    const int nv = cfg.n_view ? cfg.n_view : cfg.n_agents;
    return cfg.n_view == 0 && cfg.n_agents <= 3 && nv * cfg.view_size <= 32 && L.stage_envs * L.tmap_stride <= 3 * 64 * 16 &&
           2 * L.tmap_stride + 16 <= round_up((int)fused_step_bytes(cfg.n_agents), 16);
}

// The one rule set.  false: no instantiation for this `want` (the C ABI answers MG_E_UNSUPPORTED: hosts take the plain step
// launch and mg_encode, or mg_step_ep and mg_render_obs) or the launch does not fit LDS (mg_render_obs_lds_bytes).  Every
// pick it can return is an entry of MG_RENDER_ALL (mg_render_kernel.h; tests/test_render_pick.py holds both to it).
inline bool render_pick(const MgConfig& cfg, RenderWant want, RenderPick* out) {
    const int vs = cfg.view_size, ts = cfg.tile_size;
    const bool prestige = cfg.prestige_mask != 0;
    const int chunk_ts = (ts == 8 || ts == 16 || ts == 32) ? ts : 0;     // the tile sizes the 16-byte-chunk raster is compiled for
    RenderPick p = {0, 0, 4, 0, 0, 0};
    if (render_big_grid(cfg)) {
        // 1. the grid read in place: everything about the view and the tiles at run time, 4-wave workgroups
        p.v = prestige ? 12 : 8;
        p.rm = 3;
    } else {
        const int mode = render_mode_for(cfg);
        const int wpb = choose_wpb(cfg, mode);
        if (prestige) {
            // 2. per-env recoloured agent tiles in LDS (variant 9; 12: the static atlas stays in global memory).  The recolouring
            // code needs ~165 VGPRs, more than the 128 a 16-wave workgroup leaves per lane: 12-wave workgroups (3 waves per SIMD,
            // 168 VGPRs) where their scratch fits next to the atlas, else 8 — 0.52 -> 0.59 of 8 TB/s with three 'prestige' agents
            // at tile 8, 0.24 -> 0.29 for the reference's example (one agent, tile 11) against 8-wave workgroups
            // (profiles/r03/ab_offpath*.jsonl)
            p.v = 9;
            if (!render_fits(cfg, 4, 0)) {
                p.ts = chunk_ts;
                p.v = 12;
            } else if (mode == 2) {          // examples/human_player.py's view_tile_size 11 and GridAgentInterface's default 5
                p.vs = 7; p.ts = ts; p.rm = 2;
                p.wpb = wpb < 16 ? wpb : render_fits(cfg, 12, 2) ? 12 : render_fits(cfg, 8, 2) ? 8 : 4;
            } else if (vs == 7 && (ts == 8 || ts % 8 != 0)) {      // the shipped view: compile-time size
                p.vs = 7; p.ts = chunk_ts;
                p.wpb = wpb < 16 ? wpb : render_fits(cfg, 12, 0) ? 12 : 8;
            } else {
                p.ts = chunk_ts;
            }
        } else if (mode == 2) {
            // 3. the gather raster — exactly the shapes render_gather admits: view 7 (GridAgentInterface's default, agents.py:21)
            // with 5- .. 12-pixel tiles; views 3 .. 9 at its default 5-pixel tiles; views 11 / 13 / 15 there with 8-wave workgroups
            // where their scratch fits (their shadow-cast arrays need more than 128 VGPRs)
            p.vs = vs; p.ts = ts; p.rm = 2;
            p.wpb = vs <= 9 ? wpb : cfg.B >= 4096 && render_fits(cfg, 8, 2) ? 8 : 4;
        } else if (!render_fits(cfg, 4, 0)) {
            // 4. an atlas too large for LDS (next to 4 waves of scratch) is read from global memory (variant 8)
            p.ts = chunk_ts;
            p.v = 8;
        } else {
            // 5. the view compiled in (exact dividers, a shadow cast of VS rows) for the views 3 .. 9 — odd and even: agents.py:233-266
            // as it is written — at 8-pixel tiles and at the assemble-and-stream tile sizes, for the default view at 16 and 32; 6. a
            // run-time view's MG_MAX_VIEW-entry shadow-cast arrays need more than the 128 VGPRs of a 16-wave workgroup (spills would
            // be VMEM traffic in the middle of the run): 8 waves
            const bool view_ct = chunk_ts == 16 || chunk_ts == 32 ? vs == 7 : vs >= 3 && vs <= 9;
            p.vs = view_ct ? vs : 0;
            p.ts = chunk_ts;
            p.wpb = view_ct || wpb < 16 ? wpb : 8;
        }
    }
    int enc_ne = 0;
    if (want != kPlain) {
        // the plain pick, for the shapes compiled with the encode / the episode code: the BASELINE configs (views 7 and 9 at 8-pixel
        // tiles), any view over 9 at 8-pixel tiles (a view 3 ... 6, 8 there has a specialised plain instantiation: a second launch costs
        // it +7 %, the run-time-view instantiation would cost +40 %; views 1 and 2 are not among them either), GridAgentInterface's defaults (view 7 at 5-pixel tiles, gather).
        // Not: a grid read in place, 'prestige' agents, an atlas in global memory (all V != 0).
        const bool shape = p.v == 0 && ((p.rm == 2 && p.vs == 7 && p.ts == 5) ||
                                        (p.rm == 0 && p.ts == 8 && (p.vs == 7 || p.vs == 9 || (p.vs == 0 && vs > 9))));
        // (mg_step_render_delta, mg_step_render_delta_ex: the headline shape alone — view 7 at 8-pixel tiles, the fixed-lane chunk
        // raster — with few enough agents for render_delta_fits; what it asks of a wave's layout does not depend on the workgroup)
        if (render_want_delta(want) ? !(shape && p.rm == 0 && p.vs == 7 && render_delta_fits(cfg, render_scratch_for(cfg, p.wpb, 0))) : !shape) return false;
        p.v |= (render_want_encode(want) ? 16 : 0) | (render_want_episode(want) ? 32 : 0) | (render_want_delta(want) ? 64 : 0);
        if (render_want_encode(want)) {
            // the encode's table has to fit beside FOUR waves of scratch, whatever the batch: render_scratch_for fills LDS with staged
            // envs, so a larger workgroup's leaner layout may fit where this one does not — such a configuration has no fused encode
            enc_ne = render_enc_entries(cfg);
            if (enc_ne == 0 || render_lds_bytes(cfg, 4, p.rm, 0, enc_ne) > kRenderLdsMax) return false;
        }
    }
    size_t lds = render_lds_bytes(cfg, p.wpb, p.rm, p.v, enc_ne);
    if (lds > kRenderLdsMax && enc_ne) {      // ... and where it does not fit beside 16 / 8 waves of scratch, the workgroup is 4 waves
        p.wpb = 4;
        lds = render_lds_bytes(cfg, 4, p.rm, p.v, enc_ne);
    }
    if (lds > kRenderLdsMax) return false;
    p.lds = (int)lds;
    *out = p;
    return true;
}

// ---- the pick if any instantiation could be made (mg_rtc.hip: mg_render_specialize compiles it at run time) ---------------------
// Which instantiation the configuration would get if its view and tile size were compiled in; false: nothing to gain, the
// table's answer stays.  Only the three raster families of the table, with new values:
//   gather              <vs, ts, W, V, 2>  ts >= 5, ts % 8 != 0, a cycle of at most 4 trips (gather_trips), the padded atlas in LDS
//   chunk               <vs, ts, W, V, 0>  ts 8, 16, 32
//   assemble-and-stream <vs, 0, W, V, 0>   everything else (a compile-time tile size off the chunk sizes is no family of the table)
// W: 4 under 4096 envs, else 16 for views up to 9 and 8 above (larger views' shadow-cast arrays need more than 128 VGPRs), stepped
// down 16 -> 8 -> 4 while the workgroup does not fit LDS.  V: + 16 (kEncode, under render_pick's own conditions: a table for every
// grid byte value that fits beside four waves of scratch) or + 32 (kEpisode).  Not specialised: a grid read in place, 'prestige'
// agents, an atlas in global memory (every V != 0 of the table), kDelta, views under 3 — and a shape the table already has compiled in
// (its view and the family's tile size: a hand-picked entry, whatever its workgroup, is never replaced).
inline bool render_pick_ideal(const MgConfig& cfg, RenderWant want, RenderPick* out) {
    const int vs = cfg.view_size, ts = cfg.tile_size;
    RenderPick plain;
    if (render_want_delta(want) || vs < 3 || vs > MG_MAX_VIEW || !render_pick(cfg, kPlain, &plain) || plain.v != 0) return false;
    RenderPick p = {vs, 0, 4, 0, 0, 0};
    if (ts >= 5 && ts % 8 != 0 && gather_trips(vs, ts) <= 4 && render_fits(cfg, 4, 2)) { p.ts = ts; p.rm = 2; }
    else if (!render_fits(cfg, 4, 0)) return false;
    else if (ts == 8 || ts == 16 || ts == 32) p.ts = ts;
    int enc_ne = 0;
    if (want == kEncode) {
        enc_ne = render_enc_entries(cfg);
        if (enc_ne == 0 || render_lds_bytes(cfg, 4, p.rm, 0, enc_ne) > kRenderLdsMax) return false;
        p.v = 16;
    } else if (want == kEpisode) {
        p.v = 32;
    }
    p.wpb = cfg.B < 4096 ? 4 : vs <= 9 ? 16 : 8;
    while (p.wpb > 4 && render_lds_bytes(cfg, p.wpb, p.rm, p.v, enc_ne) > kRenderLdsMax) p.wpb >>= 1;
    const size_t lds = render_lds_bytes(cfg, p.wpb, p.rm, p.v, enc_ne);
    if (lds > kRenderLdsMax) return false;
    p.lds = (int)lds;
    RenderPick t;
    if (render_pick(cfg, want, &t) && t.vs == p.vs && t.ts == p.ts && t.v == p.v && t.rm == p.rm) return false;
    *out = p;
    return true;
}

}  // namespace mg

// ---- the instantiations ------------------------------------------------------------------------------------------------------
// In groups: mg_render_inst.hip, compiled once per group (-DMG_RENDER_INST_GROUP=<g>, in parallel), makes them; the launcher
// (mg_render.hip) looks render_pick's answer up in their list, MG_RENDER_ALL, and only refers to them.
// MG_RENDER_GROUP_x(X): X(VS, TS, WPB, V, RM).
#define MG_RENDER_GROUP_A(X) /* the chunk raster at tile 8 */                                                              \
    X(7, 8, 16, 0, 0) X(7, 8, 4, 0, 0) X(9, 8, 16, 0, 0) X(9, 8, 4, 0, 0) X(5, 8, 16, 0, 0) X(5, 8, 4, 0, 0)   \
    X(3, 8, 16, 0, 0) X(3, 8, 4, 0, 0) X(0, 8, 8, 0, 0) X(0, 8, 4, 0, 0)
#define MG_RENDER_GROUP_B(X) /* tile 16 / 32, the atlas in global memory */                                                \
    X(7, 16, 16, 0, 0) X(7, 16, 4, 0, 0) X(7, 32, 16, 0, 0) X(7, 32, 4, 0, 0) X(0, 16, 8, 0, 0) X(0, 16, 4, 0, 0)               \
    X(0, 32, 8, 0, 0) X(0, 32, 4, 0, 0) X(0, 8, 4, 8, 0) X(0, 16, 4, 8, 0) X(0, 32, 4, 8, 0) X(0, 0, 4, 8, 0) X(0, 0, 4, 8, 3)
#define MG_RENDER_GROUP_C(X) /* assemble-and-stream: any other tile size */                                                \
    X(7, 0, 16, 0, 0) X(7, 0, 4, 0, 0) X(0, 0, 8, 0, 0) X(0, 0, 4, 0, 0)
#define MG_RENDER_GROUP_D(X) /* 'prestige': per-env recoloured tiles */                                                     \
    X(7, 8, 12, 9, 0) X(7, 8, 8, 9, 0) X(7, 8, 4, 9, 0)                                                                       \
    X(0, 8, 4, 9, 0) X(0, 16, 4, 9, 0)
#define MG_RENDER_GROUP_E(X)                                                                                               \
    X(7, 0, 12, 9, 0) X(7, 0, 8, 9, 0) X(7, 0, 4, 9, 0) X(0, 32, 4, 9, 0) X(0, 0, 4, 9, 0)                                      \
    X(0, 8, 4, 12, 0) X(0, 16, 4, 12, 0) X(0, 32, 4, 12, 0) X(0, 0, 4, 12, 0) X(0, 0, 4, 12, 3)
#if defined(MG_EXP) && (MG_EXP & 8)
#define MG_RENDER_GROUP_X(X) X(7, 8, 12, 0, 0)      /* experiment builds only (mg_render.hip); made with group G */
#else
#define MG_RENDER_GROUP_X(X)
#endif
#define MG_RENDER_GROUP_G(X) /* the gather raster (mg_gather.h): view 7, 5- and 6-pixel tiles */                          \
    X(7, 5, 16, 0, 2) X(7, 5, 4, 0, 2) X(7, 6, 16, 0, 2) X(7, 6, 4, 0, 2) MG_RENDER_GROUP_X(X)
#define MG_RENDER_GROUP_H(X) /* ... 7-, 9- and 10-pixel tiles */                                                           \
    X(7, 7, 16, 0, 2) X(7, 7, 4, 0, 2) X(7, 9, 16, 0, 2) X(7, 9, 4, 0, 2) X(7, 10, 16, 0, 2) X(7, 10, 4, 0, 2)
#define MG_RENDER_GROUP_M(X) /* the gather raster for views 11, 13, 15 at 5-pixel tiles (8-wave workgroups) */                  \
    X(11, 5, 8, 0, 2) X(11, 5, 4, 0, 2) X(13, 5, 8, 0, 2) X(13, 5, 4, 0, 2) X(15, 5, 8, 0, 2) X(15, 5, 4, 0, 2)
#define MG_RENDER_GROUP_L(X) /* assemble-and-stream with a compile-time view: views 3 .. 9 at any tile size */                    \
    X(3, 0, 16, 0, 0) X(3, 0, 4, 0, 0) X(4, 0, 16, 0, 0) X(4, 0, 4, 0, 0) X(5, 0, 16, 0, 0) X(5, 0, 4, 0, 0)                       \
    X(6, 0, 16, 0, 0) X(6, 0, 4, 0, 0) X(8, 0, 16, 0, 0) X(8, 0, 4, 0, 0) X(9, 0, 16, 0, 0) X(9, 0, 4, 0, 0)
#define MG_RENDER_GROUP_K(X) /* the chunk raster at tile 8 for even views; the gather raster with 'prestige' agents at tile 5 */ \
    X(4, 8, 16, 0, 0) X(4, 8, 4, 0, 0) X(6, 8, 16, 0, 0) X(6, 8, 4, 0, 0) X(8, 8, 16, 0, 0) X(8, 8, 4, 0, 0)                       \
    X(7, 5, 12, 9, 2) X(7, 5, 8, 9, 2) X(7, 5, 4, 9, 2)
#define MG_RENDER_GROUP_J(X) /* ... views 3, 4, 5, 6, 8, 9 at 5-pixel tiles */                                                       \
    X(3, 5, 16, 0, 2) X(3, 5, 4, 0, 2) X(5, 5, 16, 0, 2) X(5, 5, 4, 0, 2) X(9, 5, 16, 0, 2) X(9, 5, 4, 0, 2)                       \
    X(4, 5, 16, 0, 2) X(4, 5, 4, 0, 2) X(6, 5, 16, 0, 2) X(6, 5, 4, 0, 2) X(8, 5, 16, 0, 2) X(8, 5, 4, 0, 2)
#define MG_RENDER_GROUP_I(X) /* ... 11- and 12-pixel tiles; 11 with 'prestige' agents (examples/human_player.py) */        \
    X(7, 11, 16, 0, 2) X(7, 11, 4, 0, 2) X(7, 12, 16, 0, 2) X(7, 12, 4, 0, 2) X(7, 11, 12, 9, 2) X(7, 11, 8, 9, 2) X(7, 11, 4, 9, 2)
#if defined(MG_AB_VARIANTS)
#define MG_RENDER_GROUP_V(X) /* measurement variants (tools/ab_render.py) */                                               \
    X(7, 8, 16, 2, 0) X(7, 8, 4, 2, 0) X(7, 8, 16, 3, 0) X(7, 8, 4, 3, 0) X(7, 8, 16, 4, 0) X(7, 8, 4, 4, 0)                     \
    X(7, 8, 16, 6, 0) X(7, 8, 4, 6, 0) X(7, 8, 16, 11, 0) X(7, 8, 4, 11, 0) X(7, 8, 16, 0, 1) X(7, 8, 4, 0, 1)
#else
#define MG_RENDER_GROUP_V(X)
#endif
#define MG_RENDER_GROUP_N(X) /* mg_step_render_encode (V + 16): the BASELINE configs' shapes, the default tile, any view at tile 8 */ \
    X(7, 8, 16, 16, 0) X(7, 8, 4, 16, 0) X(9, 8, 16, 16, 0) X(9, 8, 4, 16, 0) X(0, 8, 8, 16, 0) X(0, 8, 4, 16, 0)                       \
    X(7, 5, 16, 16, 2) X(7, 5, 4, 16, 2)
#define MG_RENDER_GROUP_P(X) /* mg_step_render_ep (V + 32): the shapes of group N */                                       \
    X(7, 8, 16, 32, 0) X(7, 8, 4, 32, 0) X(9, 8, 16, 32, 0) X(9, 8, 4, 32, 0) X(0, 8, 8, 32, 0) X(0, 8, 4, 32, 0)                       \
    X(7, 5, 16, 32, 2) X(7, 5, 4, 32, 2)
// mg_step_render_delta (V + 64): NOT part of MG_RENDER_ALL — the launcher looks a kDelta pick up in this list (inst group Q)
#define MG_RENDER_DELTA(X) X(7, 8, 16, 64, 0) X(7, 8, 4, 64, 0)
#define MG_RENDER_GROUP_Q(X) MG_RENDER_DELTA(X)
// mg_step_render_delta_ex (V + 64 + 16: with the encode, + 32: with the episode outputs, + 48: with both): not part of MG_RENDER_ALL
// either — the launcher looks a kDeltaEncode / kDeltaEpisode / kDeltaEncodeEpisode pick up in this list (inst group R)
#define MG_RENDER_DELTA_X(X)                                                                                               \
    X(7, 8, 16, 96, 0) X(7, 8, 4, 96, 0) X(7, 8, 16, 80, 0) X(7, 8, 4, 80, 0) X(7, 8, 16, 112, 0) X(7, 8, 4, 112, 0)
#define MG_RENDER_GROUP_R(X) MG_RENDER_DELTA_X(X)
// every instantiation of this build (the headline shape's group first: the launcher's lookup walks the list in order)
#if defined(MG_DEV_ONLY)      // development: compile ONE instantiation (register / ISA checks without the other hundred), e.g. -DMG_DEV_ONLY="7,5,16,0,0"
#define MG_RENDER_ONE(X, ...) X(__VA_ARGS__)
#define MG_RENDER_ALL(X) MG_RENDER_ONE(X, MG_DEV_ONLY)
#else
#define MG_RENDER_ALL(X)                                                                                                    \
    MG_RENDER_GROUP_A(X) MG_RENDER_GROUP_N(X) MG_RENDER_GROUP_P(X) MG_RENDER_GROUP_B(X) MG_RENDER_GROUP_C(X)               \
    MG_RENDER_GROUP_D(X) MG_RENDER_GROUP_E(X) MG_RENDER_GROUP_G(X) MG_RENDER_GROUP_H(X) MG_RENDER_GROUP_I(X)               \
    MG_RENDER_GROUP_J(X) MG_RENDER_GROUP_K(X) MG_RENDER_GROUP_L(X) MG_RENDER_GROUP_M(X) MG_RENDER_GROUP_V(X)
#endif
