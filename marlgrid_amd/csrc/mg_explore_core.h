// mg_explore_core.h — the bodies of mg_explore_update (mg_explore.hip): per (env, viewer) PAIR, which world cells the
// observation just returned covered — inside the view AND visible, the vis_mask of gen_obs_grid (base.py:418-451) — and where
// the agent stood.  Semantics: include/marlgrid_hip.h.  Plain functions over pointers, one call per lane item, as
// mg_goal_core.h: the kernel hands them LDS and global memory, tests/native/mg_explore.cpp (g++) heap blocks and numpy arrays.
//
// The view's map to world cells is mg_core.h's view_map / view_world and the shadow cast mg_occlude.h's, as the encoded-views
// launch uses them.  A view map is injective, so the rows of one pair touch disjoint cells of the pair's planes, and two pairs
// never share a plane: plain byte and dword stores, no atomics.
//
// mg_memory_update (`mem`, the kernel's MEM_ = true) keeps two more planes per pair beside those: `memory`, one dword per cell
// — the triple the cell showed in the pair's most recent observation of it (view_cell_triple, mg_view_triple.h: what
// mg_encode_views writes at the view cell) with known = 1 in the top byte —, and `seen_step`, the env's step count at that
// observation (-1: never seen).  The bodies below that take them are added to the launch; the others are shared unchanged.
#pragma once
#include "mg_core.h"
#include "mg_occlude.h"
#include "mg_view_triple.h"

namespace mg {

// word 1 of a pair's map (word 0: view_map): viewer k | flags | env slot of the workgroup's run << 16
enum : uint32_t { kExActive = 1u << 8, kExFresh = 1u << 9, kExSelected = 1u << 10 };

// where the planes of (env b, agent k) start, in cells: B n W H passes 2^31 at a large batch of large grids
MG_HD size_t explore_plane(const MgConfig& cfg, long long b, int k) {
    return ((size_t)b * (size_t)cfg.n_agents + (size_t)k) * ((size_t)cfg.W * (size_t)cfg.H);
}

// the see_behind table of phase A: entry o of [256], None (0) transparent, ids past the table opaque
MG_HD uint8_t explore_see_behind(const MgConfig& cfg, int o) {
    if (o == 0) return 1;
    return (o < cfg.n_obj && (cfg.obj[o].flags & MG_OF_SEE_BEHIND)) ? 1 : 0;
}

// B. one pair: its view's affine map and its flags.  `fresh`: the env's step counter is 0 — mg_reset, the same-step reset
// inside step_run or the next-step reset call has just run (step_begin sets sc0 + 1 in every other call)
MG_HD void explore_pair_map(uint64_t rec, int k, int slot, bool selected, bool fresh, int VS, int off, uint32_t* w0, uint32_t* w1) {
    const int x = (int)rec_byte(rec, MG_AG_X), y = (int)rec_byte(rec, MG_AG_Y), dir = (int)rec_byte(rec, MG_AG_DIR);
    *w0 = view_map(x, y, dir, VS, off);
    *w1 = (uint32_t)k | ((rec_byte(rec, MG_AG_FLAGS) & MG_AF_ACTIVE) ? kExActive : 0u) | (fresh ? kExFresh : 0u) |
          (selected ? kExSelected : 0u) | ((uint32_t)slot << 16);
}

// the world cell of view cell (column va, row vb), x * H + y; -1 outside the grid
MG_HD int explore_world_cell(uint32_t aff, int va, int vb, int W, int H) {
    int wx, wy;
    view_world(aff, va, vb, &wx, &wy);
    return ((unsigned)wx < (unsigned)W && (unsigned)wy < (unsigned)H) ? wx * H + wy : -1;
}

// C. one view row: its transparency bits (opacity, base.py:103-106: the grid's own object; outside the grid: transparent)
MG_HD uint32_t explore_transparency_row(const uint8_t* see, const uint8_t* g, uint32_t aff, int vb, int VS, int W, int H) {
    uint32_t bits = 0;
    for (int va = 0; va < VS; va++) {
        const int c = explore_world_cell(aff, va, vb, W, H);
        if (see[c >= 0 ? g[c] : 0]) bits |= 1u << va;
    }
    return bits;
}

// D. one pair: the visibility rows (base.py:420-425: an inactive viewer sees nothing; see_through_walls: everything; else
// process_vis).  VS_: the compile-time view, 0 the run-time one (rows walked where they are); `vis` is not `trow`
template <int VS_>
MG_HD void explore_visibility(bool active, bool see_through_walls, int VS, int off, const uint32_t* trow, uint32_t* vis) {
    if (!active) { for (int j = 0; j < VS; j++) vis[j] = 0; }
    else if (see_through_walls) { for (int j = 0; j < VS; j++) vis[j] = (1u << VS) - 1u; }
    else if constexpr (VS_ == 0) occlude_rows_mem(VS, off, trow, vis);
    else {
        uint32_t m[VS_ ? VS_ : 1];
        occlude_rows<VS_>(VS, off, trow, m);
#pragma unroll
        for (int j = 0; j < VS_; j++) vis[j] = m[j];
    }
}

// a fresh pair's planes cleared by `lanes` lanes: the visits words one by one, the seen bytes as dwords between the plane's
// first and last partial dword (those byte by byte: the neighbouring planes own the other bytes)
MG_HD void explore_clear_planes(uint8_t* seen_p, int32_t* visits_p, int cells, int lane, int lanes) {
    for (int i = lane; i < cells; i += lanes) visits_p[i] = 0;
    const int head = (int)((4u - (unsigned)(reinterpret_cast<uintptr_t>(seen_p) & 3u)) & 3u);
    if (cells <= head) {
        for (int i = lane; i < cells; i += lanes) seen_p[i] = 0;
        return;
    }
    const int words = (cells - head) / 4, tail = head + 4 * words;
    for (int i = lane; i < head; i += lanes) seen_p[i] = 0;
    uint32_t* w = reinterpret_cast<uint32_t*>(seen_p + head);
    for (int i = lane; i < words; i += lanes) w[i] = 0u;
    for (int i = tail + lane; i < cells; i += lanes) seen_p[i] = 0;
}

// E. one view row: its visible in-grid cells marked; -> how many of them were not seen before
MG_HD int explore_mark_row(uint8_t* seen_p, uint32_t aff, int vb, uint32_t vis, int VS, int W, int H) {
    int fresh = 0;
    for (int va = 0; va < VS; va++) {
        const int c = explore_world_cell(aff, va, vb, W, H);
        if (((vis >> va) & 1u) && c >= 0 && seen_p[c] == 0) {
            seen_p[c] = 1;
            fresh++;
        }
    }
    return fresh;
}

// Z, with the memory: a fresh pair's `memory` plane cleared to 0 (never seen: (0, 0, 0, 0)) and its `seen_step` plane to -1.
// One aligned dword per cell in both: plain dword stores, no alignment cases
MG_HD void explore_clear_memory(uint32_t* memory_p, int32_t* step_p, int cells, int lane, int lanes) {
    for (int i = lane; i < cells; i += lanes) memory_p[i] = 0u;
    for (int i = lane; i < cells; i += lanes) step_p[i] = -1;
}

// E, with the memory: one view row, as explore_mark_row, and each visible in-grid cell remembered: its triple as viewer k's
// observation shows it | known << 24 in one dword store, the env's step count `sc` in another.  tab / hide: the tables of
// mg_view_triple.h; rec: the n records of the env; g: its grid
MG_HD int explore_remember_row(const MgConfig& cfg, const uint32_t* tab, const uint32_t* hide, const uint64_t* rec, int n, int k,
                               const uint8_t* g, int32_t sc, uint8_t* seen_p, uint32_t* memory_p, int32_t* step_p, uint32_t aff,
                               int vb, uint32_t vis, int VS, int W, int H) {
    int fresh = 0;
    for (int va = 0; va < VS; va++) {
        int wx, wy;
        view_world(aff, va, vb, &wx, &wy);
        if (!((vis >> va) & 1u) || (unsigned)wx >= (unsigned)W || (unsigned)wy >= (unsigned)H) continue;
        const int c = wx * H + wy;
        memory_p[c] = view_cell_triple(cfg, tab, hide, rec, n, k, g[c], wx, wy) | (1u << 24);
        step_p[c] = sc;
        if (seen_p[c] == 0) {
            seen_p[c] = 1;
            fresh++;
        }
    }
    return fresh;
}

// F. one pair: the agent's own cell counted -> visits there after the increment; 0 for an agent in no cell
MG_HD int32_t explore_visit(int32_t* visits_p, uint64_t rec, int W, int H) {
    if (!(rec_byte(rec, MG_AG_FLAGS) & MG_AF_PLACED)) return 0;
    const int x = (int)rec_byte(rec, MG_AG_X), y = (int)rec_byte(rec, MG_AG_Y);
    if (x >= W || y >= H) return 0;
    const int32_t v = visits_p[x * H + y] + 1;
    visits_p[x * H + y] = v;
    return v;
}

// ---- the workgroup's LDS (the host harness lays its heap block out the same way) --------------------------------------------
struct ExploreLaunch {
    int32_t PB;         // pairs per workgroup
    int32_t nv;         // viewers per env (n_view, or n_agents)
    int32_t env_cap;    // envs whose records one workgroup stages: (PB - 1) / nv + 2
    long long pairs;    // B * nv
};
struct ExploreScratch {
    uint8_t* see;       // [256]
    uint64_t* rec;      // [env_cap][n]
    uint32_t* aff;      // [PB][2]
    uint32_t* trow;     // [PB][VS] transparency rows; after phase D the rows' counts of new cells
    uint32_t* vis;      // [PB][VS]
    uint32_t* tab;      // mem: [256] the triple table, and behind it
    uint32_t* hide;     // mem: [256] the hide table (kEvTab bytes together); both NULL without the memory
};
inline size_t explore_lds_bytes(int n_agents, int VS, int PB, int nv, bool mem = false) {
    const int env_cap = (PB - 1) / nv + 2;
    return 256 + (size_t)env_cap * n_agents * 8 + (size_t)PB * 8 + (size_t)PB * VS * 4 * 2 + (mem ? (size_t)kEvTab : 0);
}
MG_HD ExploreScratch explore_scratch(uint8_t* base, int n_agents, int VS, const ExploreLaunch& lc, bool mem = false) {
    ExploreScratch s;
    s.see = base;
    s.rec = reinterpret_cast<uint64_t*>(base + 256);
    s.aff = reinterpret_cast<uint32_t*>(s.rec + (size_t)lc.env_cap * n_agents);
    s.trow = s.aff + 2 * (size_t)lc.PB;
    s.vis = s.trow + (size_t)lc.PB * VS;
    s.tab = mem ? s.vis + (size_t)lc.PB * VS : nullptr;
    s.hide = mem ? s.tab + 256 : nullptr;
    return s;
}
// pairs per workgroup: one lane per pair where the scratch stays within 48 KiB (several workgroups per CU), else halved
inline ExploreLaunch explore_launch(const MgConfig& cfg, int block, bool mem = false) {
    ExploreLaunch lc;
    lc.nv = cfg.n_view ? cfg.n_view : cfg.n_agents;
    lc.pairs = (long long)cfg.B * lc.nv;
    int PB = block;
    while (PB > 1 && explore_lds_bytes(cfg.n_agents, cfg.view_size, PB, lc.nv, mem) > 48 * 1024) PB /= 2;
    lc.PB = PB;
    lc.env_cap = (PB - 1) / lc.nv + 2;
    return lc;
}

}  // namespace mg
