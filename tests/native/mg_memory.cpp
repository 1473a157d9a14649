// TEST INFRASTRUCTURE — the bodies of mg_memory_update (marlgrid_amd/csrc/mg_explore_core.h with mg_view_triple.h, mg_occlude.h and
// mg_core.h's view map) built for the host with g++ and called through ctypes (tests/native/hostemu_memory.py):
// explore_kernel<VS_, true> of mg_explore.hip emulated over plain arrays, as tests/native/mg_explore.cpp emulates
// explore_kernel<VS_, false>.  Workgroups of `block` lanes in launch order, each phase run for every lane of the workgroup before
// the next begins (the kernel's barriers); the "LDS" is a heap block of explore_lds_bytes(.., mem = true) filled with a pattern.
// `rt`: the run-time-view instantiation also for the views that have a compile-time one.  tests/native/mg_memory_main.cpp
// includes this file under the sanitizers.
#include <stdlib.h>
#include <string.h>

#include "mg_explore_core.h"

namespace {

template <int VS_>
void mem_run_group(const MgConfig& cfg, const MgState& st, const uint8_t* mask, uint8_t* seen, int32_t* visits, int32_t* new_cells,
                   int32_t* visit_count, uint32_t* memory, int32_t* seen_step, const mg::ExploreLaunch& lc, int wave, uint8_t* smem,
                   long long blk) {
    using namespace mg;
    const int VS = VS_ ? VS_ : cfg.view_size, n = cfg.n_agents, nv = lc.nv, H = cfg.H, W = cfg.W, cells = W * H;
    const int off = cfg.view_offset;
    const ExploreScratch s = explore_scratch(smem, n, VS, lc, true);
    const long long p0 = blk * lc.PB;
    const int cnt = (int)((lc.pairs - p0) < lc.PB ? (lc.pairs - p0) : lc.PB);
    const long long b0 = p0 / nv;
    const int ne = (int)((p0 + cnt - 1) / nv - b0) + 1;
    // A
    for (int o = 0; o < 256; o++) {
        s.see[o] = explore_see_behind(cfg, o);
        s.tab[o] = view_triple_entry(cfg, o);
        s.hide[o] = view_hide_entry(cfg, o);
    }
    for (int i = 0; i < ne * n; i++) s.rec[i] = st.agents[(size_t)b0 * n + i];
    // B
    for (int t = 0; t < cnt; t++) {
        const long long p = p0 + t;
        const long long b = p / nv;
        const int v = (int)(p - b * nv);
        const int k = cfg.n_view ? (int)cfg.view_agent[v] : v;
        const int slot = (int)(b - b0);
        const bool selected = !mask || mask[b] != 0;
        explore_pair_map(s.rec[slot * n + k], k, slot, selected, selected && st.step_count[b] == 0, VS, off, &s.aff[2 * t], &s.aff[2 * t + 1]);
    }
    // C
    const int rows = cnt * VS;
    for (int it = 0; it < rows; it++) {
        const int t = it / VS, vb = it - t * VS;
        const uint32_t aff = s.aff[2 * t], w1 = s.aff[2 * t + 1];
        if (!(w1 & kExSelected)) continue;
        const uint8_t* g = st.grid + (size_t)(b0 + (w1 >> 16)) * cfg.cells_stride;
        s.trow[it] = explore_transparency_row(s.see, g, aff, vb, VS, W, H);
    }
    // Z
    for (int t = 0; t < cnt; t++) {
        const uint32_t w1 = s.aff[2 * t + 1];
        if (!(w1 & kExFresh)) continue;
        const size_t pl = explore_plane(cfg, b0 + (w1 >> 16), (int)(w1 & 0xFFu));
        for (int lane = 0; lane < wave; lane++) {
            explore_clear_planes(seen + pl, visits + pl, cells, lane, wave);
            explore_clear_memory(memory + pl, seen_step + pl, cells, lane, wave);
        }
    }
    // D
    for (int t = 0; t < cnt; t++) {
        const uint32_t w1 = s.aff[2 * t + 1];
        if (!(w1 & kExSelected)) continue;
        explore_visibility<VS_>((w1 & kExActive) != 0, cfg.see_through_walls != 0, VS, off, s.trow + t * VS, s.vis + t * VS);
    }
    // E
    for (int it = 0; it < rows; it++) {
        const int t = it / VS, vb = it - t * VS;
        const uint32_t aff = s.aff[2 * t], w1 = s.aff[2 * t + 1];
        if (!(w1 & kExSelected)) continue;
        const int slot = (int)(w1 >> 16);
        const size_t pl = explore_plane(cfg, b0 + slot, (int)(w1 & 0xFFu));
        s.trow[it] = (uint32_t)explore_remember_row(cfg, s.tab, s.hide, s.rec + slot * n, n, (int)(w1 & 0xFFu),
                                                    st.grid + (size_t)(b0 + slot) * cfg.cells_stride, st.step_count[b0 + slot],
                                                    seen + pl, memory + pl, seen_step + pl, aff, vb, s.vis[it], VS, W, H);
    }
    // F
    for (int t = 0; t < cnt; t++) {
        const uint32_t w1 = s.aff[2 * t + 1];
        if (!(w1 & kExSelected)) continue;
        const int slot = (int)(w1 >> 16), k = (int)(w1 & 0xFFu);
        int32_t sum = 0;
        for (int j = 0; j < VS; j++) sum += (int32_t)s.trow[t * VS + j];
        const size_t pl = explore_plane(cfg, b0 + slot, k);
        const size_t at = (size_t)(b0 + slot) * n + k;
        new_cells[at] = sum;
        visit_count[at] = explore_visit(visits + pl, s.rec[slot * n + k], W, H);
    }
}

}  // namespace

extern "C" {

// -> 0, or MG_E_ARG; *pairs_per_group: the launch's PB; *lds_bytes: the workgroup's scratch
int mem_update(const MgConfig* cfg, const MgState* st, const uint8_t* mask, uint8_t* seen, int32_t* visits, int32_t* new_cells,
               int32_t* visit_count, uint8_t* memory, int32_t* seen_step, int block, int wave, int rt, int* pairs_per_group,
               int* lds_bytes) {
    if (!cfg || !st || !seen || !visits || !new_cells || !visit_count || !memory || !seen_step) return MG_E_ARG;
    if (reinterpret_cast<uintptr_t>(memory) & 3u) return MG_E_ARG;
    if (block < 1 || wave < 1 || cfg->view_size < 1 || cfg->view_size > MG_MAX_VIEW) return MG_E_ARG;
    if (cfg->B <= 0) return 0;
    const mg::ExploreLaunch lc = mg::explore_launch(*cfg, block, true);
    if (pairs_per_group) *pairs_per_group = lc.PB;
    const int VS = cfg->view_size;
    const size_t bytes = mg::explore_lds_bytes(cfg->n_agents, VS, lc.PB, lc.nv, true);
    if (lds_bytes) *lds_bytes = (int)bytes;
    if (bytes > 64 * 1024) return MG_E_ARG;
    uint8_t* mem = static_cast<uint8_t*>(malloc(bytes));          // (exact size: the sanitized program sees a byte past it)
    if (!mem) return -1;
    uint32_t* words = reinterpret_cast<uint32_t*>(memory);
    const long long blocks = (lc.pairs + lc.PB - 1) / lc.PB;
    for (long long blk = 0; blk < blocks; blk++) {
        memset(mem, 0xA5, bytes);
#define MEM_RUN(V) mem_run_group<V>(*cfg, *st, mask, seen, visits, new_cells, visit_count, words, seen_step, lc, wave, mem, blk)
        if (!rt && VS == 7) MEM_RUN(7);
        else if (!rt && VS == 5) MEM_RUN(5);
        else if (!rt && VS == 9) MEM_RUN(9);
        else MEM_RUN(0);
#undef MEM_RUN
    }
    free(mem);
    return 0;
}

}  // extern "C"
