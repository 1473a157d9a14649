// mg_explore.hip — mg_explore_update, and mg_memory_update (below): the exploration maps of every (env, viewer) pair brought up to date with the observation
// the caller has just been given: seen[b][k][x][y] |= cell (x, y) was in agent k's view and visible, visits[b][k] at the agent's
// own cell += 1, and the two per-step scalars (cells seen for the first time; visits of the own cell).  Semantics:
// include/marlgrid_hip.h; bodies: mg_explore_core.h.
//
// Roofline: per pair the launch reads the pair's record and ~vs^2 grid bytes (in L2: the step has just written them) and
// touches ~vs^2 bytes of a W H-byte plane plus one visits word — less than the encoded-views launch writes (3 vs^2 bytes); a
// fresh env adds 5 W H bytes of clearing per agent.  Bound by the view chain (map, transparency, shadow cast), as that launch.
//
// Mapping: encode_views_kernel's.  A workgroup of kBlock threads takes PB consecutive (env, viewer) pairs:
//   A. the see_behind bit of every object id and the agent records of the run's envs go to LDS;
//   B. one lane per pair: the view's affine map, the viewer, and whether its env is selected / has just begun an episode;
//   C. one lane per view ROW: the row's transparency bits;
//   Z. one WAVE per pair of a fresh env: the pair's two planes are zeroed (dword stores);
//   D. one lane per pair: the shadow cast (mg_occlude.h) as row bit-masks;
//      -- barrier: the zeroes of Z are in place before any lane of the workgroup reads or marks a plane --
//   E. one lane per view row: the visible in-grid cells whose `seen` byte is 0 get a 1 and are counted;
//   F. one lane per pair: the rows' counts summed -> new_cells; visits at the agent's cell incremented -> visit_count.
// Rows of one pair touch disjoint cells and two pairs never share a plane: byte and dword vector stores, no atomics.  The
// grid is read where it lives (any size up to 255 x 255); every plane offset is 64-bit.  Compile-time views 7 / 5 / 9, one
// run-time instantiation for the rest (up to 31).
//
// mg_memory_update is the same launch with MEM_ = true: the view chain runs ONCE for the exploration maps and the memory.
//   A also stages the object triples and the hide table (mg_view_triple.h, kEvTab = 2 KiB more LDS);
//   Z also clears the pair's `memory` plane (dwords of 0) and its `seen_step` plane (dwords of -1);
//   E also stores, per visible in-grid cell, the dword (type, colour, state, known = 1) — the triple mg_encode_views writes at
//     that view cell — and the env's step count: two scattered dword stores per cell beside the `seen` byte, 8 W H more bytes
//     of clearing per agent of a fresh env.  Write-only planes, one aligned dword per cell, 64-bit plane offsets.
// MEM_ = false is the launch it was: the additions are compiled out.
#include "mg_device.h"
#include "mg_explore_core.h"
#include "mg_launch.h"

namespace mg {

// the two planes of mg_memory_update (MEM_ = true; not read otherwise)
struct ExploreMem {
    uint32_t* memory;      // [B][n][W][H] type | colour << 8 | state << 16 | known << 24
    int32_t* seen_step;    // [B][n][W][H]
};

template <int VS_, bool MEM_>
__global__ __launch_bounds__(kBlock) void explore_kernel(MgConfig cfg, const uint8_t* __restrict__ grid,
                                                         const uint64_t* __restrict__ agents, const int32_t* __restrict__ step_count,
                                                         const uint8_t* __restrict__ mask, uint8_t* seen, int32_t* visits,
                                                         int32_t* __restrict__ new_cells, int32_t* __restrict__ visit_count,
                                                         ExploreLaunch lc, ExploreMem mm) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int tid = threadIdx.x;
    const int VS = VS_ ? VS_ : cfg.view_size, n = cfg.n_agents, nv = lc.nv, H = cfg.H, W = cfg.W, cells = W * H;
    const int off = cfg.view_offset;
    const ExploreScratch s = explore_scratch(smem, n, VS, lc, MEM_);

    const long long p0 = (long long)blockIdx.x * lc.PB;
    const int cnt = (int)min((long long)lc.PB, lc.pairs - p0);
    const long long b0 = p0 / nv;
    const int ne = (int)((p0 + cnt - 1) / nv - b0) + 1;

    // A. table and records
    for (int o = tid; o < 256; o += kBlock) s.see[o] = explore_see_behind(cfg, o);
    if constexpr (MEM_) {
        for (int o = tid; o < 256; o += kBlock) {
            s.tab[o] = view_triple_entry(cfg, o);
            s.hide[o] = view_hide_entry(cfg, o);
        }
    }
    for (int i = tid; i < ne * n; i += kBlock) s.rec[i] = agents[(size_t)b0 * n + i];
    __syncthreads();

    // B. one lane per pair
    for (int t = tid; t < cnt; t += kBlock) {
        const long long p = p0 + t;
        const long long b = p / nv;
        const int v = (int)(p - b * nv);
        const int k = cfg.n_view ? (int)cfg.view_agent[v] : v;
        const int slot = (int)(b - b0);
        const bool selected = !mask || mask[b] != 0;
        explore_pair_map(s.rec[slot * n + k], k, slot, selected, selected && step_count[b] == 0, VS, off, &s.aff[2 * t], &s.aff[2 * t + 1]);
    }
    __syncthreads();

    // C. transparency rows, one lane per view row
    const int rows = cnt * VS;
    for (int it = tid; it < rows; it += kBlock) {
        const int t = it / VS, vb = it - t * VS;
        const uint32_t aff = s.aff[2 * t], w1 = s.aff[2 * t + 1];
        if (!(w1 & kExSelected)) continue;
        const uint8_t* g = grid + (size_t)(b0 + (w1 >> 16)) * cfg.cells_stride;
        s.trow[it] = explore_transparency_row(s.see, g, aff, vb, VS, W, H);
    }
    // Z. the planes of the pairs whose env has just begun an episode, one wave per pair
    for (int t = tid / kWave; t < cnt; t += kBlock / kWave) {
        const uint32_t w1 = s.aff[2 * t + 1];
        if (!(w1 & kExFresh)) continue;
        const size_t pl = explore_plane(cfg, b0 + (w1 >> 16), (int)(w1 & 0xFFu));
        explore_clear_planes(seen + pl, visits + pl, cells, tid & (kWave - 1), kWave);
        if constexpr (MEM_) explore_clear_memory(mm.memory + pl, mm.seen_step + pl, cells, tid & (kWave - 1), kWave);
    }
    __syncthreads();

    // D. visibility, one lane per pair
    for (int t = tid; t < cnt; t += kBlock) {
        const uint32_t w1 = s.aff[2 * t + 1];
        if (!(w1 & kExSelected)) continue;
        explore_visibility<VS_>((w1 & kExActive) != 0, cfg.see_through_walls != 0, VS, off, s.trow + t * VS, s.vis + t * VS);
    }
    __syncthreads();      // (also: the zeroes of Z, written by this workgroup to global memory, are read — and with the
                          // memory overwritten — below)

    // E. marks, one lane per view row; the row's count of new cells takes its transparency word's place
    for (int it = tid; it < rows; it += kBlock) {
        const int t = it / VS, vb = it - t * VS;
        const uint32_t aff = s.aff[2 * t], w1 = s.aff[2 * t + 1];
        if (!(w1 & kExSelected)) continue;
        const size_t pl = explore_plane(cfg, b0 + (w1 >> 16), (int)(w1 & 0xFFu));
        if constexpr (MEM_) {
            const int slot = (int)(w1 >> 16);
            s.trow[it] = (uint32_t)explore_remember_row(cfg, s.tab, s.hide, s.rec + slot * n, n, (int)(w1 & 0xFFu),
                                                        grid + (size_t)(b0 + slot) * cfg.cells_stride, step_count[b0 + slot],
                                                        seen + pl, mm.memory + pl, mm.seen_step + pl, aff, vb, s.vis[it], VS, W, H);
        } else {
            s.trow[it] = (uint32_t)explore_mark_row(seen + pl, aff, vb, s.vis[it], VS, W, H);
        }
    }
    __syncthreads();

    // F. one lane per pair: the scalars and the visit
    for (int t = tid; t < cnt; t += kBlock) {
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

// memory / seen_step: both NULL (mg_explore_update) or both set (mg_memory_update)
static hipError_t launch_explore(const MgConfig& cfg, const MgState& st, const uint8_t* mask, uint8_t* seen, int32_t* visits,
                                 int32_t* new_cells, int32_t* visit_count, uint32_t* memory, int32_t* seen_step, hipStream_t s) {
    if (cfg.B <= 0) return hipSuccess;
    const int VS = cfg.view_size;
    const bool mem = memory != nullptr;
    const ExploreLaunch lc = explore_launch(cfg, kBlock, mem);
    const size_t lds = explore_lds_bytes(cfg.n_agents, VS, lc.PB, lc.nv, mem);
    if (lds > 64 * 1024) return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)((lc.pairs + lc.PB - 1) / lc.PB);
    // the instantiation: the first of the compile-time view sizes that is this one, else the run-time view (0)
    void (*kernel)(MgConfig, const uint8_t*, const uint64_t*, const int32_t*, const uint8_t*, uint8_t*, int32_t*, int32_t*, int32_t*,
                   ExploreLaunch, ExploreMem) = nullptr;
#define MG_EX_VIEWS(X) X(7) X(5) X(9) X(0)
#define MG_EX_PICK(V) if (!kernel && (V == 0 || VS == V)) kernel = mem ? explore_kernel<V, true> : explore_kernel<V, false>;
    MG_EX_VIEWS(MG_EX_PICK)
#undef MG_EX_PICK
#undef MG_EX_VIEWS
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kBlock), lds, s, cfg, st.grid, st.agents, st.step_count, mask, seen, visits, new_cells,
                       visit_count, lc, ExploreMem{memory, seen_step});
    return hipGetLastError();
}

hipError_t launch_explore_update(const MgConfig& cfg, const MgState& st, const uint8_t* mask, uint8_t* seen, int32_t* visits,
                                 int32_t* new_cells, int32_t* visit_count, hipStream_t s) {
    return launch_explore(cfg, st, mask, seen, visits, new_cells, visit_count, nullptr, nullptr, s);
}

hipError_t launch_memory_update(const MgConfig& cfg, const MgState& st, const uint8_t* mask, uint8_t* seen, int32_t* visits,
                                int32_t* new_cells, int32_t* visit_count, uint8_t* memory, int32_t* seen_step, hipStream_t s) {
    if (!memory || !seen_step || (reinterpret_cast<uintptr_t>(memory) & 3u)) return hipErrorInvalidValue;
    return launch_explore(cfg, st, mask, seen, visits, new_cells, visit_count, reinterpret_cast<uint32_t*>(memory), seen_step, s);
}

}  // namespace mg
