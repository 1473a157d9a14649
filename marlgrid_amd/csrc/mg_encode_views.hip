// mg_encode_views.hip — every agent's encoded view: MultiGridEnv.gen_obs_grid(agent) (base.py:418-451: crop, rotate, shadow
// cast, hide_item_types) followed by MultiGrid.encode(vis_mask) (base.py:196-214).  out: uint8 [B][nv][vs][vs][3], index
// [i][j] as encode returns it (i = view column, j = view row), any alignment.
//
// Roofline: the output is 3 vs^2 bytes per agent-step (147 at view 7) against the raster's 3 (vs ts)^2 (9 408 at view 7,
// tile 8): the launch is bound by the view chain, not by HBM.
//
// Mapping: a workgroup of kBlock threads takes PB consecutive (env, viewer) PAIRS — a contiguous run of output bytes:
//   A. the (type, colour, state) triple of every object id in one dword (WorldObj.encode, objects.py:90-99) with its
//      see_behind bit, the hide_item_types table and the agent records of the run's envs go to LDS;
//   B. one lane per pair: the view's affine map (origin, swap, signs: as the raster's phase 2b) and its viewer;
//   C. one lane per view ROW: the row's transparency bits (opacity, base.py:103-106: the grid's own object);
//   D. one lane per pair: the shadow cast (agents.py:290-343) as row bit-masks (mg_occlude.h);
//   E. one lane per view row: each visible cell's triple — the cell object as `grid.get` returns it after hide_item_types —
//      written into the run's output image in LDS (invisible, empty and out-of-grid cells: 0, 0, 0);
//   F. the run leaves as aligned 16-byte vector stores, its first and last partial chunks byte by byte (neighbouring runs
//      write the other bytes of those chunks).
// The grid is read where it lives (one env's cells are a few hundred bytes in L2 right after the step wrote them): no limit
// on the grid size.  Compile-time view sizes 7 (the default), 5 and 9; one run-time-view instantiation for every other size.
#include "mg_device.h"
#include "mg_launch.h"
#include "mg_occlude.h"
#include "mg_view_triple.h"

namespace mg {

struct EncViewsLaunch {
    int32_t PB;         // pairs per workgroup
    int32_t nv;         // viewers per env (n_view, or n_agents)
    int32_t env_cap;    // envs whose records one workgroup stages: (PB - 1) / nv + 2
    int32_t stage_off;  // LDS byte offset of the run's output image (16-aligned)
    long long pairs;    // B * nv
};

// mg_step_encode_views in ONE launch (STEP_ = true): the workgroup first steps its own envs — PB / nv whole envs, one lane
// per env, mg_core.h's step_load / step_run on [item][lane] LDS columns as step_kernel runs them, auto-reset included — and
// then encodes their views from the state it has just written (the same workgroup: visible after the barrier)
struct EncViewsStep {
    MgState st;
    StepArgs a;
};

template <int VS_, bool STEP_>
__global__ __launch_bounds__(kBlock) void encode_views_kernel(MgConfig cfg, const uint8_t* __restrict__ grid,
                                                              const uint64_t* __restrict__ agents,
                                                              uint8_t* __restrict__ out, EncViewsLaunch lc, EncViewsStep fs) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int tid = threadIdx.x;
    if constexpr (STEP_) {
        // 0. the step of envs b0 .. b0 + E - 1 (E = PB / nv), one lane each; its LDS is reused by the phases below
        const int E = lc.PB / lc.nv, n = cfg.n_agents;
        StepScratch sc = lane_step_scratch(smem, n, E, tid);             // (step_kernel's layout with S = E)
        if (fs.a.has_ep) { sc.ep = &fs.a.ep; sc.ep_rewards = fs.a.rewards; }
        const int b = blockIdx.x * E + tid;
        const bool live = tid < E && b < cfg.B;
        const LaneStepLayout l = lane_step_layout(n, E);
        stage_obj_tables(cfg, reinterpret_cast<MgObjDesc*>(smem + l.obj), smem + l.oflags, tid, kBlock);
        StepEnv env{0, 0};
        __syncthreads();
        if (live) env = step_load(cfg, fs.st, fs.a.actions, fs.a.action_bytes, b, sc);
        __syncthreads();
        if (live) step_run(cfg, fs.st, fs.a.prog, fs.a.has_prog != 0, fs.a.rewards, b, env, sc, fs.st.grid + (size_t)b * cfg.cells_stride);
        __syncthreads();      // (the envs' new grids and records, written to global memory above, are read below)
    }
    const int VS = VS_ ? VS_ : cfg.view_size, VV = VS * VS, n = cfg.n_agents, nv = lc.nv, H = cfg.H, W = cfg.W;
    const int off = cfg.view_offset;
    uint32_t* s_tab = reinterpret_cast<uint32_t*>(smem);                       // [256] type | colour << 8 | state << 16 | see << 24
    uint32_t* s_hide = s_tab + 256;                                            // [256] bit k: agent k hides this object id
    uint64_t* s_rec = reinterpret_cast<uint64_t*>(smem + kEvTab);              // [env_cap][n]
    uint2* s_aff = reinterpret_cast<uint2*>(s_rec + (size_t)lc.env_cap * n);   // [PB]
    uint32_t* s_trow = reinterpret_cast<uint32_t*>(s_aff + lc.PB);             // [PB][VS] transparency rows
    uint32_t* s_vis = s_trow + (size_t)lc.PB * VS;                             // [PB][VS] visibility rows
    uint8_t* s_img = smem + lc.stage_off;                                      // the run's output bytes, from its 16-byte chunk start

    const long long p0 = (long long)blockIdx.x * lc.PB;
    const int cnt = (int)min((long long)lc.PB, lc.pairs - p0);
    const long long b0 = p0 / nv;
    const int ne = (int)((p0 + cnt - 1) / nv - b0) + 1;

    // A. tables and records
    for (int o = tid; o < 256; o += kBlock) {      // (mg_view_triple.h)
        s_tab[o] = view_triple_entry(cfg, o);
        s_hide[o] = view_hide_entry(cfg, o);
    }
    for (int i = tid; i < ne * n; i += kBlock) s_rec[i] = agents[(size_t)b0 * n + i];
    __syncthreads();

    // B. one lane per pair: word 0 the view's map of (column va, row vb) to world cells (view_map, mg_core.h);
    //    word 1: viewer k | active << 8 | env slot << 16
    for (int t = tid; t < cnt; t += kBlock) {
        const long long p = p0 + t;
        const int b = (int)(p / nv), v = (int)(p - (long long)b * nv);
        const int k = cfg.n_view ? (int)cfg.view_agent[v] : v;
        const int slot = (int)(b - b0);
        const uint64_t r = s_rec[slot * n + k];
        const int x = (int)rec_byte(r, MG_AG_X), y = (int)rec_byte(r, MG_AG_Y), dir = (int)rec_byte(r, MG_AG_DIR);
        const uint32_t active = (rec_byte(r, MG_AG_FLAGS) & MG_AF_ACTIVE) ? 1u : 0u;
        s_aff[t] = make_uint2(view_map(x, y, dir, VS, off), (uint32_t)k | (active << 8) | ((uint32_t)slot << 16));
    }
    __syncthreads();

    // the world cell of view cell (va, vb) of pair t, -1 outside the grid
    auto world_cell = [&](const uint2 aff, const int va, const int vb, int& wx, int& wy) -> int {
        view_world(aff.x, va, vb, &wx, &wy);
        return ((unsigned)wx < (unsigned)W && (unsigned)wy < (unsigned)H) ? wx * H + wy : -1;
    };

    // C. transparency rows, one lane per view row
    const int rows = cnt * VS;
    for (int it = tid; it < rows; it += kBlock) {
        const int t = it / VS, vb = it - t * VS;
        const uint2 aff = s_aff[t];
        const long long b = b0 + (aff.y >> 16);
        const uint8_t* g = grid + (size_t)b * cfg.cells_stride;
        uint32_t bits = 0;
        for (int va = 0; va < VS; va++) {      // (unrolled where VS is a compile-time constant)
            int wx, wy;
            const int c = world_cell(aff, va, vb, wx, wy);
            const uint32_t base = c >= 0 ? g[c] : 0u;
            if (s_tab[base] >> 24) bits |= 1u << va;
        }
        s_trow[it] = bits;
    }
    __syncthreads();

    // D. visibility, one lane per pair (base.py:420-425: an inactive viewer sees nothing; agents.py:294-295)
    for (int t = tid; t < cnt; t += kBlock) {
        const uint2 aff = s_aff[t];
        uint32_t* vis = s_vis + t * VS;
        if (!((aff.y >> 8) & 1u)) { for (int j = 0; j < VS; j++) vis[j] = 0; }
        else if (cfg.see_through_walls) { for (int j = 0; j < VS; j++) vis[j] = (1u << VS) - 1u; }
        else if constexpr (VS_ == 0) occlude_rows_mem(VS, off, s_trow + t * VS, vis);   // (run-time view: the rows stay in LDS)
        else {
            uint32_t m[VS_ ? VS_ : 1];
            occlude_rows<VS_>(VS, off, s_trow + t * VS, m);
#pragma unroll
            for (int j = 0; j < VS_; j++) vis[j] = m[j];
        }
    }
    __syncthreads();

    // E. the triples, one lane per view row: each visible in-grid cell's occupant as grid.get returns it after
    //    hide_item_types (view_cell_triple, mg_view_triple.h)
    const int ph = (int)((reinterpret_cast<uintptr_t>(out) + (size_t)p0 * 3 * VV) & 15);
    for (int it = tid; it < rows; it += kBlock) {
        const int t = it / VS, vb = it - t * VS;
        const uint2 aff = s_aff[t];
        const int slot = (int)(aff.y >> 16), k = (int)(aff.y & 0xFFu);
        const uint8_t* g = grid + (size_t)(b0 + slot) * cfg.cells_stride;
        const uint64_t* rec = s_rec + slot * n;
        const uint32_t vis = s_vis[t * VS + vb];
        uint8_t* img = s_img + ph + (size_t)t * 3 * VV + 3 * vb;
        for (int va = 0; va < VS; va++) {      // (unrolled where VS is a compile-time constant)
            uint32_t trip = 0;
            int wx, wy;
            const int c = world_cell(aff, va, vb, wx, wy);
            if (((vis >> va) & 1u) && c >= 0) trip = view_cell_triple(cfg, s_tab, s_hide, rec, n, k, g[c], wx, wy);
            uint8_t* o = img + (size_t)va * 3 * VS;
            o[0] = (uint8_t)trip;
            o[1] = (uint8_t)(trip >> 8);
            o[2] = (uint8_t)(trip >> 16);
        }
    }
    __syncthreads();

    // F. the run [p0 * 3 VV, (p0 + cnt) * 3 VV) of `out`: s_img byte i is out byte (chunk start + i)
    typedef struct { uint32_t v[4]; } __attribute__((aligned(16))) q16;
    const long long o0 = p0 * 3 * VV;
    const int nbytes = cnt * 3 * VV;
    uint8_t* base_out = out + o0 - ph;                                         // 16-byte aligned
    const int nq = (ph + nbytes + 15) / 16;
    for (int q = tid; q < nq; q += kBlock) {
        const int lo = 16 * q, hi = lo + 16;
        if (lo >= ph && hi <= ph + nbytes) {
            *reinterpret_cast<q16*>(base_out + lo) = *reinterpret_cast<const q16*>(s_img + lo);
        } else {
            for (int i = max(lo, ph); i < min(hi, ph + nbytes); i++) base_out[i] = s_img[i];
        }
    }
}

// LDS of a workgroup for PB pairs
static size_t encode_views_lds(const MgConfig& cfg, int PB, int nv, int* env_cap, int* stage_off) {
    const int VS = cfg.view_size;
    *env_cap = (PB - 1) / nv + 2;
    size_t b = kEvTab + (size_t)*env_cap * cfg.n_agents * 8 + (size_t)PB * 8 + (size_t)PB * VS * 4 * 2;
    b = (b + 15) & ~(size_t)15;
    *stage_off = (int)b;
    return b + 16 + (size_t)PB * 3 * VS * VS + 16;
}

// fs == NULL: the views of the current state.  fs: step first, in the same launch (whole envs per workgroup); returns
// hipErrorNotSupported — nothing launched — when a workgroup of whole envs does not fit 64 KiB of LDS (the caller then runs
// mg_step and the views launch)
hipError_t launch_encode_views(const MgConfig& cfg, const MgState& st, uint8_t* out, hipStream_t s, const EncViewsStep* fs) {
    if (cfg.B <= 0) return hipSuccess;
    const int VS = cfg.view_size, nv = cfg.n_view ? cfg.n_view : cfg.n_agents;
    EncViewsLaunch lc;
    lc.nv = nv;
    lc.pairs = (long long)cfg.B * nv;
    // pairs per workgroup: as many as keep the run's output image and the staged records within 48 KiB (several workgroups
    // per CU), at most one lane per pair; with the step, whole envs (a multiple of nv) and the step's scratch within the same LDS
    int PB = kBlock;
    size_t lds = 0;
    for (;; PB /= 2) {
        int pb = PB;
        if (fs) pb = PB / nv * nv;
        if (fs && pb == 0) return hipErrorNotSupported;
        lds = encode_views_lds(cfg, pb, nv, &lc.env_cap, &lc.stage_off);
        if (fs) lds = std::max(lds, lane_step_bytes(cfg.n_agents, pb / nv));
        lc.PB = pb;
        if (lds <= 48 * 1024 || PB == 1) break;
    }
    if (lds > 64 * 1024) return fs ? hipErrorNotSupported : hipErrorInvalidValue;
    const unsigned blocks = (unsigned)((lc.pairs + lc.PB - 1) / lc.PB);
    // the instantiation: the first of the compile-time view sizes that is this one, else the run-time view (0)
    void (*kernel)(MgConfig, const uint8_t*, const uint64_t*, uint8_t*, EncViewsLaunch, EncViewsStep) = nullptr;
#define MG_EV_VIEWS(X) X(7) X(5) X(9) X(0)
#define MG_EV_PICK(V) if (!kernel && (V == 0 || VS == V)) kernel = fs ? encode_views_kernel<V, true> : encode_views_kernel<V, false>;
    MG_EV_VIEWS(MG_EV_PICK)
#undef MG_EV_PICK
#undef MG_EV_VIEWS
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kBlock), lds, s, cfg, st.grid, st.agents, out, lc, fs ? *fs : EncViewsStep{});
    return hipGetLastError();
}

hipError_t launch_step_encode_views(const MgConfig& cfg, const MgState& st, const void* actions, int action_bytes,
                                    float* rewards, const MgGenProgram* prog, uint8_t* out, hipStream_t s, const MgEpisode* ep) {
    EncViewsStep fs{};
    fs.st = st;
    if (!step_args(&fs.a, actions, action_bytes, rewards, prog, ep)) return hipErrorInvalidValue;
    const hipError_t e = launch_encode_views(cfg, st, out, s, &fs);
    if (e != hipErrorNotSupported) return e;
    // no workgroup of whole envs fits (many agents with a large view): the step, then the views
    const hipError_t e1 = launch_step(cfg, st, actions, action_bytes, rewards, prog, s, ep);
    if (e1 != hipSuccess) return e1;
    return launch_encode_views(cfg, st, out, s, nullptr);
}

}  // namespace mg
