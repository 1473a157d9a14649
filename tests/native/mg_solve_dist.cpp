// TEST INFRASTRUCTURE — the bodies of mg_solve_distance (marlgrid_amd/csrc/mg_solve_core.h) built for the host with g++ and
// called through ctypes (tests/native/hostemu_solve.py): solve_lds_kernel of mg_solve_dist.hip emulated over plain arrays — the
// phases in the kernel's order, the lanes of a phase run one after the other (64: the kernel's wave; 1: one lane walks every
// item), the "LDS" a heap block of solve_scratch_bytes.  Every scratch index is checked against the size of what it indexes
// (MG_SOLVE_HOST_CHECKS: plain asserts).  sd_run returns 0, -100 / -101 where mg_solve_distance would (MG_E_ARG /
// MG_E_UNSUPPORTED), having written nothing.
#include <stdlib.h>
#include <string.h>

#define MG_SOLVE_HOST_CHECKS 1
#include "mg_solve_core.h"

extern "C" {

size_t sd_scratch_bytes(int W, int H, int max_doors, int max_items) { return mg::solve_scratch_bytes(W, H, max_doors, max_items); }

int sd_run(const MgConfig* cfg, const MgState* st, const uint8_t* mask, int max_doors, int max_items, int32_t* agent_dist,
           int8_t* agent_action, uint8_t* env_exact, int lanes) {
    const int W = cfg->W, H = cfg->H, n = cfg->n_agents;
    if (max_doors < 0 || max_doors > mg::kSolveMaxDoors || max_items < 0 || max_items > mg::kSolveMaxItems) return MG_E_ARG;
    if (lanes < 1 || lanes > 64) return MG_E_ARG;
    const size_t bytes = mg::solve_scratch_bytes(W, H, max_doors, max_items);
    if (bytes > 160 * 1024) return MG_E_UNSUPPORTED;
    void* mem = malloc(bytes);
    if (!mem) return -1;
    for (int b = 0; b < cfg->B; b++) {
        if (mask && !mask[b]) continue;
        memset(mem, 0xA5, bytes);       // (LDS is not zero when a wave starts)
        const mg::SolveScratch s0 = mg::solve_scratch(mem, W, H, max_doors, max_items);
        assert((uint8_t*)(s0.t + 1) <= (uint8_t*)mem + bytes && (uint8_t*)s0.t == (uint8_t*)mem + bytes - mg::kSolveTailBytes);
        const uint8_t* grid_b = st->grid + (size_t)b * cfg->cells_stride;
        const uint64_t* rec_b = st->agents + (size_t)b * n;
        for (int l = 0; l < lanes; l++) mg::solve_build(*cfg, grid_b, s0, l, lanes);
        for (int l = 0; l < lanes; l++) mg::solve_count(s0, l, lanes);
        for (int l = 0; l < lanes; l++) mg::solve_table(*cfg, grid_b, s0, max_doors, max_items, l, lanes);
        const int D = s0.t->D, K = s0.t->K;
        assert(D >= 0 && D <= max_doors && K >= 0 && K <= max_items);
        for (int cls = mg::solve_next_class(*cfg, rec_b, -1); cls >= 0; cls = mg::solve_next_class(*cfg, rec_b, cls)) {
            mg::SolveScratch s = s0;
            const int Ke = cls ? 0 : K, pass_key = cls >= 2 ? cls - 2 : -1;
            const int layers = mg::solve_layers(D, Ke);
            assert(layers <= s.cap_layers);
            const uint64_t all = layers >= 64 ? ~0ull : (1ull << layers) - 1ull;
            for (int l = 0; l < lanes; l++) mg::solve_pass_init(s, l, lanes);
            uint64_t fm = 0, stale = all;
            bool pending = false, due = false;
            for (int l = 0; l < lanes; l++) fm |= mg::solve_expand(s, nullptr, s.front, layers, D, all, l, lanes);
            for (int l = 0; l < lanes; l++) pending |= mg::solve_agents(*cfg, rec_b, s, nullptr, s.front, cls, Ke, 1, l, lanes);
            const int max_levels = mg::solve_max_levels(W, H, layers, D);
            int level = 1;
            while (pending && (fm || due) && level < max_levels) {
                level++;
                uint64_t nm = 0;
                due = pending = false;
                for (int l = 0; l < lanes; l++) nm |= mg::solve_expand(s, s.front, s.next, layers, D, fm | stale, l, lanes);
                if (D + Ke > 0)         // (the kernel skips the phase for an env without tracked objects)
                    for (int l = 0; l < lanes; l++) nm |= mg::solve_edges(s, s.front, s.next, layers, D, Ke, pass_key, l, lanes, &due);
                for (int l = 0; l < lanes; l++) pending |= mg::solve_agents(*cfg, rec_b, s, s.front, s.next, cls, Ke, level, l, lanes);
                stale = fm;
                fm = nm;
                uint64_t* t = s.front;
                s.front = s.next;
                s.next = t;
            }
        }
        for (int l = 0; l < lanes; l++)
            mg::solve_finish(*cfg, s0, agent_dist + (size_t)b * n, agent_action ? agent_action + (size_t)b * n : nullptr,
                             env_exact ? env_exact + b : nullptr, l, lanes);
    }
    free(mem);
    return 0;
}

}  // extern "C"
