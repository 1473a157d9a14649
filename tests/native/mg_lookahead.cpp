// TEST INFRASTRUCTURE — the bodies of mg_fork_rows and mg_rollout (marlgrid_amd/csrc/mg_lookahead_core.h) built for the host with
// g++ and called through ctypes (tests/native/hostemu_lookahead.py): fork_kernel and rollout_kernel of mg_lookahead.hip emulated
// over plain arrays.  la_fork: the waves in launch order, the `lanes` lanes of a wave one after the other (64: the kernel's wave;
// 1: one lane walks every item).  la_rollout: workgroups of S lanes (64 / 256: the kernel's; 1), the "LDS" a heap block of
// lane_step_bytes(n, S) filled with a pattern and the tables staged before any row runs; the rows of a workgroup one after the
// other, each through all its T steps — on the GPU they interleave, and a row that read another row's column would differ here.
#include <stdlib.h>
#include <string.h>

#include "mg_lookahead_core.h"

extern "C" {

int la_fork(const MgConfig* cfg, const MgState* src, const MgState* dst, const int64_t* src_of_dst, const int64_t* dst_of_row, int dst_B,
            int R, int m, int lanes) {
    if (R < 0 || m < 1 || R % m != 0 || lanes < 1 || lanes > 64) return MG_E_ARG;
    for (int w = 0; w < R; w++) {
        const int r = mg::fork_row_of_wave(w, R, m);
        if (r < 0 || r >= R) return -104;
        for (int l = 0; l < lanes; l++) mg::fork_row(*cfg, *src, *dst, src_of_dst, dst_of_row, dst_B, r, m, l, lanes);
    }
    return 0;
}

int la_rollout(const MgConfig* cfg, const MgState* st, const void* actions, int action_bytes, int T, int m, float* rewards, uint8_t* done,
               int32_t* errors, int S) {
    if (action_bytes != 1 && action_bytes != 4 && action_bytes != 8) return MG_E_ARG;
    if (T < 0 || m < 1 || cfg->B % m != 0 || (S != 1 && S != 64 && S != 256)) return MG_E_ARG;
    const int n = cfg->n_agents;
    const size_t bytes = mg::lane_step_bytes(n, S);
    uint8_t* mem = static_cast<uint8_t*>(aligned_alloc(16, (bytes + 15) / 16 * 16));
    if (!mem) return -1;
    const mg::LaneStepLayout l = mg::lane_step_layout(n, S);
    MgGenProgram none;
    memset(&none, 0, sizeof(none));
    for (int r0 = 0; r0 < cfg->B; r0 += S) {
        memset(mem, 0xA5, bytes);       // (LDS is not zero when a workgroup starts)
        for (int tid = 0; tid < S; tid++)
            mg::stage_obj_tables(*cfg, reinterpret_cast<MgObjDesc*>(mem + l.obj), mem + l.oflags, tid, S);
        for (int tid = 0; tid < S && r0 + tid < cfg->B; tid++)
            mg::rollout_row(*cfg, *st, none, actions, action_bytes, T, m, rewards, done, errors, r0 + tid,
                            mg::lane_step_scratch(mem, n, S, tid));
    }
    free(mem);
    return 0;
}

}  // extern "C"
