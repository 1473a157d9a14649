// TEST INFRASTRUCTURE — the launcher's pick for mg_step_render_delta_ex (marlgrid_amd/csrc/mg_render_pick.h: the wants
// kDeltaEncode, kDeltaEpisode, kDeltaEncodeEpisode and their list MG_RENDER_DELTA_X), built for the host with g++ and called
// through ctypes (tests/test_obs_delta_ex_host.py).
#include "mg_render_pick.h"

extern "C" {

int dx_sizeof_config(void) { return (int)sizeof(MgConfig); }

// the values of kDelta, kDeltaEncode, kDeltaEpisode, kDeltaEncodeEpisode
void dx_want_values(int32_t out[4]) {
    out[0] = (int32_t)mg::kDelta; out[1] = (int32_t)mg::kDeltaEncode; out[2] = (int32_t)mg::kDeltaEpisode; out[3] = (int32_t)mg::kDeltaEncodeEpisode;
}

// out [n][7]: picked (1 / 0), vs, ts, wpb, v, rm, lds for `want` (a RenderWant value)
void dx_rows(const MgConfig* cfgs, int n, int want, int32_t* out) {
    for (int i = 0; i < n; i++) {
        int32_t* o = out + (size_t)i * 7;
        mg::RenderPick p = {0, 0, 0, 0, 0, 0};
        o[0] = mg::render_pick(cfgs[i], (mg::RenderWant)want, &p) ? 1 : 0;
        o[1] = p.vs; o[2] = p.ts; o[3] = p.wpb; o[4] = p.v; o[5] = p.rm; o[6] = p.lds;
    }
}

// the entries of a list as [count][5]: vs, ts, wpb, v, rm — which: 0 MG_RENDER_DELTA_X, 1 MG_RENDER_DELTA, 2 MG_RENDER_ALL
int dx_list(int which, int32_t* out, int cap) {
    int k = 0;
#define MG_PICK_ENTRY(VS, TS, WPB, V, RM) \
    if (k < cap) { int32_t* o = out + 5 * k; o[0] = VS; o[1] = TS; o[2] = WPB; o[3] = V; o[4] = RM; } \
    k++;
    if (which == 0) { MG_RENDER_DELTA_X(MG_PICK_ENTRY) }
    else if (which == 1) { MG_RENDER_DELTA(MG_PICK_ENTRY) }
    else { MG_RENDER_ALL(MG_PICK_ENTRY) }
#undef MG_PICK_ENTRY
    return k;
}

}  // extern "C"
