// TEST INFRASTRUCTURE — the launcher's pick for mg_step_render_delta (marlgrid_amd/csrc/mg_render_pick.h: RenderWant kDelta and
// its list MG_RENDER_DELTA), built for the host with g++ and called through ctypes (tests/test_obs_delta_host.py).
#include "mg_render_pick.h"

extern "C" {

int delta_sizeof_config(void) { return (int)sizeof(MgConfig); }

// out [n][7]: picked (1 / 0), vs, ts, wpb, v, rm, lds for the fourth want
void delta_rows(const MgConfig* cfgs, int n, int32_t* out) {
    for (int i = 0; i < n; i++) {
        int32_t* o = out + (size_t)i * 7;
        mg::RenderPick p = {0, 0, 0, 0, 0, 0};
        o[0] = mg::render_pick(cfgs[i], mg::kDelta, &p) ? 1 : 0;
        o[1] = p.vs; o[2] = p.ts; o[3] = p.wpb; o[4] = p.v; o[5] = p.rm; o[6] = p.lds;
    }
}

// the entries of MG_RENDER_DELTA as [count][5]: vs, ts, wpb, v, rm
int delta_list(int32_t* out, int cap) {
    int k = 0;
#define MG_PICK_ENTRY(VS, TS, WPB, V, RM) \
    if (k < cap) { int32_t* o = out + 5 * k; o[0] = VS; o[1] = TS; o[2] = WPB; o[3] = V; o[4] = RM; } \
    k++;
    MG_RENDER_DELTA(MG_PICK_ENTRY)
#undef MG_PICK_ENTRY
    return k;
}

int delta_want_value(void) { return (int)mg::kDelta; }

}  // extern "C"
