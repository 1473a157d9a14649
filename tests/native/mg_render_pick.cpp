// TEST INFRASTRUCTURE — the launcher's pick (marlgrid_amd/csrc/mg_render_pick.h), the very text libmarlgrid_hip.so compiles,
// built for the host with g++ and called through ctypes (tests/test_render_pick.py).
#include "mg_render_pick.h"

extern "C" {

int pick_sizeof_config(void) { return (int)sizeof(MgConfig); }

// out [n][3 wants][7]: picked (1 / 0), vs, ts, wpb, v, rm, lds;  min_lds [n]: render_min_lds_bytes (mg_render_obs_lds_bytes)
void pick_rows(const MgConfig* cfgs, int n, int32_t* out, int32_t* min_lds) {
    for (int i = 0; i < n; i++) {
        min_lds[i] = mg::render_min_lds_bytes(cfgs[i]);
        for (int w = 0; w < 3; w++) {
            int32_t* o = out + ((size_t)i * 3 + w) * 7;
            mg::RenderPick p = {0, 0, 0, 0, 0, 0};
            o[0] = mg::render_pick(cfgs[i], (mg::RenderWant)w, &p) ? 1 : 0;
            o[1] = p.vs; o[2] = p.ts; o[3] = p.wpb; o[4] = p.v; o[5] = p.rm; o[6] = p.lds;
        }
    }
}

// the entries of MG_RENDER_ALL (product build: no measurement variants) as [count][5]: vs, ts, wpb, v, rm
int pick_list(int32_t* out, int cap) {
    int k = 0;
#define MG_PICK_ENTRY(VS, TS, WPB, V, RM) \
    if (k < cap) { int32_t* o = out + 5 * k; o[0] = VS; o[1] = TS; o[2] = WPB; o[3] = V; o[4] = RM; } \
    k++;
    MG_RENDER_ALL(MG_PICK_ENTRY)
#undef MG_PICK_ENTRY
    return k;
}

}  // extern "C"
