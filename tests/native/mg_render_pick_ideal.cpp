// TEST INFRASTRUCTURE — render_pick_ideal (marlgrid_amd/csrc/mg_render_pick.h: which instantiation a configuration would get if
// any could be made — what mg_render_specialize compiles), the very text libmarlgrid_hip.so compiles, built for the host with
// g++ and called through ctypes (tests/test_specialize_host.py).
#include "mg_render_pick.h"

extern "C" {

int ideal_sizeof_config(void) { return (int)sizeof(MgConfig); }

// out [n][4 wants][2][7]: [0] render_pick_ideal, [1] render_pick — picked (1 / 0), vs, ts, wpb, v, rm, lds;
// facts [n][4]: render_big_grid, render_fits(cfg, 4, 0), render_fits(cfg, 4, 2), gather_trips(view_size, tile_size)
void ideal_rows(const MgConfig* cfgs, int n, int32_t* out, int32_t* facts) {
    for (int i = 0; i < n; i++) {
        const MgConfig& c = cfgs[i];
        for (int w = 0; w < 4; w++)
            for (int k = 0; k < 2; k++) {
                int32_t* o = out + (((size_t)i * 4 + w) * 2 + k) * 7;
                mg::RenderPick p = {0, 0, 0, 0, 0, 0};
                o[0] = (k == 0 ? mg::render_pick_ideal(c, (mg::RenderWant)w, &p) : mg::render_pick(c, (mg::RenderWant)w, &p)) ? 1 : 0;
                o[1] = p.vs; o[2] = p.ts; o[3] = p.wpb; o[4] = p.v; o[5] = p.rm; o[6] = p.lds;
            }
        int32_t* f = facts + (size_t)i * 4;
        f[0] = mg::render_big_grid(c) ? 1 : 0;
        f[1] = mg::render_fits(c, 4, 0) ? 1 : 0;
        f[2] = mg::render_fits(c, 4, 2) ? 1 : 0;
        f[3] = c.tile_size >= 1 && c.view_size >= 1 ? mg::gather_trips(c.view_size, c.tile_size) : 0;
    }
}

}  // extern "C"
