// mg_render.hip — the launcher of the observation raster (mg_render_obs / mg_step_render*): render_pick (mg_render_pick.h) says
// which instantiation of mg::render_kernel (mg_render_kernel.h) a configuration gets, one generated lookup over MG_RENDER_ALL
// finds it.  The instantiations themselves are made, in parallel, by mg_render_inst.hip; here they are only referred to.
#include "mg_render_kernel.h"

namespace mg {

#if defined(MG_AB_VARIANTS)
unsigned long long* g_ab_stamps = nullptr;
extern "C" int mg_ab_stamps(unsigned long long* p) { g_ab_stamps = p; return 0; }
#endif

#if !defined(MG_DEV_ONLY)
MG_RENDER_ALL(MG_RENDER_EXTERN)
MG_RENDER_DELTA(MG_RENDER_EXTERN)
MG_RENDER_DELTA_X(MG_RENDER_EXTERN)
#endif

using RenderLauncher = hipError_t (*)(const MgConfig&, const MgState&, uint8_t*, uint8_t*, uint8_t*, uint8_t*, hipStream_t,
                                      const FusedStep&, size_t);
static RenderLauncher render_launcher(const RenderPick& p) {
#define MG_RENDER_MATCH(VS, TS, WPB, V, RM) \
    if (p.vs == VS && p.ts == TS && p.wpb == WPB && p.v == V && p.rm == RM) return &launch_render_t<VS, TS, WPB, V, RM>;
    MG_RENDER_ALL(MG_RENDER_MATCH)
    return nullptr;
}
// ... and a kDelta pick in its own list (mg_step_render_delta), a kDeltaEncode / kDeltaEpisode / kDeltaEncodeEpisode pick in theirs
// (mg_step_render_delta_ex)
static RenderLauncher render_delta_launcher(const RenderPick& p) {
#if !defined(MG_DEV_ONLY)
    MG_RENDER_DELTA(MG_RENDER_MATCH)
    MG_RENDER_DELTA_X(MG_RENDER_MATCH)
#endif
    return nullptr;
}
#undef MG_RENDER_MATCH

#if defined(MG_AB_VARIANTS) || defined(MG_EXP) || defined(MG_DEV_ONLY)
// Measurement and development builds only (libmarlgrid_hip_ab.so, `make exp`, -DMG_DEV_ONLY): another instantiation than the
// pick's, asked for through the environment or the build.  The product build has none of this.
static void render_override(const MgConfig& cfg, RenderPick& p) {
    int wpb = 0;        // the workgroup shape asked for: the largest one of the pick's shape, no larger, that is instantiated and fits LDS
    const int enc_ne = (p.v & 16) ? render_enc_entries(cfg) : 0;
#if defined(MG_AB_VARIANTS)
    if (const char* f = getenv("MG_RENDER_WPB")) wpb = atoi(f);
    if (p.vs == 7 && p.ts == 8 && p.v == 0 && p.rm == 0) {      // tools/ab_render.py
        const int v = getenv("MG_RENDER_VARIANT") ? atoi(getenv("MG_RENDER_VARIANT")) : 0;
        if (v == 2 || v == 3 || v == 4 || v == 6 || v == 11) p.v = v;
        else if (getenv("MG_RENDER_RASTER") && atoi(getenv("MG_RENDER_RASTER")) == 1) p.rm = 1;   // assemble-and-stream at tile 8
    }
    if (p.v == 9 && p.rm == 2 && getenv("MG_RENDER_RT_TS") && atoi(getenv("MG_RENDER_RT_TS")) != 0) {   // the run-time-tile twin of a gather pick
        p.ts = 0; p.rm = 0;
        if (p.wpb > 4 || choose_wpb(cfg, 2) == 16) p.wpb = render_fits(cfg, 12, 0) ? 12 : 8;
    }
#endif
#if defined(MG_EXP) && (MG_EXP & 6)      // experiment builds (tools/wpb_sweep.py): one workgroup shape for every batch
    wpb = (MG_EXP & 6) == 2 ? 4 : (MG_EXP & 6) == 4 ? 8 : 16;
#endif
#if defined(MG_EXP) && (MG_EXP & 8)      // experiment build: 12-wave workgroups (3 waves per SIMD, a 168-VGPR budget) for the plain kernel
    if (p.vs == 7 && p.ts == 8 && p.wpb == 16 && p.v == 0 && p.rm == 0) p.wpb = 12;
#endif
    for (int w = wpb; w == 16 || w == 12 || w == 8 || w == 4; w -= 4) {
        p.wpb = w;
        if (render_launcher(p) && (w == 4 || render_lds_bytes(cfg, w, p.rm, p.v, enc_ne) <= kRenderLdsMax)) break;
    }
#if defined(MG_DEV_ONLY)
    const int only[5] = {MG_DEV_ONLY};
    p.vs = only[0]; p.ts = only[1]; p.wpb = only[2]; p.v = only[3]; p.rm = only[4];
#endif
    p.lds = (int)render_lds_bytes(cfg, p.wpb, p.rm, p.v, (p.v & 16) ? render_enc_entries(cfg) : 0);      // (MG_DEV_ONLY: v may differ)
}
#endif

// The kernel launch of mg_render_obs / mg_step_render / mg_step_render_encode / mg_step_render_ep / mg_step_render_delta[_ex].
hipError_t launch_render(const MgConfig& cfg, const MgState& st, uint8_t* obs, uint8_t* view_cells,
                         uint8_t* view_agent, uint8_t* vis_mask, hipStream_t s, const FusedStep* fused_step, const RenderPick* picked) {
    if (cfg.B <= 0) return hipSuccess;
    FusedStep fs{};                 // no step: the raster alone
    fs.action_bytes = 8;
    if (fused_step) fs = *fused_step;
    const RenderWant want = render_want_of(fs.sig != nullptr, fs.encode_out != nullptr, fs.has_ep != 0);
    if (!fs.sig && fs.has_ep && fs.encode_out) return hipErrorInvalidValue;
    if ((view_cells || view_agent || vis_mask) && (want != kPlain || !(view_cells && view_agent && vis_mask))) return hipErrorInvalidValue;
    RenderPick p;
    if (picked) p = *picked;
    else if (!render_pick(cfg, want, &p)) return want == kPlain ? hipErrorInvalidValue : hipErrorNotSupported;
    if (render_want_encode(want)) fs.enc_ne = render_enc_entries(cfg);
#if defined(MG_AB_VARIANTS) || defined(MG_EXP) || defined(MG_DEV_ONLY)
    render_override(cfg, p);
    if (p.lds > (int)kRenderLdsMax) return hipErrorInvalidValue;
#endif
    RenderLauncher launch = render_launcher(p);
    if (!launch && render_want_delta(want)) launch = render_delta_launcher(p);
    if (!launch) return hipErrorInvalidValue;
    return launch(cfg, st, obs, view_cells, view_agent, vis_mask, s, fs, (size_t)p.lds);
}

}  // namespace mg
