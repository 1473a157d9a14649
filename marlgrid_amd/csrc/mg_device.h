// mg_device.h — device-side helpers shared by the gfx950 kernels of libmarlgrid_hip.so.
//
// Written for CDNA4 only (wave64, 160 KiB LDS/CU); no portability layer.
#pragma once

#if !defined(__HIPCC_RTC__)   // (a run-time compile — mg_rtc.hip — has no system headers: its source supplies these names)
#include <hip/hip_runtime.h>
#include <stdint.h>
#endif

#include "marlgrid_hip.h"
#include "mg_core.h"
#include "mg_render_pick.h"   // the obs kernel's LDS layouts (shared with the host) and the launcher's pick

namespace mg {

constexpr int kWave = 64;
constexpr int kBlock = 256;  // workgroup size of the lane-per-env / lane-per-cell kernels

// intra-wave LDS hand-off: DS operations of one wave execute in order, so only the compiler has
// to be kept from reordering across the hand-off.
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// GridAgentInterface.render_post (marlgrid/agents.py:92-119): the sprite colour of an active
// 'prestige' agent, between red (prestige 0) and blue: (ps*blue + (1-ps)*red).astype(int)
struct PrestigeColor { uint32_t r, g, b; };
__device__ inline PrestigeColor prestige_color(double prestige, double scale) {
    const double ps = tanh(prestige / scale);
    PrestigeColor c;
    c.r = (uint32_t)(long long)(ps * 0.0 + (1. - ps) * 255.0);
    c.g = (uint32_t)(long long)(ps * 0.0 + (1. - ps) * 0.0);
    c.b = (uint32_t)(long long)(ps * 255.0 + (1. - ps) * 0.0);
    return c;
}

// One pixel of the tile a recoloured agent produces: alpha = the white sprite's coverage value,
// `base` = the overlappable object's pixel it stands on (blend_tiles, base.py:260-273) or NULL,
// `border` = the empty tile's pixel when the border rule applies (base.py:296-298) or NULL.
__device__ inline void prestige_pixel(uint32_t alpha, const PrestigeColor& col, uint32_t M, const uint8_t* base,
                                      const uint8_t* border, uint8_t* out) {
    uint32_t v[3] = {(alpha * col.r) >> 8, (alpha * col.g) >> 8, (alpha * col.b) >> 8};
    if (base) {
        if (M == 0) { v[0] = base[0]; v[1] = base[1]; v[2] = base[2]; }
        else {
            const uint32_t al = v[0] + v[1] + v[2];
#pragma unroll
            for (int c = 0; c < 3; c++) v[c] = ((uint32_t)base[c] * (M - al) + v[c] * al) / M;
        }
    }
    if (border) { v[0] += border[0]; v[1] += border[1]; v[2] += border[2]; }     // uint8 wrap-around add
    out[0] = (uint8_t)v[0]; out[1] = (uint8_t)v[1]; out[2] = (uint8_t)v[2];
}

// What mg_step_render adds to a launch of the obs kernel: the wave that renders an env first steps it.
struct FusedStep {
    const void* actions;      // [B][n], action_bytes each
    float* rewards;           // [B][n]
    int32_t action_bytes, enabled, has_prog;
    MgGenProgram prog;        // auto-reset program (has_prog)
    uint8_t* encode_out;      // mg_step_render_encode: MultiGrid.encode of the stepped batch, [B][W][H][3] (null: not asked for)
    uint32_t enc_m_cells, enc_m_n;   // ... its divide-by-multiply constants: ceil(2^32 / (W * H)), ceil(2^32 / n)
    int32_t enc_ne;           // ... dwords of its LDS table — one per grid byte value: object kinds, then the agent codes n_obj +
                              //     4 k + dir —, (n_obj + 4 n) rounded up to 16 (mg_render_pick.h: render_enc_entries; 0: none)
    int32_t has_ep;           // mg_step_render_ep: `ep` is set — the launcher then takes an instantiation with the episode code
    MgEpisode ep;             //     compiled in (V + 32); the plain ones never look at either
    uint16_t* sig;            // mg_step_render_delta (V + 64): the signature of what `obs` holds (null: not asked for) — compact: per agent
                              //     image a 64-byte slot of one-byte codes, env e at e * n * 64 (delta_sig_*, mg_step_layout.h); kSigWide:
                              //     per env the tmap's 16-bit entries, RenderScratch::tmap_stride bytes
    int32_t sig_flags;        //     kSigForce — every band counts as changed, the signature is only recorded — | kSigWide — the 16-bit
                              //     layout, for a configuration whose codes do not fit a byte (the launcher: delta_sig_compact)
};
enum { kSigForce = 1, kSigWide = 2 };

// x / d for small operands (x * d < 2^32) by multiply-high with ceil(2^32 / d): item index -> (slot, rest)
struct SmallDiv {
    uint32_t d, m;
    __host__ __device__ explicit SmallDiv(uint32_t d_) : d(d_), m(d_ > 1 ? 0xFFFFFFFFu / d_ + 1u : 0u) {}
    __device__ uint32_t div(uint32_t x) const { return d > 1 ? __umulhi(x, m) : x; }
};

// x / d with ONE full-rate multiply: on CDNA a 32-bit v_mul_lo / v_mul_hi issues at a quarter of the rate of the
// 24-bit v_mul_u32_u24 (and of every add, shift and compare), and the view / raster index arithmetic is made of
// divisions — which is why the instantiations off the HBM-bound fast path were VALU-bound.  m = ceil(2^20 / d);
// (x * m) >> 20 is x / d or x / d + 1 for every x < 2^20 whose quotient is < 2^11 (the product stays under 2^32,
// both operands under 2^24), and the one compare-and-subtract makes it exact.  `exact`: the caller knows
// x * (m * d - 2^20) < 2^20 for every x it passes (small compile-time divisors), so the fix-up is dropped.
struct Div20 {
    uint32_t d, m;
    __host__ __device__ explicit Div20(uint32_t d_) : d(d_), m(((1u << 20) + d_ - 1u) / d_) {}
    __host__ __device__ Div20(uint32_t d_, uint32_t m_) : d(d_), m(m_) {}      // (m worked out by the launcher)
    template <bool exact = false>
    __device__ __forceinline__ uint32_t div(uint32_t x) const {
        uint32_t q = __umul24(x, m) >> 20;
        if constexpr (!exact) q -= (__umul24(q, d) > x) ? 1u : 0u;
        return q;
    }
};

// What a launch of the obs kernel would otherwise work out in every wave before it requests its first byte — the
// LDS layout (render_scratch_for: four candidate layouts), the envs per wave, the dividers' multipliers: ~600
// instructions, 1.5 us of the launch's store-free head (tools/phase_stamps.py) — worked out by the launcher instead.
struct RenderLaunch {
    RenderScratch L;
    int per_wave;                               // envs per wave of the persistent grid
    uint32_t m_n, m_nv, m_nvVV, m_VV, m_VS, m_nvVS;   // Div20 multipliers of n, nv, nv * VS^2, VS^2, VS, nv * VS
    int depth_mode;                             // measurement builds: look-ahead depth forced for all waves (0: by wave)
    int atlas_lds;                              // bytes the atlas takes in LDS (render_atlas_lds_bytes; 0: read in place)
    RenderShared sh;                            // the block-shared tables behind it (render_shared_layout)
#if defined(MG_AB_VARIANTS)
    unsigned long long* stamps;                 // measurement build: phase stamps of every wave (tools/phase_stamps.py), or null
    int prio_mode;                              // measurement build: the delta launch's wave-priority policy (kDeltaPrio*, mg_render_kernel.h)
#endif
};

}  // namespace mg
