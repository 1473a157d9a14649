// mg_hostemu_episode.cpp — TEST INFRASTRUCTURE, not product code.
//
// The step bodies of marlgrid_amd/csrc/mg_core.h driven with an MgEpisode (reset mode and episode outputs), on the host:
// sequentially (step_run, as mg_step_ep's kernel runs a lane) and as the obs kernel's fused step does (batches of 8 envs
// in S = 8 columns: step_begin / step_par_publish / _resolve / _commit / step_agents / step_end).  The twin of
// mg_hostemu.cpp's emu_step / emu_step_par with the one new StepScratch member set; tests/test_episode_hostemu.py steps
// it against the oracle.  Nothing under marlgrid_amd/ loads it.
#include <string.h>

#include <vector>

#include "mg_core.h"

extern "C" {

int emu_ep_sizeof(void) { return (int)sizeof(MgEpisode); }

// par == 0: one env at a time, S = 1.  Odd envs without pre-loaded front cells, every third with the write-back left to
// the caller (as emu_step).
static int ep_step_seq(const MgConfig* cfg, const MgState* st, const void* actions, int action_bytes, float* rewards,
                       const MgGenProgram& prog, bool has_prog, const MgEpisode* ep) {
    std::vector<uint64_t> rec(MG_MAX_AGENTS);
    std::vector<uint32_t> head(MG_MT_HEAD);
    std::vector<uint8_t> act(MG_MAX_AGENTS), fb(MG_MAX_AGENTS), oflags(MG_MAX_OBJ, 0), ord(MG_MAX_AGENTS);
    for (int i = 1; i < cfg->n_obj; i++) oflags[i] = cfg->obj[i].flags;
    mg::StepScratch sc;
    sc.rec = rec.data(); sc.head = head.data(); sc.act = act.data(); sc.ord = ord.data();
    sc.obj = cfg->obj; sc.oflags = oflags.data(); sc.S = 1; sc.col = 0;
    sc.ep = ep;
    sc.ep_rewards = rewards;
    for (int b = 0; b < cfg->B; b++) {
        sc.fb = (b & 1) ? nullptr : fb.data();
        const mg::StepEnv e = mg::step_load(*cfg, *st, actions, action_bytes, b, sc);
        uint8_t* home = st->grid + (size_t)b * cfg->cells_stride;
        std::vector<uint8_t> staged(home, home + cfg->cells_stride);
        sc.defer_writeback = (b % 3) == 2;
        const mg::StepOut out = mg::step_run(*cfg, *st, prog, has_prog, rewards, b, e, sc, staged.data());
        if (sc.defer_writeback) {
            for (int k = 0; k < cfg->n_agents; k++) st->agents[(size_t)b * cfg->n_agents + k] = rec[k];
            for (int j = 0; j < MG_MT_HEAD; j++) st->mt_head[(size_t)b * MG_MT_HEAD + j] = head[(j + out.head_k) & (MG_MT_HEAD - 1)];
        }
        if (out.wrote) memcpy(home, staged.data(), cfg->cells_stride);
        else if (memcmp(home, staged.data(), cfg->cells_stride) != 0) return -101;
    }
    return 0;
}

int emu_ep_step(const MgConfig* cfg, const MgState* st, const void* actions, int action_bytes, float* rewards,
                const MgGenProgram* auto_reset, const MgEpisode* ep, int par, int64_t* n_serial) {
    if (action_bytes != 1 && action_bytes != 4 && action_bytes != 8) return -100;
    if (ep && ep->reset_mode == 1 && !auto_reset) return -100;
    MgGenProgram none;
    memset(&none, 0, sizeof(none));
    const MgGenProgram& prog = auto_reset ? *auto_reset : none;
    if (!par || cfg->n_agents > 8) return ep_step_seq(cfg, st, actions, action_bytes, rewards, prog, auto_reset != nullptr, ep);
    const int n = cfg->n_agents, stride = cfg->cells_stride;
    std::vector<uint64_t> rec(n * 8), rec_out(n * 8);
    std::vector<uint32_t> head(MG_MT_HEAD * 8);
    std::vector<uint8_t> act(n * 8), pflag(n * 8), ordp(n * 8), oflags(MG_MAX_OBJ, 0), grids((size_t)8 * stride);
    std::vector<int32_t> psc(8);
    for (int i = 1; i < cfg->n_obj; i++) oflags[i] = cfg->obj[i].flags;
    for (int b0 = 0; b0 < cfg->B; b0 += 8) {
        const int kb = cfg->B - b0 < 8 ? cfg->B - b0 : 8;
        mg::StepScratch sc;
        sc.rec = rec.data(); sc.head = head.data(); sc.act = act.data(); sc.fb = nullptr;
        sc.obj = cfg->obj; sc.oflags = oflags.data(); sc.S = 8; sc.col = 0;
        sc.pflag = pflag.data(); sc.ordp = ordp.data(); sc.psc = psc.data(); sc.rec_out = rec_out.data();
        sc.defer_writeback = true;
        sc.ep = ep;
        sc.ep_rewards = rewards;
        memset(pflag.data(), 0xEE, pflag.size());
        memset(ordp.data(), 0xEE, ordp.size());
        mg::StepCtx ctx[8];
        for (int j = 0; j < kb; j++) {
            sc.col = j;
            memcpy(grids.data() + (size_t)j * stride, st->grid + (size_t)(b0 + j) * stride, stride);
            const mg::StepEnv e = mg::step_load(*cfg, *st, actions, action_bytes, b0 + j, sc);
            ctx[j] = mg::step_begin(*cfg, *st, b0 + j, e, sc, grids.data() + (size_t)j * stride);
            mg::step_par_publish(*cfg, sc, ctx[j]);
        }
        mg::ParLane P[64];
        bool serial[64];
        for (int lane = 0; lane < 64; lane++) P[lane] = mg::step_par_resolve(*cfg, sc, grids.data(), kb, lane);
        for (int lane = 0; lane < 64; lane++) serial[lane] = mg::step_par_commit(*cfg, *st, rewards, b0, sc, P[lane], lane);
        for (int lane = 0; lane < 64; lane++)
            if (P[lane].live && !serial[lane]) rec[lane] = rec_out[lane];
        for (int j = 0; j < kb; j++) {
            const int b = b0 + j;
            sc.col = j;
            uint8_t* g = grids.data() + (size_t)j * stride;
            for (int k = 1; k < n; k++)
                if (serial[k * 8 + j] != serial[j]) return -102;
            if (ctx[j].pending && serial[j]) return -103;          // a reset call asks for nothing
            if (serial[j]) { mg::step_agents(*cfg, *st, rewards, b, sc, g, ctx[j]); if (n_serial) (*n_serial)++; }
            const mg::StepOut out = mg::step_end(*cfg, *st, prog, auto_reset != nullptr, b, sc, g, ctx[j]);
            for (int k = 0; k < n; k++) st->agents[(size_t)b * n + k] = rec[k * 8 + j];
            for (int i = 0; i < MG_MT_HEAD; i++) st->mt_head[(size_t)b * MG_MT_HEAD + i] = head[((i + out.head_k) & (MG_MT_HEAD - 1)) * 8 + j];
            uint8_t* home = st->grid + (size_t)b * stride;
            if (out.wrote) memcpy(home, g, stride);
            else if (memcmp(home, g, stride) != 0) return -101;
        }
    }
    return 0;
}

}  // extern "C"
