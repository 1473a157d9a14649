// TEST INFRASTRUCTURE — the body of mg_level_apply_rows (marlgrid_amd/csrc/mg_level_core.h) built for the host with g++ and
// called through ctypes (tests/test_level_rows_host.py): level_apply_rows_kernel of mg_levels.hip emulated over numpy arrays —
// every lane decides, the "wave" copies for the selected ones with `lanes` lanes in turn (64: the kernel's; 1: one lane walks
// every item), every lane publishes.
#include "mg_level_core.h"

extern "C" {

void lvr_seed(int n, const int64_t* seeds, int n_slots, uint32_t* bank_mt, int32_t* bank_pos, uint32_t* bank_head, int64_t* bank_seed) {
    for (int i = 0; i < n; i++) mg::level_seed_row(i, seeds, nullptr, nullptr, n_slots, bank_mt, bank_pos, bank_head, bank_seed);
}

void lvr_apply_rows(const MgConfig* cfg, const MgState* st, int rule, const uint8_t* mask, const int64_t* level_of_env, int n_slots,
                    const uint32_t* bank_mt, const int32_t* bank_pos, const uint32_t* bank_head, const int64_t* bank_seed,
                    int64_t* episode_level, int64_t* out_level, const uint8_t* bank_params, const uint8_t* bank_edits, int K,
                    uint8_t* env_params, uint8_t* env_edits, int lanes) {
    mg::LevelRows rows;
    rows.bank_params = reinterpret_cast<const uint32_t*>(bank_params);
    rows.env_params = reinterpret_cast<uint32_t*>(env_params);
    rows.bank_edits = reinterpret_cast<const uint32_t*>(bank_edits);
    rows.env_edits = reinterpret_cast<uint32_t*>(env_edits);
    rows.K = K;
    for (int b = 0; b < cfg->B; b++) {
        const int what = mg::level_select(*cfg, *st, b, rule, mask, level_of_env, n_slots, bank_seed);
        if (what >= 0)
            for (int lane = 0; lane < lanes; lane++) mg::level_copy(*st, b, what, bank_mt, bank_pos, bank_head, lane, lanes, &rows);
        mg::level_publish(*cfg, *st, b, what, bank_seed, episode_level, out_level);
    }
}

}  // extern "C"
