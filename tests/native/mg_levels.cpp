// TEST INFRASTRUCTURE — the bodies of mg_level_seed / mg_level_apply (marlgrid_amd/csrc/mg_level_core.h) built for the host
// with g++ and called through ctypes (tests/test_levels_host.py): the kernels of mg_levels.hip emulated lane by lane over
// numpy arrays.
#include "mg_level_core.h"

extern "C" {

int lv_key(long long seed, uint32_t* key) { return mg::level_key((int64_t)seed, key); }
int lv_key_rule(uint32_t w0, uint32_t w1, uint32_t* key) { return mg::level_key_rule(w0, w1, key); }

// one generator from a key, by the seeding body of the bank (which = 1) or by mt_seed_env, the one of mg_mt_seed (0)
void lv_seed_key(int which, const uint32_t* key, int klen, uint32_t* mt, int32_t* mt_pos, uint32_t* head) {
    if (which) mg::level_seed_mt(key, klen, mt, mt_pos, head);
    else mg::mt_seed_env(key, klen, mt, mt_pos, head);
}

// level_seed_kernel: rows in turn
void lv_seed(int n, const int64_t* seeds, const int64_t* slots, const uint8_t* mask, int n_slots, uint32_t* bank_mt, int32_t* bank_pos,
             uint32_t* bank_head, int64_t* bank_seed) {
    for (int i = 0; i < n; i++) mg::level_seed_row(i, seeds, slots, mask, n_slots, bank_mt, bank_pos, bank_head, bank_seed);
}

// level_apply_kernel: every lane decides, the "wave" (one lane here) copies for the selected ones, every lane publishes
void lv_apply(const MgConfig* cfg, const MgState* st, int rule, const uint8_t* mask, const int64_t* level_of_env, int n_slots,
              const uint32_t* bank_mt, const int32_t* bank_pos, const uint32_t* bank_head, const int64_t* bank_seed,
              int64_t* episode_level, int64_t* out_level) {
    for (int b = 0; b < cfg->B; b++) {
        const int what = mg::level_select(*cfg, *st, b, rule, mask, level_of_env, n_slots, bank_seed);
        if (what >= 0) mg::level_copy(*st, b, what, bank_mt, bank_pos, bank_head, 0, 1);
        mg::level_publish(*cfg, *st, b, what, bank_seed, episode_level, out_level);
    }
}

// the predicate the step uses, for the test's constructed records
int lv_episode_ended(const MgConfig* cfg, const uint64_t* rec, int step_count) { return mg::episode_ended(*cfg, rec, 1, 0, step_count) ? 1 : 0; }

}  // extern "C"
