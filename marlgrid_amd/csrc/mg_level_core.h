// mg_level_core.h — replayable levels: the bodies of mg_level_seed / mg_level_apply (mg_levels.hip) as plain inline
// functions, like mg_core.h: the same text compiles with g++ for the host tests (tests/native/mg_levels.cpp).
//
// A level is a seed.  `env.seed(s); env.reset()` of the reference (marlgrid/base.py:371-374, 402-416) gives the episode
// that follows a generator freshly seeded with s: gym's seeding.np_random hashes the seed — sha512 of its decimal text,
// the digest's first eight bytes as two little-endian words — into the key of MT19937's init_by_array.  A *bank* holds
// generators seeded that way (bank_mt [L][624], bank_pos [L], bank_head [L][16], bank_seed [L], -1 = empty slot); an env
// that resets is handed a copy of its level's row in place of its running stream.
#pragma once

#if !defined(__HIPCC_RTC__)   // (a run-time compile — mg_rtc.hip — has no system headers: its source supplies these names)
#include <stdint.h>
#endif

#include "mg_core.h"

namespace mg {

// ---- seed -> key: marlgrid_amd/seeding.py::seed_words on the device ---------------------------------------------------
MG_HD uint64_t sha_rotr(uint64_t x, int r) { return (x >> r) | (x << (64 - r)); }

// The first 64-bit word of SHA-512 over the decimal text of `seed` (>= 0: at most 19 digits, one block).
MG_HD uint64_t level_sha512_word0(int64_t seed) {
    constexpr uint64_t K[80] = {
        0x428a2f98d728ae22ull, 0x7137449123ef65cdull, 0xb5c0fbcfec4d3b2full, 0xe9b5dba58189dbbcull, 0x3956c25bf348b538ull,
        0x59f111f1b605d019ull, 0x923f82a4af194f9bull, 0xab1c5ed5da6d8118ull, 0xd807aa98a3030242ull, 0x12835b0145706fbeull,
        0x243185be4ee4b28cull, 0x550c7dc3d5ffb4e2ull, 0x72be5d74f27b896full, 0x80deb1fe3b1696b1ull, 0x9bdc06a725c71235ull,
        0xc19bf174cf692694ull, 0xe49b69c19ef14ad2ull, 0xefbe4786384f25e3ull, 0x0fc19dc68b8cd5b5ull, 0x240ca1cc77ac9c65ull,
        0x2de92c6f592b0275ull, 0x4a7484aa6ea6e483ull, 0x5cb0a9dcbd41fbd4ull, 0x76f988da831153b5ull, 0x983e5152ee66dfabull,
        0xa831c66d2db43210ull, 0xb00327c898fb213full, 0xbf597fc7beef0ee4ull, 0xc6e00bf33da88fc2ull, 0xd5a79147930aa725ull,
        0x06ca6351e003826full, 0x142929670a0e6e70ull, 0x27b70a8546d22ffcull, 0x2e1b21385c26c926ull, 0x4d2c6dfc5ac42aedull,
        0x53380d139d95b3dfull, 0x650a73548baf63deull, 0x766a0abb3c77b2a8ull, 0x81c2c92e47edaee6ull, 0x92722c851482353bull,
        0xa2bfe8a14cf10364ull, 0xa81a664bbc423001ull, 0xc24b8b70d0f89791ull, 0xc76c51a30654be30ull, 0xd192e819d6ef5218ull,
        0xd69906245565a910ull, 0xf40e35855771202aull, 0x106aa07032bbd1b8ull, 0x19a4c116b8d2d0c8ull, 0x1e376c085141ab53ull,
        0x2748774cdf8eeb99ull, 0x34b0bcb5e19b48a8ull, 0x391c0cb3c5c95a63ull, 0x4ed8aa4ae3418acbull, 0x5b9cca4f7763e373ull,
        0x682e6ff3d6b2b8a3ull, 0x748f82ee5defb2fcull, 0x78a5636f43172f60ull, 0x84c87814a1f0ab72ull, 0x8cc702081a6439ecull,
        0x90befffa23631e28ull, 0xa4506cebde82bde9ull, 0xbef9a3f7b2c67915ull, 0xc67178f2e372532bull, 0xca273eceea26619cull,
        0xd186b8c721c0c207ull, 0xeada7dd6cde0eb1eull, 0xf57d4f7fee6ed178ull, 0x06f067aa72176fbaull, 0x0a637dc5a2c898a6ull,
        0x113f9804bef90daeull, 0x1b710b35131c471bull, 0x28db77f523047d84ull, 0x32caab7b40c72493ull, 0x3c9ebe0a15c9bebcull,
        0x431d67c49c100d4cull, 0x4cc5d4becb3e42b6ull, 0x597f299cfc657e2aull, 0x5fcb6fab3ad6faecull, 0x6c44198c4a475817ull};
    // the block: the digits, 0x80, zeros, the length in bits — big-endian words, of which only the first three and the
    // last can be non-zero.  Digits come out least significant first: digit i from the right is byte len - 1 - i.
    const uint64_t v = (uint64_t)seed;
    int len = 1;
    for (uint64_t p = 10; len < 20 && v >= p; p *= 10) len++;
    uint64_t m0 = 0, m1 = 0, m2 = 0;
    uint64_t rest = v;
    for (int i = 0; i <= len; i++) {      // (i == 0: the 0x80 behind the last digit)
        const int at = len - i;
        uint64_t byte = 0x80;
        if (i > 0) { byte = 0x30 + rest % 10; rest /= 10; }
        const uint64_t put = byte << (56 - 8 * (at & 7));
        if ((at >> 3) == 0) m0 |= put;
        else if ((at >> 3) == 1) m1 |= put;
        else m2 |= put;
    }
    uint64_t w[16] = {m0, m1, m2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, (uint64_t)len * 8};
    uint64_t a = 0x6a09e667f3bcc908ull, b = 0xbb67ae8584caa73bull, c = 0x3c6ef372fe94f82bull, d = 0xa54ff53a5f1d36f1ull;
    uint64_t e = 0x510e527fade682d1ull, f = 0x9b05688c2b3e6c1full, g = 0x1f83d9abfb41bd6bull, h = 0x5be0cd19137e2179ull;
    const uint64_t a0 = a;
#if defined(__HIPCC__)
#pragma unroll      // (every index of w[] a constant: the schedule stays in registers)
#endif
    for (int t = 0; t < 80; t++) {
        if (t >= 16) {
            const uint64_t w15 = w[(t + 1) & 15], w2 = w[(t + 14) & 15];
            const uint64_t s0 = sha_rotr(w15, 1) ^ sha_rotr(w15, 8) ^ (w15 >> 7);
            const uint64_t s1 = sha_rotr(w2, 19) ^ sha_rotr(w2, 61) ^ (w2 >> 6);
            w[t & 15] += s0 + w[(t + 9) & 15] + s1;
        }
        const uint64_t S1 = sha_rotr(e, 14) ^ sha_rotr(e, 18) ^ sha_rotr(e, 41);
        const uint64_t ch = (e & f) ^ (~e & g);
        const uint64_t t1 = h + S1 + ch + K[t] + w[t & 15];
        const uint64_t S0 = sha_rotr(a, 28) ^ sha_rotr(a, 34) ^ sha_rotr(a, 39);
        const uint64_t maj = (a & b) ^ (a & c) ^ (b & c);
        const uint64_t t2 = S0 + maj;
        h = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
    }
    return a0 + a;
}

MG_HD uint32_t level_bswap32(uint32_t x) { return (x >> 24) | ((x >> 8) & 0xFF00u) | ((x << 8) & 0xFF0000u) | (x << 24); }

// two little-endian words of a digest -> init_by_array's key: the base-2^32 digits of w0 + w1 * 2^32, [0] for zero
MG_HD int level_key_rule(uint32_t w0, uint32_t w1, uint32_t key[MG_KEY_WORDS]) {
    key[0] = w0;
    key[1] = w1;
    return w1 ? 2 : 1;
}

MG_HD int level_key(int64_t seed, uint32_t key[MG_KEY_WORDS]) {
    const uint64_t h = level_sha512_word0(seed);     // digest bytes 0..7 are h's, most significant first
    return level_key_rule(level_bswap32((uint32_t)(h >> 32)), level_bswap32((uint32_t)h), key);
}

// mt_seed_env (mg_core.h) for a lane that has a memory latency to itself: one row of a sparse call is a chain of 1 870
// dependent steps, and as mt_seed_env walks it every step waits for a load of the array it is filling.  Here the first
// pass (init_genrand) is never stored — its word i is made in a register as the second pass needs it —, the second pass
// only stores, and the third reads what the second stored sixteen words at a time, ahead of the chain.  The same words.
MG_HD void level_seed_mt(const uint32_t* key, int klen, uint32_t* mt, int32_t* mt_pos, uint32_t* head) {
    if (klen < 1) klen = 1;
    if (klen > MG_KEY_WORDS) klen = MG_KEY_WORDS;
    uint32_t g = 19650218u;       // init_genrand(19650218): word 0, then word i as the loop reaches it
    uint32_t prev = g, first = 0;
    int j = 0;
    for (int i = 1; i < MG_MT_N; i++) {
        g = 1812433253u * (g ^ (g >> 30)) + (uint32_t)i;
        const uint32_t v = (g ^ ((prev ^ (prev >> 30)) * 1664525u)) + (j ? key[1] : key[0]) + (uint32_t)j;
        mt[i] = v;
        if (i == 1) first = v;
        prev = v;
        j = j + 1 >= klen ? 0 : j + 1;
    }
    // (the 624th step of that pass is word 1 again; it is rewritten once more by the last step of the next pass: a register)
    first = (first ^ ((prev ^ (prev >> 30)) * 1664525u)) + (j ? key[1] : key[0]) + (uint32_t)j;
    prev = first;
    int i = 2;
    for (; i + 16 <= MG_MT_N; i += 16) {
        uint32_t x[16];
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int u = 0; u < 16; u++) x[u] = mt[i + u];
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int u = 0; u < 16; u++) {
            prev = (x[u] ^ ((prev ^ (prev >> 30)) * 1566083941u)) - (uint32_t)(i + u);
            mt[i + u] = prev;
        }
    }
    for (; i < MG_MT_N; i++) {
        prev = (mt[i] ^ ((prev ^ (prev >> 30)) * 1566083941u)) - (uint32_t)i;
        mt[i] = prev;
    }
    mt[1] = (first ^ ((prev ^ (prev >> 30)) * 1566083941u)) - 1u;
    mt[0] = 0x80000000u;
    // numpy's pos == 624 (nothing generated yet) is pos 0 of the lazy form; then the first head
    int pos = 0;
    for (int h = 0; h < MG_MT_HEAD; h += 8) mt_generate(mt, pos, 8, head + h);
    *mt_pos = pos;
}

// ---- mg_level_seed: one row -------------------------------------------------------------------------------------------
// row i of a call: seeds[i] into bank slot slots[i] (slots null: i), unless mask[i] == 0 (mask null: every row; the
// polarity of mg_reset's env_mask).  A seed below 0 empties the slot and leaves its generator's bytes alone.
MG_HD void level_seed_row(int i, const int64_t* seeds, const int64_t* slots, const uint8_t* mask, int n_slots, uint32_t* bank_mt,
                          int32_t* bank_pos, uint32_t* bank_head, int64_t* bank_seed) {
    if (mask && !mask[i]) return;
    const int64_t slot = slots ? slots[i] : (int64_t)i;
    if (slot < 0 || slot >= (int64_t)n_slots) return;
    const int64_t seed = seeds[i];
    if (seed < 0) { bank_seed[slot] = -1; return; }
    uint32_t key[MG_KEY_WORDS];
    const int klen = level_key(seed, key);
    int32_t pos;
    level_seed_mt(key, klen, bank_mt + (size_t)slot * MG_MT_N, &pos, bank_head + (size_t)slot * MG_MT_HEAD);
    bank_pos[slot] = pos;
    bank_seed[slot] = seed;
}

// ---- mg_level_apply: one env ------------------------------------------------------------------------------------------
enum { kLevelKeep = -2, kLevelFree = -1 };

// What env b does in this launch: kLevelKeep — not selected, nothing changes —, kLevelFree — selected and free-running: it
// keeps its running stream, episode_level = -1 —, or the bank slot (>= 0) whose generator it takes.  `rule`: MG_LEVEL_PENDING —
// selected where the episode has ended, by the predicate the step itself uses on the state the last call left (never the
// done flags: the host rotates them through its buffer sets) —, MG_LEVEL_MASK — where mask[b] != 0, every env without a
// mask —, MG_LEVEL_PUBLISH — none.
MG_HD int level_select(const MgConfig& cfg, const MgState& st, int b, int rule, const uint8_t* mask, const int64_t* level_of_env,
                       int n_slots, const int64_t* bank_seed) {
    bool sel = false;
    if (rule == MG_LEVEL_PENDING) sel = episode_ended(cfg, st.agents + (size_t)b * cfg.n_agents, 1, 0, st.step_count[b]);
    else if (rule == MG_LEVEL_MASK) sel = !mask || mask[b] != 0;
    if (!sel) return kLevelKeep;
    const int64_t lv = level_of_env[b];
    if (lv < 0 || lv >= (int64_t)n_slots || bank_seed[lv] < 0) return kLevelFree;
    return (int)lv;
}

struct alignas(16) LevelVec { uint32_t x, y, z, w; };
constexpr int kLevelMtVecs = MG_MT_N * 4 / 16;            // 156: a generator's 2 496 bytes
constexpr int kLevelHeadVecs = MG_MT_HEAD * 4 / 16;       // 4: the 64-byte head
constexpr int kLevelItems = kLevelMtVecs + kLevelHeadVecs + 1;   // ... and mt_pos

// mg_level_apply_rows: what a level holds besides its generator — the slot's row of the parameter table (MG_GEN_DRAWS bytes)
// and its K edit entries (4 bytes each) —, and the env's tables they are copied into (the tails of the buffer a reset program's
// template_grid points into, marlgrid_hip.h).  A null pair: that part is not copied.  Rows of 32-bit words behind 4-byte
// aligned bases.
struct LevelRows {
    const uint32_t* bank_params = nullptr;      // [L][MG_GEN_DRAWS / 4]
    uint32_t* env_params = nullptr;             // [B][MG_GEN_DRAWS / 4]
    const uint32_t* bank_edits = nullptr;       // [L][K]
    uint32_t* env_edits = nullptr;              // [B][K]
    int K = 0;
};
constexpr int kLevelParamWords = MG_GEN_DRAWS / 4;

// Bank row `slot` -> env b's generator, items lane, lane + lanes, ...: 16-byte loads and stores (rows of 2 496 and 64
// bytes behind 16-byte aligned bases).  A wave calls it with its 64 lanes, the host with (0, 1).  With `rows` the slot's
// parameter row and edit rows are further items of the same loop: 8 + 4 K bytes, a 32-bit word each.
MG_HD void level_copy(const MgState& st, int b, int slot, const uint32_t* bank_mt, const int32_t* bank_pos, const uint32_t* bank_head,
                      int lane, int lanes, const LevelRows* rows = nullptr) {
    const LevelVec* src_mt = reinterpret_cast<const LevelVec*>(bank_mt + (size_t)slot * MG_MT_N);
    const LevelVec* src_head = reinterpret_cast<const LevelVec*>(bank_head + (size_t)slot * MG_MT_HEAD);
    LevelVec* dst_mt = reinterpret_cast<LevelVec*>(st.mt + (size_t)b * MG_MT_N);
    LevelVec* dst_head = reinterpret_cast<LevelVec*>(st.mt_head + (size_t)b * MG_MT_HEAD);
    const int K = rows && rows->bank_edits ? rows->K : 0;
    const int items = kLevelItems + (rows ? kLevelParamWords + K : 0);
    for (int i = lane; i < items; i += lanes) {
        if (i < kLevelMtVecs) dst_mt[i] = src_mt[i];
        else if (i < kLevelMtVecs + kLevelHeadVecs) dst_head[i - kLevelMtVecs] = src_head[i - kLevelMtVecs];
        else if (i == kLevelItems - 1) st.mt_pos[b] = bank_pos[slot];
        else if (i < kLevelItems + kLevelParamWords) {
            const int w = i - kLevelItems;
            if (rows->bank_params) rows->env_params[(size_t)b * kLevelParamWords + w] = rows->bank_params[(size_t)slot * kLevelParamWords + w];
        } else {
            const int w = i - kLevelItems - kLevelParamWords;
            rows->env_edits[(size_t)b * K + w] = rows->bank_edits[(size_t)slot * K + w];
        }
    }
}

// the env's own lane, last: the level of the running episode, and this call's copy of it.  An env that takes a level also
// turns its agents to heading 0: a reset keeps every agent's heading (the reference's agent objects outlive reset()), and a
// level that started from whatever the last episode left would not be the same level twice — it starts as it does in an
// env made for it, `MultiGridEnv(seed=s)` and nothing else before the reset.
MG_HD void level_publish(const MgConfig& cfg, const MgState& st, int b, int what, const int64_t* bank_seed, int64_t* episode_level,
                         int64_t* out_level) {
    int64_t lv;
    if (what == kLevelKeep) lv = episode_level[b];
    else episode_level[b] = lv = what == kLevelFree ? (int64_t)-1 : bank_seed[what];
    if (what >= 0)
        for (int k = 0; k < cfg.n_agents; k++) {
            uint64_t* r = st.agents + (size_t)b * cfg.n_agents + k;
            *r = rec_set(*r, MG_AG_DIR, 0);
        }
    if (out_level) out_level[b] = lv;
}

}  // namespace mg
