// TEST INFRASTRUCTURE — a stand-alone program around tests/native/mg_memory.cpp (and mg_explore.cpp) for a sanitizer build
// (tests/test_memory_sanitized.py: g++ -fsanitize=address,undefined -fno-sanitize-recover=all): random grids, agent records and
// hide tables from a seed, W and H from 1 to 40 and 255, views 3 to 31, every buffer of the exact size.  Three observations per
// case (a fresh one, a masked one, one of every env) through mem_update; checked after each: the four exploration tensors
// against ex_update on buffers of its own, the invariants between the six, and the dword of every cell stamped in this
// observation against the hide rules written out here, the plain way.  Exit code 0 and "ok <cases>" on the last line, or 1 and
// the first mismatch.  Usage: prog <seed> <cases>
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "mg_explore.cpp"
#include "mg_memory.cpp"

namespace {

struct Rng {
    uint64_t s;
    uint32_t next() {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)(s >> 33);
    }
    int below(int n) { return (int)(next() % (uint32_t)n); }
};

// grid.get after hide_item_types for viewer k at (x, y) (base.py:441-449, 547-552), then WorldObj.encode
uint32_t plain_triple(const MgConfig& cfg, const std::vector<MgObjDesc>& obj, const std::vector<uint32_t>& hide, uint32_t base,
                      const uint64_t* rec, int n, int k, int x, int y) {
    std::vector<std::pair<int, int>> here;      // (rank, agent) of the placed agents of the cell
    for (int j = 0; j < n; j++) {
        const int fl = (int)((rec[j] >> (8 * MG_AG_FLAGS)) & 0xFF);
        if ((fl & MG_AF_PLACED) && (int)(rec[j] & 0xFF) == x && (int)((rec[j] >> 8) & 0xFF) == y)
            here.push_back({(int)((rec[j] >> (8 * MG_AG_RANK)) & 0xFF), j});
    }
    std::sort(here.begin(), here.end());
    int a = -1;
    if (base != 0) {
        const bool hidden = base < obj.size() && ((hide[base] >> k) & 1u);
        if (!hidden) {
            if (base >= obj.size()) return 0;
            return (uint32_t)obj[base].type_idx | ((uint32_t)obj[base].color_idx << 8) | ((uint32_t)obj[base].state << 16);
        }
        if (!here.empty()) a = here[0].second;
    } else if (!here.empty()) {
        a = here[0].second;
        if (a != k && ((cfg.hide_agent_mask >> k) & 1u)) a = here.size() > 1 ? here[1].second : -1;
    }
    if (a < 0) return 0;
    return (uint32_t)cfg.agent_type_idx | ((uint32_t)cfg.agent_color_idx[a] << 8) | (uint32_t)(((rec[a] >> (8 * MG_AG_DIR)) & 0xFF) << 16);
}

#define FAIL(...) do { printf("case %d obs %d: ", c, obs); printf(__VA_ARGS__); printf("\n"); return 1; } while (0)

}  // namespace

int main(int argc, char** argv) {
    const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
    const int cases = argc > 2 ? atoi(argv[2]) : 100;
    Rng rng{seed * 2654435761ull + 12345};
    for (int c = 0; c < cases; c++) {
        const int W = (c % 9 == 0) ? 255 : ((c % 7 == 0) ? (c / 7) % 40 + 1 : rng.below(40) + 1);
        const int H = (c % 9 == 4) ? 255 : ((c % 7 == 1) ? (c / 7) % 40 + 1 : rng.below(40) + 1);
        const int VS = (c % 5 == 0) ? 3 + (c / 5) % 29 : 3 + rng.below(29);
        const int n = 1 + rng.below(5), B = 1 + rng.below(4), cells = W * H, n_obj = 2 + rng.below(9);
        const int block = (c % 3 == 0) ? 256 : ((c % 3 == 1) ? 64 : 1), wave = (c % 2) ? 64 : 7, rt = c % 4 == 2;
        std::vector<MgObjDesc> obj(n_obj);
        memset(obj.data(), 0, sizeof(MgObjDesc) * n_obj);
        std::vector<uint32_t> hide(n_obj, 0u);
        for (int o = 1; o < n_obj; o++) {
            obj[o].type_idx = (uint8_t)(1 + rng.below(11));
            obj[o].color_idx = (uint8_t)rng.below(6);
            obj[o].state = (uint8_t)rng.below(3);
            obj[o].flags = rng.below(2) ? MG_OF_SEE_BEHIND : 0;
            if (rng.below(3) == 0) hide[o] = rng.next() & ((1u << n) - 1u);
        }
        MgConfig cfg;
        memset(&cfg, 0, sizeof(cfg));
        cfg.B = B; cfg.n_agents = n; cfg.W = W; cfg.H = H; cfg.cells_stride = cells;
        cfg.view_size = VS; cfg.view_offset = rng.below(3) == 0 ? rng.below(VS / 2 + 1) : 0;
        cfg.see_through_walls = rng.below(5) == 0;
        cfg.n_obj = n_obj; cfg.obj = obj.data();
        cfg.any_hide = c % 6 != 5; cfg.hide_by_obj = (c % 6 == 4) ? nullptr : hide.data();
        cfg.hide_agent_mask = rng.below(2) ? rng.next() & ((1u << n) - 1u) : 0u;
        cfg.agent_type_idx = 12;
        for (int j = 0; j < n; j++) cfg.agent_color_idx[j] = (uint8_t)rng.below(6);
        const bool hides_objects = cfg.any_hide && cfg.hide_by_obj;
        const std::vector<uint32_t> no_hide(n_obj, 0u);
        // a view group of some of the agents, or (n_view 0) all of them
        std::vector<int> viewers;
        if (rng.below(3) == 0) {
            for (int j = 0; j < n; j++) if (rng.below(2)) { cfg.view_agent[cfg.n_view++] = (uint8_t)j; }
            if (cfg.n_view == 0) cfg.view_agent[cfg.n_view++] = (uint8_t)rng.below(n);
        }
        for (int v = 0; v < (cfg.n_view ? cfg.n_view : n); v++) viewers.push_back(cfg.n_view ? cfg.view_agent[v] : v);

        std::vector<uint8_t> grid((size_t)B * cells), seen((size_t)B * n * cells, 0x5A), seen2(seen), mask(B);
        std::vector<uint64_t> rec((size_t)B * n);
        std::vector<int32_t> sc(B), visits((size_t)B * n * cells, 0x5A5A), visits2(visits), nc((size_t)B * n, -7), nc2(nc), vc(nc), vc2(nc);
        std::vector<uint32_t> memory((size_t)B * n * cells, 0x5A5A5A5Au);
        std::vector<int32_t> stamp((size_t)B * n * cells, 0x5A5A);
        MgState st;
        memset(&st, 0, sizeof(st));
        st.grid = grid.data(); st.agents = rec.data(); st.step_count = sc.data();
        for (int obs = 0; obs < 3; obs++) {
            for (auto& g : grid) g = (uint8_t)(rng.below(3) ? 0 : (rng.below(20) ? rng.below(n_obj) : rng.below(256)));
            for (int b = 0; b < B; b++) {
                std::vector<int> rank(n);
                for (int j = 0; j < n; j++) rank[j] = j;
                for (int j = n - 1; j > 0; j--) std::swap(rank[j], rank[rng.below(j + 1)]);
                const int hx = rng.below(W), hy = rng.below(H);         // where agents crowd: stacks
                for (int j = 0; j < n; j++) {
                    const bool crowd = rng.below(2);
                    const int x = crowd ? hx : rng.below(W), y = crowd ? hy : rng.below(H);
                    const int fl = (rng.below(6) ? MG_AF_ACTIVE : 0) | (rng.below(8) ? MG_AF_PLACED : 0);
                    rec[(size_t)b * n + j] = (uint64_t)x | ((uint64_t)y << 8) | ((uint64_t)rng.below(4) << 16) | ((uint64_t)fl << 24) |
                                             ((uint64_t)rank[j] << (8 * MG_AG_RANK));
                }
                sc[b] = obs;                                            // obs 0: every env is fresh, and the sentinels go
                mask[b] = obs == 1 ? (uint8_t)rng.below(2) : 1;
            }
            const uint8_t* m = obs == 1 ? mask.data() : nullptr;
            const std::vector<uint32_t> memory0(memory);
            const std::vector<int32_t> stamp0(stamp);
            int pb = 0, lds = 0;
            if (mem_update(&cfg, &st, m, seen.data(), visits.data(), nc.data(), vc.data(), reinterpret_cast<uint8_t*>(memory.data()),
                           stamp.data(), block, wave, rt, &pb, &lds) != 0) FAIL("mem_update failed");
            if (ex_update(&cfg, &st, m, seen2.data(), visits2.data(), nc2.data(), vc2.data(), block, wave, rt, nullptr) != 0) FAIL("ex_update failed");
            if (seen != seen2 || visits != visits2 || nc != nc2 || vc != vc2) FAIL("the two entry points disagree on the exploration tensors");
            for (int b = 0; b < B; b++)
                for (int k = 0; k < n; k++) {
                    const bool mine = std::find(viewers.begin(), viewers.end(), k) != viewers.end();
                    for (int i = 0; i < cells; i++) {
                        const size_t at = ((size_t)b * n + k) * cells + i;
                        if (!mine || !mask[b]) {
                            if (memory[at] != memory0[at] || stamp[at] != stamp0[at]) FAIL("env %d agent %d cell %d: not this launch's, and written", b, k, i);
                            continue;
                        }
                        if ((memory[at] >> 24) != seen[at] || (stamp[at] >= 0) != (seen[at] != 0) || seen[at] > 1)
                            FAIL("env %d agent %d cell %d: memory %08x, seen_step %d, seen %d", b, k, i, memory[at], stamp[at], seen[at]);
                        if (!seen[at] && (memory[at] != 0 || stamp[at] != -1)) FAIL("env %d agent %d cell %d: never seen, %08x %d", b, k, i, memory[at], stamp[at]);
                        if (stamp[at] > sc[b]) FAIL("env %d agent %d cell %d: stamped %d at step %d", b, k, i, stamp[at], sc[b]);
                        if (stamp[at] == sc[b]) {
                            const uint32_t want = plain_triple(cfg, obj, hides_objects ? hide : no_hide, grid[(size_t)b * cells + i],
                                                               rec.data() + (size_t)b * n, n, k, i / H, i % H) | (1u << 24);
                            if (memory[at] != want) FAIL("env %d agent %d cell (%d, %d): memory %08x, want %08x", b, k, i / H, i % H, memory[at], want);
                        } else if (sc[b] == 0 ? (memory[at] != 0 || stamp[at] != -1) : (memory[at] != memory0[at] || stamp[at] != stamp0[at])) {
                            FAIL("env %d agent %d cell %d: not seen in this observation, and neither cleared (step 0) nor kept", b, k, i);
                        }
                    }
                }
        }
    }
    printf("ok %d\n", cases);
    return 0;
}
