// TEST INFRASTRUCTURE — a stand-alone program around tests/native/mg_goal_dist.cpp for a sanitizer build
// (tests/test_goal_distance_sanitized.py: g++ -fsanitize=address,undefined -fno-sanitize-recover=all): random grids from a seed,
// every emulated path against a queue search written here.  Exit code 0 and "ok <cases>" on the last line, or 1 and the first
// mismatch.  Usage: prog <seed> <cases>
#include <stdio.h>

#include <deque>
#include <vector>

#include "mg_goal_dist.cpp"

namespace {

struct Rng {
    uint64_t s;
    uint32_t next() {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)(s >> 33);
    }
    int below(int n) { return (int)(next() % (uint32_t)n); }
};

enum { kWall = 1, kGoal = 2, kLava = 3, kFloor = 4, kKinds = 5 };
const int DX[4] = {1, 0, -1, 0}, DY[4] = {0, 1, 0, -1};

// every state's distance by a reverse queue search: the definition of mg_goal_core.h
std::vector<int32_t> reference(int W, int H, const std::vector<uint8_t>& grid) {
    auto free_at = [&](int x, int y) { const uint8_t v = grid[(size_t)x * H + y]; return v == 0 || v == kFloor; };
    auto goal_at = [&](int x, int y) { return grid[(size_t)x * H + y] == kGoal; };
    std::vector<int32_t> dist((size_t)W * H * 4, -1);
    std::deque<int> q;
    for (int x = 0; x < W; x++)
        for (int y = 0; y < H; y++) {
            if (!free_at(x, y) && !goal_at(x, y)) continue;
            for (int d = 0; d < 4; d++) {
                const int fx = x + DX[d], fy = y + DY[d];
                if (fx >= 0 && fx < W && fy >= 0 && fy < H && goal_at(fx, fy)) {
                    dist[((size_t)x * H + y) * 4 + d] = 1;
                    q.push_back((x * H + y) * 4 + d);
                }
            }
        }
    while (!q.empty()) {
        const int s = q.front();
        q.pop_front();
        const int d = s & 3, y = (s >> 2) % H, x = (s >> 2) / H;
        const int32_t k = dist[s] + 1;
        for (int nd : {(d + 3) & 3, (d + 1) & 3}) {
            const int t = (x * H + y) * 4 + nd;
            if (dist[t] < 0) { dist[t] = k; q.push_back(t); }
        }
        if (free_at(x, y)) {
            const int px = x - DX[d], py = y - DY[d];
            if (px >= 0 && px < W && py >= 0 && py < H && (free_at(px, py) || goal_at(px, py))) {
                const int t = (px * H + py) * 4 + d;
                if (dist[t] < 0) { dist[t] = k; q.push_back(t); }
            }
        }
    }
    return dist;
}

}  // namespace

int main(int argc, char** argv) {
    const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
    const int cases = argc > 2 ? atoi(argv[2]) : 200;
    Rng rng{seed * 2654435761ull + 12345};
    MgObjDesc obj[kKinds];
    memset(obj, 0, sizeof(obj));
    obj[kGoal].flags = MG_OF_CAN_OVERLAP | MG_OF_ENDS_EPISODE;
    obj[kGoal].reward_kind = 1;
    obj[kLava].flags = MG_OF_CAN_OVERLAP | MG_OF_ENDS_EPISODE;
    obj[kFloor].flags = MG_OF_CAN_OVERLAP;
    const int tall[4] = {64, 65, 128, 255};
    for (int c = 0; c < cases; c++) {
        // W and H from 1 to 70, the word boundaries among them; every fourth case one of the tall grids
        const int W = (c % 7 == 0) ? (c / 7) % 70 + 1 : rng.below(70) + 1;
        const int H = (c % 4 == 3) ? tall[(c / 4) % 4] : ((c % 7 == 1) ? (c / 7) % 70 + 1 : rng.below(70) + 1);
        const int B = 2, n = 3, stride = (W * H + 15) / 16 * 16;
        std::vector<uint8_t> grid((size_t)B * stride, 0);
        std::vector<uint64_t> rec((size_t)B * n);
        const int density = rng.below(4);       // walls: none, few, some, many
        for (int b = 0; b < B; b++) {
            for (int i = 0; i < W * H; i++) {
                const int r = rng.below(20);
                grid[(size_t)b * stride + i] = r < density * 3 ? kWall : r == 17 ? kLava : r == 18 ? kFloor : r == 19 ? 200 : 0;
            }
            for (int g = rng.below(3); g > 0; g--) grid[(size_t)b * stride + rng.below(W * H)] = kGoal;
            for (int k = 0; k < n; k++) {
                const uint64_t flags = k == 2 && b == 1 ? MG_AF_DONE : (MG_AF_ACTIVE | MG_AF_PLACED);
                rec[(size_t)b * n + k] = (uint64_t)rng.below(W) | ((uint64_t)rng.below(H) << 8) | ((uint64_t)rng.below(4) << 16) | (flags << 24);
            }
        }
        MgConfig cfg;
        memset(&cfg, 0, sizeof(cfg));
        cfg.B = B; cfg.W = W; cfg.H = H; cfg.n_agents = n; cfg.cells_stride = stride; cfg.n_obj = kKinds; cfg.obj = obj;
        MgState st;
        memset(&st, 0, sizeof(st));
        st.grid = grid.data();
        st.agents = rec.data();
        std::vector<int32_t> want_field, want_dist((size_t)B * n, -1);
        for (int b = 0; b < B; b++) {
            const std::vector<uint8_t> gb(grid.begin() + (size_t)b * stride, grid.begin() + (size_t)b * stride + W * H);
            const std::vector<int32_t> f = reference(W, H, gb);
            want_field.insert(want_field.end(), f.begin(), f.end());
            for (int k = 0; k < n; k++) {
                // (the record decoded here, not by the code under test: x, y, dir, flags in bytes 0 .. 3)
                const uint64_t r = rec[(size_t)b * n + k];
                const int ax = (int)(r & 0xFF), ay = (int)((r >> 8) & 0xFF), ad = (int)((r >> 16) & 3), fl = (int)((r >> 24) & 0xFF);
                if ((fl & MG_AF_ACTIVE) && !(fl & MG_AF_EVICTED) && ax < W && ay < H)
                    want_dist[(size_t)b * n + k] = f[((size_t)ax * H + ay) * 4 + ad];
            }
        }
        for (int path = 0; path < 3; path++) {      // general at 64 lanes, at 1, register-resident
            if (path == 2 && !mg::goal_reg_fits(W, H)) continue;
            for (int with_field = 0; with_field < 2; with_field++) {
                // exact-size heap blocks: a store one entry past an env's rows is the sanitizer's to catch
                std::vector<int32_t> dist((size_t)B * n, -7), field(with_field ? (size_t)B * W * H * 4 : 0, -7);
                int32_t* fp = with_field ? field.data() : nullptr;
                const int rc = path == 2 ? gd_reg(&cfg, &st, nullptr, dist.data(), fp) : gd_general(&cfg, &st, nullptr, dist.data(), fp, path == 0 ? 64 : 1);
                if (rc != 0 || dist != want_dist || (with_field && field != want_field)) {
                    printf("MISMATCH case %d W %d H %d path %d field %d rc %d\n", c, W, H, path, with_field, rc);
                    return 1;
                }
            }
        }
    }
    printf("ok %d\n", cases);
    return 0;
}
