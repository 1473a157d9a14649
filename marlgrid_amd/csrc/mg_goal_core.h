// mg_goal_core.h — goal distance: the bodies of mg_goal_distance (mg_goal_dist.hip) as plain inline functions, like
// mg_level_core.h: the same text compiles with g++ for the host tests (tests/native/mg_goal_dist.cpp).
//
// The question, per env: from the state (x, y, dir), what is the smallest number of actions `left`, `right`, `forward`
// (marlgrid/base.py:530-585) after which a `forward` ENTERS a goal cell — on the env's grid as it is, other agents ignored,
// nothing toggled, picked up or dropped.  Cells by their grid byte, an id into cfg.obj[]:
//   goal     reward_kind == 1 and MG_OF_ENDS_EPISODE;
//   free     id 0, or MG_OF_CAN_OVERLAP without MG_OF_ENDS_EPISODE (floor, bonus tiles, open doors);
//   blocked  everything else (walls, keys, balls, boxes, closed and locked doors, lava), and every id >= n_obj.
// Entering a goal ends the agent's episode: goal cells are never passed through, and an agent that STANDS on one has not
// entered it — it may turn there and leave.  Nothing wraps: outside the grid is blocked.
//
// A level-synchronous REVERSE search over bit planes.  plane[dir][x] holds the cells of column x along y as bits, H <= 255 a
// chain of NW = ceil(H / 64) 64-bit words (grid index x * H + y: a column is contiguous bytes).  With open = free | goal:
//   level 1    = open & (goal one step ahead)
//   level k+1  = open & ~visited & (level k of dir - 1 | level k of dir + 1 | (level k & free) one step ahead)
// "one step ahead" along +-y is a shift inside the chain, along +-x the neighbouring column's word, a turn is an OR between
// planes, and the far side of the grid's edge falls out as zeros.  No shift is ever by the word width.  The level at which a
// state's bit first appears is its distance; a state that never appears has none (-1).
#pragma once

#if !defined(__HIPCC_RTC__)   // (a run-time compile — mg_rtc.hip — has no system headers: its source supplies these names)
#include <stddef.h>
#include <stdint.h>
#endif

#include "mg_core.h"

namespace mg {

enum { kGoalBlocked = 0, kGoalFree = 1, kGoalGoal = 2 };
enum { kGoalPathAuto = 0, kGoalPathReg = 1, kGoalPathLds = 2 };      // mg_goal_distance_path's `path`

MG_HD int goal_cell_kind(const MgConfig& cfg, uint32_t id) {
    if (id == 0) return kGoalFree;
    if (id >= (uint32_t)cfg.n_obj) return kGoalBlocked;
    const uint32_t flags = cfg.obj[id].flags;
    if (flags & MG_OF_ENDS_EPISODE) return cfg.obj[id].reward_kind == 1 ? kGoalGoal : kGoalBlocked;
    return (flags & MG_OF_CAN_OVERLAP) ? kGoalFree : kGoalBlocked;
}

// rows y0, y0 + ystep, ... below y1 of column x -> their bits of the column's word that starts at row `base`
MG_HD void goal_column_bits(const MgConfig& cfg, const uint8_t* grid_b, int x, int base, int y0, int ystep, int y1, uint64_t* free_w,
                            uint64_t* goal_w) {
    uint64_t f = 0, g = 0;
    const uint8_t* col = grid_b + (size_t)x * cfg.H;
    for (int y = y0; y < y1; y += ystep) {
        const int kind = goal_cell_kind(cfg, col[y]);
        const uint64_t bit = 1ull << (y - base);
        if (kind == kGoalFree) f |= bit;
        else if (kind == kGoalGoal) g |= bit;
    }
    *free_w = f;
    *goal_w = g;
}

// the rows of word w that exist: H - 64 w of them, at most 64
MG_HD uint64_t goal_row_mask(int H, int w) {
    const int n = H - 64 * w;
    return n >= 64 ? ~0ull : (n <= 0 ? 0ull : (1ull << n) - 1ull);
}

// "one step ahead" for direction d, as a word of the states that look there: bit y of the answer is the cell (x, y) + dirvec(d).
// xp / xm: the same word of columns x + 1 / x - 1 (0 outside the grid); above / below: the next / previous word of the column's
// own chain (0 past its ends).
MG_HD uint64_t goal_ahead_word(int d, uint64_t self, uint64_t xp, uint64_t xm, uint64_t above, uint64_t below) {
    switch (d & 3) {
    case 0: return xp;
    case 1: return (self >> 1) | (above << 63);
    case 2: return xm;
    default: return (self << 1) | (below >> 63);
    }
}

MG_HD uint64_t goal_next_word(uint64_t open_w, uint64_t visited, uint64_t turn_a, uint64_t turn_b, uint64_t ahead) {
    return open_w & ~visited & (turn_a | turn_b | ahead);
}

// field[x][y][d] = value for the set bits of word w of plane (d, x); field_b: the env's [W][H][4]
MG_HD void goal_field_store(int32_t* field_b, int H, int x, int w, int d, uint64_t bits, int32_t value) {
    while (bits) {
        const int y = 64 * w + __builtin_ctzll(bits);
        bits &= bits - 1;
        field_b[((size_t)x * H + y) * 4 + d] = value;
    }
}

// An agent's state, if it is in a cell: active, not MG_AF_EVICTED, inside the grid.  (Not active: not yet spawned, or done.)
struct GoalAgent { int x, y, d, in_cell; };
MG_HD GoalAgent goal_agent(const MgConfig& cfg, uint64_t r) {
    GoalAgent a;
    const uint32_t flags = rec_byte(r, MG_AG_FLAGS);
    a.x = (int)rec_byte(r, MG_AG_X);
    a.y = (int)rec_byte(r, MG_AG_Y);
    a.d = (int)rec_byte(r, MG_AG_DIR) & 3;
    a.in_cell = ((flags & MG_AF_ACTIVE) && !(flags & MG_AF_EVICTED) && a.x < cfg.W && a.y < cfg.H) ? 1 : 0;
    return a;
}

MG_HD int goal_max_levels(int W, int H) { return 4 * W * H + 1; }

// ---- the general path: every W, H <= 255, planes in scratch memory (LDS on the device) -----------------------------------
// Words, WN = W * NW per plane set: free [WN], goal [WN], visited [4 WN], two frontiers [4 WN] each, index (d * W + x) * NW + w;
// then the agents' labels.  14 * 8 * 1020 + 128 = 114 368 bytes at 255 x 255.
struct GoalScratch {
    uint64_t *free_w, *goal_w, *visited, *front, *next;
    int32_t* adist;     // [MG_MAX_AGENTS]
    int W, H, NW, WN;
};

MG_HD int goal_words(int H) { return (H + 63) >> 6; }
MG_HD size_t goal_scratch_bytes(int W, int H) { return (size_t)14 * 8 * W * goal_words(H) + 4 * MG_MAX_AGENTS; }

MG_HD GoalScratch goal_scratch(void* base, int W, int H) {
    GoalScratch s;
    s.W = W;
    s.H = H;
    s.NW = goal_words(H);
    s.WN = W * s.NW;
    s.free_w = static_cast<uint64_t*>(base);
    s.goal_w = s.free_w + s.WN;
    s.visited = s.goal_w + s.WN;
    s.front = s.visited + 4 * s.WN;
    s.next = s.front + 4 * s.WN;
    s.adist = reinterpret_cast<int32_t*>(s.next + 4 * s.WN);
    return s;
}

// word (x, w) of a [W][NW] map, 0 outside it
MG_HD uint64_t goal_map_word(const uint64_t* m, const GoalScratch& s, int x, int w) {
    return (x < 0 || x >= s.W || w < 0 || w >= s.NW) ? 0ull : m[x * s.NW + w];
}

// Every function below is one PHASE for the items lane, lane + lanes, ...: a wave calls it with its 64 lanes and hands the
// scratch over between phases (mg_device.h: wave_lds_sync), the host runs the lanes of a phase one after the other — with 64
// lanes and with 1.  A phase reads only what earlier phases wrote, or what its own item wrote.

// phase 1: the free and goal maps of env b's grid, and the agents' labels to -1
MG_HD void goal_gen_build(const MgConfig& cfg, const uint8_t* grid_b, const GoalScratch& s, int lane, int lanes) {
    for (int i = lane; i < s.WN; i += lanes) {
        const int x = i / s.NW, w = i - x * s.NW;
        const int y1 = s.H < 64 * (w + 1) ? s.H : 64 * (w + 1);
        goal_column_bits(cfg, grid_b, x, 64 * w, 64 * w, 1, y1, s.free_w + i, s.goal_w + i);
    }
    for (int k = lane; k < MG_MAX_AGENTS; k += lanes) s.adist[k] = -1;
}

// the candidates of plane (d, x), word w, from the frontier `src` (null: level 1, the goal map itself)
MG_HD uint64_t goal_gen_word(const GoalScratch& s, const uint64_t* src, int d, int x, int w) {
    const int i = x * s.NW + w;
    const uint64_t open_w = s.free_w[i] | s.goal_w[i];
    if (!src) {
        const uint64_t* g = s.goal_w;
        return open_w & goal_ahead_word(d, g[i], goal_map_word(g, s, x + 1, w), goal_map_word(g, s, x - 1, w),
                                        goal_map_word(g, s, x, w + 1), goal_map_word(g, s, x, w - 1));
    }
    // (the frontier's states that stand on a free cell: a goal cell is entered, never crossed)
    const uint64_t* f = src + (size_t)d * s.WN;
    const uint64_t self = f[i] & s.free_w[i];
    const uint64_t xp = goal_map_word(f, s, x + 1, w) & goal_map_word(s.free_w, s, x + 1, w);
    const uint64_t xm = goal_map_word(f, s, x - 1, w) & goal_map_word(s.free_w, s, x - 1, w);
    const uint64_t above = goal_map_word(f, s, x, w + 1) & goal_map_word(s.free_w, s, x, w + 1);
    const uint64_t below = goal_map_word(f, s, x, w - 1) & goal_map_word(s.free_w, s, x, w - 1);
    return goal_next_word(open_w, s.visited[(size_t)d * s.WN + i], src[(size_t)((d + 1) & 3) * s.WN + i],
                          src[(size_t)((d + 3) & 3) * s.WN + i], goal_ahead_word(d, self, xp, xm, above, below));
}

// phase 2 (src null, level 1) and the level loop's first half: dst = the states first reached at `level`, visited |= dst,
// their field entries.  Returns whether this lane found any.
MG_HD bool goal_gen_expand(const GoalScratch& s, const uint64_t* src, uint64_t* dst, int level, int32_t* field_b, int lane, int lanes) {
    bool any = false;
    for (int i = lane; i < 4 * s.WN; i += lanes) {
        const int d = i / s.WN, r = i - d * s.WN;
        const int x = r / s.NW, w = r - x * s.NW;
        const uint64_t nw = goal_gen_word(s, src, d, x, w);
        dst[i] = nw;
        s.visited[i] = src ? (s.visited[i] | nw) : nw;
        if (nw) {
            any = true;
            if (field_b) goal_field_store(field_b, s.H, x, w, d, nw, level);
        }
    }
    return any;
}

// the level loop's second half: agents lane, lane + lanes, ... look their state up in the new frontier.  Returns whether one of
// them is in a cell and still without a label.
MG_HD bool goal_gen_agents(const MgConfig& cfg, const uint64_t* rec_b, const GoalScratch& s, const uint64_t* frontier, int level, int lane,
                           int lanes) {
    bool pending = false;
    for (int k = lane; k < cfg.n_agents; k += lanes) {
        const GoalAgent a = goal_agent(cfg, rec_b[k]);
        if (!a.in_cell || s.adist[k] >= 0) continue;
        const uint64_t word = frontier[((size_t)a.d * s.W + a.x) * s.NW + (a.y >> 6)];
        if ((word >> (a.y & 63)) & 1ull) s.adist[k] = level;
        else pending = true;
    }
    return pending;
}

// last phase: the labels, and -1 into the field for every state that was never reached (each entry is written once)
MG_HD void goal_gen_finish(const MgConfig& cfg, const GoalScratch& s, int32_t* dist_b, int32_t* field_b, int lane, int lanes) {
    for (int k = lane; k < cfg.n_agents; k += lanes) dist_b[k] = s.adist[k];
    if (!field_b) return;
    for (int i = lane; i < 4 * s.WN; i += lanes) {
        const int d = i / s.WN, r = i - d * s.WN;
        const int x = r / s.NW, w = r - x * s.NW;
        goal_field_store(field_b, s.H, x, w, d, ~s.visited[i] & goal_row_mask(s.H, w), -1);
    }
}

// ---- the register-resident path: 4 W <= 64 and H <= 64 ---------------------------------------------------------------------
// Lane d * W + x holds plane (d, x) as one 64-bit value; turns and +-x steps are reads of another lane's value.  What a lane
// computes is here; the exchange between lanes is the kernel's (cross-lane reads) and the host twin's (arrays).
MG_HD bool goal_reg_fits(int W, int H) { return 4 * W <= 64 && H <= 64; }

// the lane whose frontier word lane (d, x) reads for its turn by `by` (+1 / +3) ...
MG_HD int goal_reg_turn_lane(int W, int d, int x, int by) { return ((d + by) & 3) * W + x; }
// ... and for its step ahead along +-x: *ok = 0 where that column is outside the grid (directions 1 and 3 read their own word)
MG_HD int goal_reg_ahead_lane(int W, int d, int x, int* ok) {
    const int nx = d == 0 ? x + 1 : (d == 2 ? x - 1 : x);
    *ok = (nx >= 0 && nx < W) ? 1 : 0;
    return *ok ? d * W + nx : d * W + x;
}

// lane (d, x)'s new frontier word: `turn_a` / `turn_b` the frontier words of the turn lanes, `mine` its own, `got` the word
// (frontier & free) of the ahead lane — for level 1 the goal word of that column, with `mine` the lane's own goal word
MG_HD uint64_t goal_reg_word(int d, uint64_t open_w, uint64_t visited, uint64_t turn_a, uint64_t turn_b, uint64_t mine, uint64_t got, int ok) {
    const uint64_t side = ok ? got : 0ull;
    return goal_next_word(open_w, visited, turn_a, turn_b, goal_ahead_word(d, mine, side, side, 0ull, 0ull));
}

}  // namespace mg
