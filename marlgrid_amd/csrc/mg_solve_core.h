// mg_solve_core.h — solve distance: the bodies of mg_solve_distance (mg_solve_dist.hip) as plain inline functions, like
// mg_goal_core.h: the same text compiles with g++ for the host tests (tests/native/mg_solve_dist.cpp).
//
// The question, per agent of an env: the smallest number of actions `left` (0), `right` (1), `forward` (2), `pickup` (3) and
// `toggle` (5) after which the agent's `forward` ENTERS a goal cell — on the env's grid as it is, the agent carrying what it
// carries, other agents ignored, under the step's rules (mg_core.h: step_agents).  `drop` and `done` are never used, so an
// agent picks up at most one object: two locked doors of two colours have no path.  Cells are mg_goal_core.h's free / goal /
// blocked; what is new is that a blocked cell can become free:
//   item       a blocked cell whose object has MG_OF_CAN_PICKUP: `pickup` with empty hands empties it (cost 1);
//   shut door  a blocked cell whose object has MG_OF_IS_DOOR without MG_OF_CAN_OVERLAP and MG_OF_IS_BOX.  A closed one is
//              opened by one `toggle` (-> toggle_next), a locked one by two (-> unlock_next, a closed door, -> its toggle_next)
//              by an agent that holds an MG_OF_IS_KEY object of the door's color_idx.  A door counts as openable only if the
//              id it ends as is a free cell (and, locked, only if unlock_next is a closed door); it is never closed again.
// The first max_doors shut doors and the first max_items items of the grid in index order x * H + y are TRACKED; the others
// block and are never touched (the result is then an upper bound, and `exact` is 0).  An agent that already carries something
// tracks no item.
//
// A LAYER is (set S of tracked doors opened, tracked item picked up or none): index S + sel * 2^D, sel 0 = none, D <= max_doors
// and K <= max_items the env's own counts.  Inside a layer the cells are the base maps with the opened doors' cells and the
// picked item's cell free, and the moves are mg_goal_core.h's plane recurrence.  Between layers there are few edges, each from
// the (at most four) states that face the object: pick up (from a layer without an item, cost 1), open a closed door (cost 1),
// open a locked door (cost 2, the key being the layer's item or the agent's own carry).  The search is mg_goal_distance's
// reverse search by levels, over all layers at once; an edge whose target state was first reached at level r puts its source
// state into the frontier of level r + cost.  Agents with different carries ask different questions: the env is searched once
// per CLASS of its agents (empty hands; carrying no key; carrying a key of colour c), in rising order of class.
#pragma once

#if !defined(__HIPCC_RTC__)   // (a run-time compile — mg_rtc.hip — has no system headers: its source supplies these names)
#include <stddef.h>
#include <stdint.h>
#endif

#include "mg_goal_core.h"

// the host twin checks every scratch index against the size of what it indexes
#if defined(MG_SOLVE_HOST_CHECKS)
#include <assert.h>
#define MG_SOLVE_AT(i, n) assert((size_t)(i) < (size_t)(n))
#else
#define MG_SOLVE_AT(i, n) do {} while (0)
#endif

namespace mg {

enum { kSolveMaxDoors = 4, kSolveMaxItems = 3, kSolveItem0 = 4, kSolveObjs = 7 };    // object slots: doors 0 .. 3, items 4 .. 6
enum { kSolveNoPath = 6 };          // the first action where there is no path: `done`
enum { kSolveTailBytes = 1024 };    // what the scratch holds behind the planes (SolveTail)

MG_HD int solve_layers(int doors, int items) { return (1 + items) << doors; }
// planes: free [WN], goal [WN]; per layer visited and two frontiers, [4 WN] each
MG_HD size_t solve_plane_words(int W, int H, int max_doors, int max_items) {
    return (size_t)W * goal_words(H) * (2 + 12 * solve_layers(max_doors, max_items));
}
MG_HD size_t solve_scratch_bytes(int W, int H, int max_doors, int max_items) {
    return 8 * solve_plane_words(W, H, max_doors, max_items) + kSolveTailBytes;
}
// every level but the empty ones labels a new state, and a level is empty only while a cost-2 edge is due
MG_HD int solve_max_levels(int W, int H, int layers, int doors) { return layers * (4 * W * H + 4 * doors) + 2; }

struct SolveTail {
    int32_t adist[MG_MAX_AGENTS];
    int32_t aact[MG_MAX_AGENTS];
    uint32_t cnt[64];               // per lane: shut doors | items << 16 of its run of words
    int32_t ox[kSolveObjs], oy[kSolveObjs];
    int32_t okind[kSolveObjs];      // door: cost (0 not openable, 1 closed, 2 locked) | color_idx << 8; item: its key colour, 256 none
    int32_t D, K, exact;
    uint8_t pend[4 << 6];           // [layer * 4 + dir]: the cost-2 edges of the source states (layer, dir) that are due next level
    uint8_t fired[4];               // [dir]: the objects whose edge put layer 0's state into this level's frontier
};
static_assert(sizeof(SolveTail) <= kSolveTailBytes, "SolveTail outgrew its place in the scratch");

struct SolveScratch {
    GoalScratch g;          // the base maps (free_w, goal_w) and the shape; its other planes are not used
    uint64_t *visited, *front, *next;       // [layers][4 WN]
    SolveTail* t;
    int cap_layers;
    size_t layer_words;     // cap_layers * 4 WN: the size of each of the three
};

MG_HD SolveScratch solve_scratch(void* base, int W, int H, int max_doors, int max_items) {
    SolveScratch s;
    s.g.W = W;
    s.g.H = H;
    s.g.NW = goal_words(H);
    s.g.WN = W * s.g.NW;
    s.cap_layers = solve_layers(max_doors, max_items);
    s.layer_words = (size_t)s.cap_layers * 4 * s.g.WN;
    s.g.free_w = static_cast<uint64_t*>(base);
    s.g.goal_w = s.g.free_w + s.g.WN;
    s.visited = s.g.goal_w + s.g.WN;
    s.front = s.visited + s.layer_words;
    s.next = s.front + s.layer_words;
    s.g.visited = s.g.front = s.g.next = nullptr;
    s.g.adist = nullptr;
    s.t = reinterpret_cast<SolveTail*>(s.next + s.layer_words);
    return s;
}

// The class of an agent's question: 0 empty hands, 1 carrying something that is no key, 2 + c carrying a key of colour c.
MG_HD int solve_class(const MgConfig& cfg, uint64_t r) {
    const uint32_t carry = rec_byte(r, MG_AG_CARRY);
    if (!carry) return 0;
    if (carry >= (uint32_t)cfg.n_obj || !(cfg.obj[carry].flags & MG_OF_IS_KEY)) return 1;
    return 2 + (int)cfg.obj[carry].color_idx;
}
// the smallest class above `after` among the env's agents that are in a cell, -1 if none (every lane works it out alike)
MG_HD int solve_next_class(const MgConfig& cfg, const uint64_t* rec_b, int after) {
    int best = -1;
    for (int k = 0; k < cfg.n_agents; k++) {
        const uint64_t r = rec_b[k];
        if (!goal_agent(cfg, r).in_cell) continue;
        const int c = solve_class(cfg, r);
        if (c > after && (best < 0 || c < best)) best = c;
    }
    return best;
}

// what a shut door costs to open: 0 (not openable), 1 (closed), 2 (locked)
MG_HD int solve_door_cost(const MgConfig& cfg, uint32_t id) {
    const MgObjDesc od = cfg.obj[id];
    uint32_t shut = id;
    if (od.flags & MG_OF_DOOR_LOCKED) {
        shut = od.unlock_next;
        if (shut == 0 || shut >= (uint32_t)cfg.n_obj) return 0;
        const uint32_t f = cfg.obj[shut].flags;
        if (!(f & MG_OF_IS_DOOR) || (f & (MG_OF_DOOR_LOCKED | MG_OF_IS_BOX | MG_OF_CAN_OVERLAP | MG_OF_CAN_PICKUP))) return 0;
    }
    if (goal_cell_kind(cfg, cfg.obj[shut].toggle_next) != kGoalFree) return 0;
    return (od.flags & MG_OF_DOOR_LOCKED) ? 2 : 1;
}

// Every function below is one PHASE for the items lane, lane + lanes, ... (lanes <= 64), as in mg_goal_core.h: a phase reads
// only what earlier phases wrote, or what its own item wrote.

// phase 1: the base maps; the shut doors' and the items' bits, parked in the first 2 WN words of `next` (which the search
// writes from level 2 on); the agents' labels
MG_HD void solve_build(const MgConfig& cfg, const uint8_t* grid_b, const SolveScratch& s, int lane, int lanes) {
    const int WN = s.g.WN, NW = s.g.NW, H = s.g.H;
    for (int i = lane; i < WN; i += lanes) {
        const int x = i / NW, w = i - x * NW;
        const int y1 = H < 64 * (w + 1) ? H : 64 * (w + 1);
        const uint8_t* col = grid_b + (size_t)x * H;
        uint64_t f = 0, g = 0, dr = 0, it = 0;
        for (int y = 64 * w; y < y1; y++) {
            const uint32_t id = col[y];
            const int kind = goal_cell_kind(cfg, id);
            const uint64_t bit = 1ull << (y - 64 * w);
            if (kind == kGoalFree) f |= bit;
            else if (kind == kGoalGoal) g |= bit;
            else if (id && id < (uint32_t)cfg.n_obj) {
                const uint32_t fl = cfg.obj[id].flags;
                if (fl & MG_OF_CAN_PICKUP) it |= bit;
                else if ((fl & MG_OF_IS_DOOR) && !(fl & (MG_OF_CAN_OVERLAP | MG_OF_IS_BOX))) dr |= bit;
            }
        }
        MG_SOLVE_AT(WN + i, s.layer_words);
        s.g.free_w[i] = f;
        s.g.goal_w[i] = g;
        s.next[i] = dr;
        s.next[WN + i] = it;
    }
    for (int k = lane; k < MG_MAX_AGENTS; k += lanes) {
        s.t->adist[k] = -1;
        s.t->aact[k] = kSolveNoPath;
    }
}

// the run of words lane `lane` counts and lists: index order is word order
MG_HD void solve_run(const SolveScratch& s, int lane, int lanes, int* lo, int* hi) {
    const int c = (s.g.WN + lanes - 1) / lanes;
    *lo = lane * c < s.g.WN ? lane * c : s.g.WN;
    *hi = *lo + c < s.g.WN ? *lo + c : s.g.WN;
}

// phase 2: how many shut doors and items each lane's run of words holds
MG_HD void solve_count(const SolveScratch& s, int lane, int lanes) {
    for (int l = lane; l < 64; l += lanes) {
        uint32_t cd = 0, ci = 0;
        if (l < lanes) {
            int lo, hi;
            solve_run(s, l, lanes, &lo, &hi);
            for (int i = lo; i < hi; i++) {
                cd += (uint32_t)__builtin_popcountll(s.next[i]);
                ci += (uint32_t)__builtin_popcountll(s.next[s.g.WN + i]);
            }
        }
        s.t->cnt[l] = cd | (ci << 16);
    }
}

MG_HD void solve_slot(const MgConfig& cfg, const uint8_t* grid_b, const SolveScratch& s, int slot, int x, int y) {
    MG_SOLVE_AT(slot, kSolveObjs);
    const uint32_t id = grid_b[(size_t)x * s.g.H + y];
    s.t->ox[slot] = x;
    s.t->oy[slot] = y;
    if (slot < kSolveItem0) s.t->okind[slot] = solve_door_cost(cfg, id) | ((int)cfg.obj[id].color_idx << 8);
    else s.t->okind[slot] = (cfg.obj[id].flags & MG_OF_IS_KEY) ? (int)cfg.obj[id].color_idx : 256;
}

// phase 3: the tracked objects' table — a lane lists those of its run whose rank in the grid is under the cap —, the env's
// counts and its `exact`
MG_HD void solve_table(const MgConfig& cfg, const uint8_t* grid_b, const SolveScratch& s, int max_doors, int max_items, int lane, int lanes) {
    for (int l = lane; l < lanes; l += lanes) {
        int pd = 0, pi = 0;
        for (int j = 0; j < l; j++) {
            pd += (int)(s.t->cnt[j] & 0xFFFFu);
            pi += (int)(s.t->cnt[j] >> 16);
        }
        if (l == 0) {
            int td = 0, ti = 0;
            for (int j = 0; j < lanes; j++) {
                td += (int)(s.t->cnt[j] & 0xFFFFu);
                ti += (int)(s.t->cnt[j] >> 16);
            }
            s.t->D = td < max_doors ? td : max_doors;
            s.t->K = ti < max_items ? ti : max_items;
            s.t->exact = (td <= max_doors && ti <= max_items) ? 1 : 0;
        }
        if (pd >= max_doors && pi >= max_items) continue;
        int lo, hi;
        solve_run(s, l, lanes, &lo, &hi);
        for (int i = lo; i < hi; i++) {
            const int x = i / s.g.NW, w = i - x * s.g.NW;
            for (uint64_t bits = s.next[i]; bits && pd < max_doors; bits &= bits - 1, pd++)
                solve_slot(cfg, grid_b, s, pd, x, 64 * w + __builtin_ctzll(bits));
            for (uint64_t bits = s.next[s.g.WN + i]; bits && pi < max_items; bits &= bits - 1, pi++)
                solve_slot(cfg, grid_b, s, kSolveItem0 + pi, x, 64 * w + __builtin_ctzll(bits));
        }
    }
}

// before each class's search: no edge due
MG_HD void solve_pass_init(const SolveScratch& s, int lane, int lanes) {
    for (int e = lane; e < (4 << 6); e += lanes) s.t->pend[e] = 0;
    for (int d = lane; d < 4; d += lanes) s.t->fired[d] = 0;
}

// word (x, w) of layer L's free map, 0 outside the grid: the base word patched with the layer's opened doors and its item
MG_HD uint64_t solve_free_word(const SolveScratch& s, int L, int D, int x, int w) {
    if (x < 0 || x >= s.g.W || w < 0 || w >= s.g.NW) return 0ull;
    uint64_t f = s.g.free_w[x * s.g.NW + w];
    if (!L) return f;
    const SolveTail& t = *s.t;
    for (int j = 0; j < D; j++)
        if (((L >> j) & 1) && t.ox[j] == x && (t.oy[j] >> 6) == w) f |= 1ull << (t.oy[j] & 63);
    const int sel = L >> D;
    if (sel) {
        const int o = kSolveItem0 + sel - 1;
        MG_SOLVE_AT(o, kSolveObjs);
        if (t.ox[o] == x && (t.oy[o] >> 6) == w) f |= 1ull << (t.oy[o] & 63);
    }
    return f;
}

// level 1 (src null: the goal map itself is the frontier) and the first third of a level: dst = the states the moves inside
// their layer first reach now, for the layers of `work` (those with a frontier, or with an old one left in dst).  An item is
// a (d, x, w): its own word, the ONE neighbouring word direction d reads and their base maps are fetched once, and only an
// item with a tracked object in either word patches them per layer.  Returns the layers in which this lane found any.
MG_HD uint64_t solve_expand(const SolveScratch& s, const uint64_t* src, uint64_t* dst, int layers, int D, uint64_t work, int lane, int lanes) {
    const GoalScratch& g = s.g;
    const int WN = g.WN, NW = g.NW, per = 4 * WN, K = (layers >> D) - 1;
    const SolveTail& t = *s.t;
    uint64_t found = 0;
    for (int r = lane; r < per; r += lanes) {
        const int d = r / WN, q = r - d * WN;
        const int x = q / NW, w = q - x * NW;
        int nx = x, nw = w;
        switch (d) {
        case 0: nx = x + 1; break;
        case 1: nw = w + 1; break;
        case 2: nx = x - 1; break;
        default: nw = w - 1; break;
        }
        const bool nb_in = nx >= 0 && nx < g.W && nw >= 0 && nw < NW;
        const int ni = nb_in ? nx * NW + nw : q;
        bool touched = false;
        for (int o = 0; o < kSolveItem0 + K; o++) {
            if (o >= D && o < kSolveItem0) continue;
            const int ow = t.oy[o] >> 6;
            touched |= (t.ox[o] == x && ow == w) || (nb_in && t.ox[o] == nx && ow == nw);
        }
        const uint64_t base_here = g.free_w[q], goal_here = g.goal_w[q], base_nb = nb_in ? g.free_w[ni] : 0ull;
        for (int L = 0; L < layers; L++) {
            if (!((work >> L) & 1ull)) continue;
            const size_t at = (size_t)L * per;
            MG_SOLVE_AT(at + r, s.layer_words);
            uint64_t free_here = base_here, free_nb = base_nb;
            if (touched && L) {
                free_here = solve_free_word(s, L, D, x, w);
                free_nb = solve_free_word(s, L, D, nx, nw);
            }
            const uint64_t open_w = free_here | goal_here;
            uint64_t got = 0;
            if (open_w) {
                // (the frontier's states that stand on a free cell: a goal cell is entered, never crossed)
                const uint64_t* m = src ? src + at + (size_t)d * WN : g.goal_w;
                const uint64_t nb = nb_in ? (src ? m[ni] & free_nb : m[ni]) : 0ull;
                const uint64_t self = (d & 1) ? (src ? m[q] & free_here : m[q]) : 0ull;
                const uint64_t ahead = goal_ahead_word(d, self, d == 0 ? nb : 0ull, d == 2 ? nb : 0ull, d == 1 ? nb : 0ull, d == 3 ? nb : 0ull);
                got = src ? goal_next_word(open_w, s.visited[at + r], src[at + (size_t)((d + 1) & 3) * WN + q],
                                           src[at + (size_t)((d + 3) & 3) * WN + q], ahead)
                          : open_w & ahead;
            }
            dst[at + r] = got;
            s.visited[at + r] = src ? (s.visited[at + r] | got) : got;
            if (got) found |= 1ull << L;
        }
    }
    return found;
}

// whether state (x, y, d) of layer L is in frontier f
MG_HD bool solve_bit(const SolveScratch& s, const uint64_t* f, int L, int x, int y, int d) {
    if (x < 0 || x >= s.g.W || y < 0 || y >= s.g.H) return false;
    const size_t i = (size_t)L * 4 * s.g.WN + ((size_t)(d & 3) * s.g.W + x) * s.g.NW + (y >> 6);
    MG_SOLVE_AT(i, s.layer_words);
    return (f[i] >> (y & 63)) & 1ull;
}

// the second third of a level: the edges between layers.  Item (L, d): the states of layer L that face a tracked object in
// direction d — nobody else writes plane (L, d) in this phase.  `front` holds level - 1, `next` level.  Returns the layers in
// which this lane added a state; *due: an edge of cost 2 is due at the next level.
MG_HD uint64_t solve_edges(const SolveScratch& s, const uint64_t* front, uint64_t* next, int layers, int D, int K, int pass_key, int lane,
                           int lanes, bool* due) {
    const SolveTail& t = *s.t;
    uint64_t found = 0;
    for (int e = lane; e < 4 * layers; e += lanes) {
        const int L = e >> 2, d = e & 3, S = L & ((1 << D) - 1), sel = L >> D;
        MG_SOLVE_AT(e, sizeof(t.pend));
        const uint32_t pend = s.t->pend[e];
        uint32_t pend_next = 0, fired = 0;
        for (int o = 0; o < kSolveItem0 + K; o++) {
            if (o >= D && o < kSolveItem0) continue;
            int target, cost = 1;
            if (o < D) {
                cost = t.okind[o] & 0xFF;
                if (((S >> o) & 1) || !cost) continue;
                if (cost == 2 && (sel ? t.okind[kSolveItem0 + sel - 1] : pass_key) != (t.okind[o] >> 8)) continue;
                target = L | (1 << o);
            } else {
                if (sel) continue;
                target = L + ((o - kSolveItem0 + 1) << D);
            }
            MG_SOLVE_AT(target, layers);
            const int px = t.ox[o] - dir_dx(d), py = t.oy[o] - dir_dy(d);
            const bool hit = solve_bit(s, front, target, px, py, d);
            bool join = hit;
            if (cost == 2) {
                join = (pend >> o) & 1u;
                if (hit) pend_next |= 1u << o;
            }
            if (!join) continue;
            fired |= 1u << o;
            const size_t i = (size_t)L * 4 * s.g.WN + ((size_t)d * s.g.W + px) * s.g.NW + (py >> 6);
            MG_SOLVE_AT(i, s.layer_words);
            const uint64_t bit = 1ull << (py & 63);
            if (s.visited[i] & bit) continue;
            s.visited[i] |= bit;
            next[i] |= bit;
            found |= 1ull << L;
        }
        s.t->pend[e] = (uint8_t)pend_next;
        if (pend_next) *due = true;
        if (L == 0) s.t->fired[d] = (uint8_t)fired;
    }
    return found;
}

// the first action of a shortest path from (x, y, d) of layer 0, labelled at `level`: the lowest action id whose successor is
// in `prev`, the frontier of level - 1 (for the first toggle of a locked door: of level - 2, which `fired` remembers)
MG_HD int solve_first_action(const SolveScratch& s, const uint64_t* prev, int K, int level, int x, int y, int d) {
    if (level == 1) return 2;
    if (solve_bit(s, prev, 0, x, y, d + 3)) return 0;
    if (solve_bit(s, prev, 0, x, y, d + 1)) return 1;
    const int fx = x + dir_dx(d), fy = y + dir_dy(d);
    if (fx < 0 || fx >= s.g.W || fy < 0 || fy >= s.g.H) return kSolveNoPath;
    if (((s.g.free_w[fx * s.g.NW + (fy >> 6)] >> (fy & 63)) & 1ull) && solve_bit(s, prev, 0, fx, fy, d)) return 2;
    for (int o = 0; o < kSolveItem0 + K; o++)
        if (((s.t->fired[d] >> o) & 1) && s.t->ox[o] == fx && s.t->oy[o] == fy) return o < kSolveItem0 ? 5 : 3;
    return kSolveNoPath;
}

// the last third of a level: the agents of class `cls` look their state up in layer 0 of the new frontier `cur`.  Returns
// whether one of them is still without a label.
MG_HD bool solve_agents(const MgConfig& cfg, const uint64_t* rec_b, const SolveScratch& s, const uint64_t* prev, const uint64_t* cur, int cls,
                        int K, int level, int lane, int lanes) {
    bool pending = false;
    for (int k = lane; k < cfg.n_agents; k += lanes) {
        const uint64_t r = rec_b[k];
        const GoalAgent a = goal_agent(cfg, r);
        if (!a.in_cell || s.t->adist[k] >= 0 || solve_class(cfg, r) != cls) continue;
        if (solve_bit(s, cur, 0, a.x, a.y, a.d)) {
            s.t->adist[k] = level;
            s.t->aact[k] = solve_first_action(s, prev, K, level, a.x, a.y, a.d);
        } else {
            pending = true;
        }
    }
    return pending;
}

// last phase: the labels
MG_HD void solve_finish(const MgConfig& cfg, const SolveScratch& s, int32_t* dist_b, int8_t* act_b, uint8_t* exact_b, int lane, int lanes) {
    for (int k = lane; k < cfg.n_agents; k += lanes) {
        dist_b[k] = s.t->adist[k];
        if (act_b) act_b[k] = (int8_t)s.t->aact[k];
    }
    if (exact_b && lane == 0) *exact_b = (uint8_t)s.t->exact;
}

}  // namespace mg
