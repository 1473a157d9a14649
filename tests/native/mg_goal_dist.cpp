// TEST INFRASTRUCTURE — the bodies of mg_goal_distance (marlgrid_amd/csrc/mg_goal_core.h) built for the host with g++ and called
// through ctypes (tests/native/hostemu_goal.py) or from a main of its own (mg_goal_dist_main.cpp): the two kernels of
// mg_goal_dist.hip emulated over plain arrays.
//   gd_general  goal_lds_kernel: the phases of the general path, the lanes of a phase run one after the other (64: the kernel's
//               wave; 1: one lane walks every item), the "LDS" a heap block of goal_scratch_bytes
//   gd_reg      goal_reg_kernel: 64 lane states in arrays; what the kernel reads from another lane is read from the array of
//               the values all lanes held before the exchange
// Both return 0, or -1 where the kernel would not be launched for the shape.
#include <stdlib.h>
#include <string.h>

#include "mg_goal_core.h"

extern "C" {

int gd_general(const MgConfig* cfg, const MgState* st, const uint8_t* mask, int32_t* agent_dist, int32_t* field, int lanes) {
    const int W = cfg->W, H = cfg->H, n = cfg->n_agents;
    const size_t bytes = mg::goal_scratch_bytes(W, H);
    if (bytes > 160 * 1024 || lanes < 1) return -1;
    void* mem = malloc(bytes);
    if (!mem) return -1;
    for (int b = 0; b < cfg->B; b++) {
        if (mask && !mask[b]) continue;
        memset(mem, 0xA5, bytes);       // (LDS is not zero when a wave starts)
        mg::GoalScratch s = mg::goal_scratch(mem, W, H);
        const uint8_t* grid_b = st->grid + (size_t)b * cfg->cells_stride;
        const uint64_t* rec_b = st->agents + (size_t)b * n;
        int32_t* field_b = field ? field + (size_t)b * W * H * 4 : nullptr;
        bool any = false, pending = false;
        for (int l = 0; l < lanes; l++) mg::goal_gen_build(*cfg, grid_b, s, l, lanes);
        for (int l = 0; l < lanes; l++) any |= mg::goal_gen_expand(s, nullptr, s.front, 1, field_b, l, lanes);
        for (int l = 0; l < lanes; l++) pending |= mg::goal_gen_agents(*cfg, rec_b, s, s.front, 1, l, lanes);
        const int max_levels = mg::goal_max_levels(W, H);
        int level = 1;
        while (any && (field_b || pending) && level < max_levels) {
            level++;
            any = pending = false;
            for (int l = 0; l < lanes; l++) any |= mg::goal_gen_expand(s, s.front, s.next, level, field_b, l, lanes);
            for (int l = 0; l < lanes; l++) pending |= mg::goal_gen_agents(*cfg, rec_b, s, s.next, level, l, lanes);
            uint64_t* t = s.front;
            s.front = s.next;
            s.next = t;
        }
        for (int l = 0; l < lanes; l++) mg::goal_gen_finish(*cfg, s, agent_dist + (size_t)b * n, field_b, l, lanes);
    }
    free(mem);
    return 0;
}

int gd_reg(const MgConfig* cfg, const MgState* st, const uint8_t* mask, int32_t* agent_dist, int32_t* field) {
    const int W = cfg->W, H = cfg->H, n = cfg->n_agents;
    if (!mg::goal_reg_fits(W, H)) return -1;
    constexpr int L = 64;
    for (int b = 0; b < cfg->B; b++) {
        if (mask && !mask[b]) continue;
        const uint8_t* grid_b = st->grid + (size_t)b * cfg->cells_stride;
        int32_t* field_b = field ? field + (size_t)b * W * H * 4 : nullptr;
        uint64_t pf[L] = {}, pg[L] = {}, free_w[L], goal_w[L], open_w[L], front[L], visited[L], walk[L], nw[L];
        int d[L], x[L], ta[L], tb[L], ahead[L], ok[L];
        bool has[L];
        for (int l = 0; l < L; l++) {
            has[l] = l < 4 * W;
            d[l] = has[l] ? l / W : 0;
            x[l] = has[l] ? l - d[l] * W : 0;
            if (has[l]) mg::goal_column_bits(*cfg, grid_b, x[l], 0, d[l], 4, H, &pf[l], &pg[l]);
        }
        for (int l = 0; l < L; l++) {
            const int s1 = mg::goal_reg_turn_lane(W, d[l], x[l], 1), s2 = mg::goal_reg_turn_lane(W, d[l], x[l], 2),
                      s3 = mg::goal_reg_turn_lane(W, d[l], x[l], 3);
            free_w[l] = has[l] ? pf[l] | pf[s1] | pf[s2] | pf[s3] : 0;
            goal_w[l] = has[l] ? pg[l] | pg[s1] | pg[s2] | pg[s3] : 0;
            open_w[l] = free_w[l] | goal_w[l];
            ta[l] = mg::goal_reg_turn_lane(W, d[l], x[l], 1);
            tb[l] = mg::goal_reg_turn_lane(W, d[l], x[l], 3);
            ok[l] = 0;
            ahead[l] = l;
            if (has[l]) ahead[l] = mg::goal_reg_ahead_lane(W, d[l], x[l], &ok[l]);
        }
        mg::GoalAgent ag[L];
        int32_t my_dist[L];
        for (int l = 0; l < L; l++) {
            ag[l] = mg::GoalAgent{0, 0, 0, 0};
            if (l < n) ag[l] = mg::goal_agent(*cfg, st->agents[(size_t)b * n + l]);
            my_dist[l] = -1;
        }
        for (int l = 0; l < L; l++) visited[l] = front[l] = mg::goal_reg_word(d[l], open_w[l], 0, 0, 0, goal_w[l], goal_w[ahead[l]], ok[l]);
        const int max_levels = mg::goal_max_levels(W, H);
        int level = 1;
        for (;;) {
            bool any = false, pending = false;
            for (int l = 0; l < L; l++) {
                if (field_b && front[l]) mg::goal_field_store(field_b, H, x[l], 0, d[l], front[l], level);
                const int owner = ag[l].in_cell ? ag[l].d * W + ag[l].x : 0;
                if (ag[l].in_cell && my_dist[l] < 0 && ((front[owner] >> ag[l].y) & 1ull)) my_dist[l] = level;
                any |= front[l] != 0;
                pending |= ag[l].in_cell && my_dist[l] < 0;
            }
            if (!any || (!field_b && !pending) || level >= max_levels) break;
            level++;
            for (int l = 0; l < L; l++) walk[l] = front[l] & free_w[l];
            for (int l = 0; l < L; l++)
                nw[l] = mg::goal_reg_word(d[l], open_w[l], visited[l], front[ta[l]], front[tb[l]], walk[l], walk[ahead[l]], ok[l]);
            for (int l = 0; l < L; l++) {
                visited[l] |= nw[l];
                front[l] = nw[l];
            }
        }
        for (int l = 0; l < L; l++) {
            if (l < n) agent_dist[(size_t)b * n + l] = my_dist[l];
            if (field_b && has[l]) mg::goal_field_store(field_b, H, x[l], 0, d[l], ~visited[l] & mg::goal_row_mask(H, 0), -1);
        }
    }
    return 0;
}

size_t gd_scratch_bytes(int W, int H) { return mg::goal_scratch_bytes(W, H); }

}  // extern "C"
