// mg_view_triple.h — the (type, colour, state) triple of a visible world cell as agent k's view shows it: the cell object as
// `grid.get` returns it after hide_item_types (base.py:441-449), encoded as WorldObj.encode (objects.py:90-99) — the ONE
// definition of the hide rules.  mg_encode_views.hip (phases A and E) writes it into the encoded view, mg_explore.hip
// (MEM_ = true) into the agent's memory map; tests/native/mg_memory.cpp runs it under g++.  Plain functions over pointers, one
// call per lane item: the kernels hand them LDS tables, the host harness heap blocks.
#pragma once
#include "mg_core.h"

namespace mg {

constexpr int kEvTab = 256 * 4 * 2;          // bytes of the two tables below: triples + see_behind bit, hide_item_types masks

// entry o of the triple table [256]: type | colour << 8 | state << 16 | see_behind << 24.  None (0): (0, 0, 0), transparent
// (base.py:103-106); ids past the object table: (0, 0, 0), opaque
MG_HD uint32_t view_triple_entry(const MgConfig& cfg, int o) {
    if (o == 0) return 1u << 24;
    if (o >= cfg.n_obj) return 0;
    const MgObjDesc d = cfg.obj[o];
    return (uint32_t)d.type_idx | ((uint32_t)d.color_idx << 8) | ((uint32_t)d.state << 16) |
           ((d.flags & MG_OF_SEE_BEHIND) ? 1u << 24 : 0u);
}

// entry o of the hide table [256]: bit k = agent k hides this object id
MG_HD uint32_t view_hide_entry(const MgConfig& cfg, int o) {
    return (o < cfg.n_obj && cfg.any_hide && cfg.hide_by_obj) ? cfg.hide_by_obj[o] : 0u;
}

// A cell's occupant as grid.get returns it: the object; on an empty cell the lowest-rank agent standing there (the cell
// object, base.py:547-552) — an agent on an object is not encoded.  hide_item_types (base.py:441-449): a hidden object becomes
// its agents[0] (the lowest-rank agent on it) or None; a hidden agent that is not the viewer becomes ITS agents[0] (the
// second-lowest rank of the cell) or None.
// tab / hide: the tables above; rec: the n agent records of the env; base: the grid's object id at world cell (wx, wy), which
// is inside the grid; k: the viewer.  -> type | colour << 8 | state << 16
MG_HD uint32_t view_cell_triple(const MgConfig& cfg, const uint32_t* tab, const uint32_t* hide, const uint64_t* rec, int n, int k,
                                uint32_t base, int wx, int wy) {
    const bool hid_obj = base != 0 && ((hide[base] >> k) & 1u);
    if (base != 0 && !hid_obj) return tab[base] & 0xFFFFFFu;
    // the lowest- and second-lowest-rank agents of the cell
    const uint32_t cxy = (uint32_t)wx | ((uint32_t)wy << 8);
    uint32_t r1 = 0x100, r2 = 0x100, a1 = 0xFF, a2 = 0xFF;
    for (int j = 0; j < n; j++) {
        const uint64_t rj = rec[j];
        if ((rec_byte(rj, MG_AG_FLAGS) & MG_AF_PLACED) && rec_xy(rj) == cxy) {
            const uint32_t rk = rec_byte(rj, MG_AG_RANK);
            if (rk < r1) { r2 = r1; a2 = a1; r1 = rk; a1 = (uint32_t)j; }
            else if (rk < r2) { r2 = rk; a2 = (uint32_t)j; }
        }
    }
    uint32_t a = a1;
    if (!hid_obj && a1 != 0xFF && a1 != (uint32_t)k && ((cfg.hide_agent_mask >> k) & 1u)) a = a2;
    if (a == 0xFF) return 0;
    return (uint32_t)cfg.agent_type_idx | ((uint32_t)cfg.agent_color_idx[a] << 8) | (rec_byte(rec[a], MG_AG_DIR) << 16);
}

}  // namespace mg
