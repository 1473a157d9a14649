// TEST INFRASTRUCTURE — the compact signature of mg_step_render_delta (marlgrid_amd/csrc/mg_step_layout.h: delta_sig_*), built
// for the host with g++ and called through ctypes (tests/test_delta_sig_host.py).
#include "mg_step_layout.h"

extern "C" {

int sig_slot_bytes(void) { return mg::kDeltaSigSlot; }
unsigned sig_none(void) { return mg::kDeltaSigNone; }
int sig_compact(int n_tiles, int n_agents, int view_size) { return mg::delta_sig_compact(n_tiles, n_agents, view_size) ? 1 : 0; }
unsigned sig_code(unsigned entry, unsigned tile_dwords) { return mg::delta_sig_code(entry, tile_dwords); }
unsigned sig_entry(unsigned code, unsigned tile_dwords) { return mg::delta_sig_entry(code, tile_dwords); }
long long sig_env_bytes(int n_agents) { return (long long)mg::delta_sig_env_bytes(n_agents); }
long long sig_slot(long long e, int v, int n_agents) { return (long long)mg::delta_sig_slot((size_t)e, v, n_agents); }
long long sig_alloc_bytes(int n_agents, int view_size) { return (long long)MG_DELTA_SIG_BYTES(n_agents, view_size); }

}  // extern "C"
