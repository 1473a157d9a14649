// TEST INFRASTRUCTURE — the delta launch's wave priority (marlgrid_amd/csrc/mg_step_layout.h: delta_wave_prio, the function the
// kernel calls when a view group begins), built for the host with g++ and called through ctypes (tests/test_delta_prio_host.py).
#include "mg_step_layout.h"

extern "C" {

int delta_prio(int groups_done, int groups_total) { return mg::delta_wave_prio(groups_done, groups_total); }

}  // extern "C"
