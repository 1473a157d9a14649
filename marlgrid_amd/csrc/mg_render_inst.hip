// mg_render_inst.hip — the instantiations of mg::render_kernel, one group of MG_RENDER_ALL (mg_render_pick.h) per object
// (and group Q: MG_RENDER_DELTA, the list of mg_step_render_delta's instantiations; group R: MG_RENDER_DELTA_X, mg_step_render_delta_ex's):
// the Makefile compiles this file once per group with -DMG_RENDER_INST_GROUP=<letter>, in parallel.
#include "mg_render_kernel.h"
#define MG_RENDER_GROUP_OF2(g) MG_RENDER_GROUP_##g
#define MG_RENDER_GROUP_OF(g) MG_RENDER_GROUP_OF2(g)
namespace mg {
#if !defined(MG_DEV_ONLY)
MG_RENDER_GROUP_OF(MG_RENDER_INST_GROUP)(MG_RENDER_INSTANTIATE)
#endif
}  // namespace mg
