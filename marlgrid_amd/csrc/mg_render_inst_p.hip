// mg_render_inst_p.hip — instantiations of mg::render_kernel, group P (mg_render_kernel.h: MG_RENDER_GROUP_P): the fused step
// with the reset mode and the episode outputs of MgEpisode (mg_step_render_ep)
#include "mg_render_kernel.h"
#if defined(MG_AB_VARIANTS)
#include <stdlib.h>
#endif
namespace mg {
#if !defined(MG_DEV_ONLY)
MG_RENDER_GROUP_P(MG_RENDER_INSTANTIATE)
#endif
}  // namespace mg
