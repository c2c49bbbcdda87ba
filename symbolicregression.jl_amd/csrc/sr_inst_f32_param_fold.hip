// f32 BASIC-tier FOLD kernels for parametric calls (generic loss): the shapes of their loss launches.
#include "sr_tile_impl.h"
SR_INSTANTIATE_PARAM(float, 16, SR_MODE_FOLD, false, SR_TIER_BASIC, 4, -1, true)
SR_INSTANTIATE_PARAM(float, 8, SR_MODE_FOLD, false, SR_TIER_BASIC, 4, -1, false)
SR_INSTANTIATE_PARAM(float, 8, SR_MODE_FOLD, true, SR_TIER_BASIC, 4, -1, false)
