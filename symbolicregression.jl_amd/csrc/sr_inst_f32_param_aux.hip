// f32 exact-check (4 waves, FULL-tier build for every operator set) and FULL-tier FOLD kernels for
// parametric calls.
#include "sr_tile_impl.h"
SR_INSTANTIATE_PARAM(float, 4, SR_MODE_EXACT, false, SR_TIER_FULL, 4, -1, false)
SR_INSTANTIATE_PARAM(float, 4, SR_MODE_EXACT, true, SR_TIER_FULL, 4, -1, false)
SR_INSTANTIATE_PARAM(float, 4, SR_MODE_FOLD, false, SR_TIER_FULL, 4, -1, false)
SR_INSTANTIATE_PARAM(float, 4, SR_MODE_FOLD, true, SR_TIER_FULL, 4, -1, false)
