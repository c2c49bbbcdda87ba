// f64 exact-check kernels for parametric calls (4 waves, FULL-tier build for every operator set).
#include "sr_tile_impl.h"
SR_INSTANTIATE_PARAM(double, 2, SR_MODE_EXACT, false, SR_TIER_FULL, 4, -1, false)
SR_INSTANTIATE_PARAM(double, 2, SR_MODE_EXACT, true, SR_TIER_FULL, 4, -1, false)
