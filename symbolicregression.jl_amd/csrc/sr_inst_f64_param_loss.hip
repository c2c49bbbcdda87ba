// f64 BASIC-tier loss kernels for parametric calls: 4 rows/lane (L2 / generic over the full dataset,
// generic over a row view) and the 8-rows/lane register-stack build.
#include "sr_tile_impl.h"
SR_INSTANTIATE_PARAM(double, 4, SR_MODE_LOSS, false, SR_TIER_BASIC, 4, SR_LOSS_L2, false)
SR_INSTANTIATE_PARAM(double, 4, SR_MODE_LOSS, false, SR_TIER_BASIC, 4, -1, false)
SR_INSTANTIATE_PARAM(double, 4, SR_MODE_LOSS, true, SR_TIER_BASIC, 4, -1, false)
SR_INSTANTIATE_PARAM(double, 8, SR_MODE_LOSS, false, SR_TIER_BASIC, 4, SR_LOSS_L2, true)
SR_INSTANTIATE_PARAM(double, 8, SR_MODE_LOSS, false, SR_TIER_BASIC, 4, -1, true)
