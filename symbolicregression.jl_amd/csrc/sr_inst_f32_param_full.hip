// f32 FULL-tier loss and prediction kernels for parametric calls (4 rows/lane).
#include "sr_tile_impl.h"
SR_INSTANTIATE_PARAM(float, 4, SR_MODE_LOSS, false, SR_TIER_FULL, 4, -1, false)
SR_INSTANTIATE_PARAM(float, 4, SR_MODE_LOSS, true, SR_TIER_FULL, 4, -1, false)
SR_INSTANTIATE_PARAM(float, 4, SR_MODE_PRED, false, SR_TIER_FULL, 4, -1, false)
SR_INSTANTIATE_PARAM(float, 4, SR_MODE_PRED, true, SR_TIER_FULL, 4, -1, false)
