// f32 register-stack loss kernels for parametric calls: BASIC tier at 16 rows/lane (L2 and generic loss).
#include "sr_tile_impl.h"
SR_INSTANTIATE_PARAM(float, 16, SR_MODE_LOSS, false, SR_TIER_BASIC, 4, SR_LOSS_L2, true)
SR_INSTANTIATE_PARAM(float, 16, SR_MODE_LOSS, false, SR_TIER_BASIC, 4, -1, true)
