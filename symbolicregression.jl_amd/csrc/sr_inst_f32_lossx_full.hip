// f32 FULL-tier (per-node checks, every operator) loss kernels of expression-loss calls: 4 rows/lane, full
// dataset and row view.
#include "sr_tile_impl.h"
SR_INSTANTIATE_WL(float, 4, SR_MODE_LOSS, false, SR_TIER_FULL, 4, SR_LOSS_EXPR)
SR_INSTANTIATE_WL(float, 4, SR_MODE_LOSS, true, SR_TIER_FULL, 4, SR_LOSS_EXPR)
