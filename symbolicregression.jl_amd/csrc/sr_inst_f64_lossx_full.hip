// f64 FULL-tier loss kernels of expression-loss calls: 2 rows/lane, full dataset and row view.
#include "sr_tile_impl.h"
SR_INSTANTIATE_WL(double, 2, SR_MODE_LOSS, false, SR_TIER_FULL, 4, SR_LOSS_EXPR)
SR_INSTANTIATE_WL(double, 2, SR_MODE_LOSS, true, SR_TIER_FULL, 4, SR_LOSS_EXPR)
