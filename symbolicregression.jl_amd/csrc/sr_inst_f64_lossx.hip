// f64 BASIC-tier loss kernels of expression-loss calls (SR_LOSS_EXPR, sr_loss_expr.h): 4 rows/lane, over the
// full dataset and over a row view.
#include "sr_tile_impl.h"
SR_INSTANTIATE_WL(double, 4, SR_MODE_LOSS, false, SR_TIER_BASIC, 4, SR_LOSS_EXPR)
SR_INSTANTIATE_WL(double, 4, SR_MODE_LOSS, true, SR_TIER_BASIC, 4, SR_LOSS_EXPR)
