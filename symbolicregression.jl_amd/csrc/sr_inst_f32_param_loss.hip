// f32 loss kernels for parametric calls (LOAD_PARAM / P operands): BASIC tier at 8 rows/lane, the L2 and
// the generic-loss build over the full dataset, the generic one over a row view.
#include "sr_tile_impl.h"
SR_INSTANTIATE_PARAM(float, 8, SR_MODE_LOSS, false, SR_TIER_BASIC, 4, SR_LOSS_L2, false)
SR_INSTANTIATE_PARAM(float, 8, SR_MODE_LOSS, false, SR_TIER_BASIC, 4, -1, false)
SR_INSTANTIATE_PARAM(float, 8, SR_MODE_LOSS, true, SR_TIER_BASIC, 4, -1, false)
