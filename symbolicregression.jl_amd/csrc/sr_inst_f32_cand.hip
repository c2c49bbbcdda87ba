// f32 register-stack loss kernels that also compose each row block's in-order fold steps under
// candidate binades (SR_TIER_CAND, sr_tile_impl.h): the loss launch of a large plain call under the
// reference's in-order fold, 16 rows per lane.
#include "sr_tile_impl.h"
SR_INSTANTIATE_WLV(float, 16, SR_MODE_LOSS, false, SR_TIER_BASIC | SR_TIER_CAND, 4, SR_LOSS_L2, true)
SR_INSTANTIATE_WLV(float, 16, SR_MODE_LOSS, false, SR_TIER_BASIC | SR_TIER_CAND, 4, -1, true)
