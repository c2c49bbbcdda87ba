// sr_grad_lossx_f32_gather.hip — the expression-loss gradient kernels (sr_grad_impl.h, LOSSX), float, gathered rows (row views):
// tangent widths 1 - 16 at sr_grad_param_rows rows per lane.
#include "sr_grad_impl.h"

template hipError_t sr_launch_grad_lossx_any<float, true>(const SrGradArgs<float>&, const SrLossProgArgs<float>&, int, int, int,
                                                          hipStream_t);
