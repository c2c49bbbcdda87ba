// sr_grad_lossx_f64_full.hip — the expression-loss gradient kernels (sr_grad_impl.h, LOSSX), double, full view:
// tangent widths 1 - 16 at sr_grad_param_rows rows per lane.
#include "sr_grad_impl.h"

template hipError_t sr_launch_grad_lossx_any<double, false>(const SrGradArgs<double>&, const SrLossProgArgs<double>&, int, int, int,
                                                          hipStream_t);
