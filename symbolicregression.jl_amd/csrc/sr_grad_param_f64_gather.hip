// sr_grad_param_f64_gather.hip — the parametric gradient kernels (sr_grad_impl.h, PARAM), double, gathered row views:
// tangent widths 1 - 16 at sr_grad_param_rows rows per lane and at 1.
#include "sr_grad_impl.h"

template hipError_t sr_launch_grad_param_any<double, true>(const SrGradArgs<double>&, const SrGradParamArgs<double>&, int, int, int,
                                                          hipStream_t);
