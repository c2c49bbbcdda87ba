// sr_grad_param_f32_full.hip — the parametric gradient kernels (sr_grad_impl.h, PARAM), float, full view:
// tangent widths 1 - 16 at sr_grad_param_rows rows per lane and at 1.
#include "sr_grad_impl.h"

template hipError_t sr_launch_grad_param_any<float, false>(const SrGradArgs<float>&, const SrGradParamArgs<float>&, int, int, int,
                                                          hipStream_t);
