// sr_grad_param_f64_full.hip — the parametric gradient kernels (sr_grad_impl.h, PARAM), double, full view:
// tangent widths 1 - 16 at sr_grad_param_rows rows per lane and at 1.
#include "sr_grad_impl.h"

template hipError_t sr_launch_grad_param_any<double, false>(const SrGradArgs<double>&, const SrGradParamArgs<double>&, int, int, int,
                                                           hipStream_t);
