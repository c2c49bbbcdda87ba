// sr_grad_inst.hip — one explicit instantiation of a gradient launcher (sr_grad_impl.h; its dispatch over
// tangent widths and rows per lane is recursive over the template); compiled once per unit with
// -DSR_UNIT=<unit> (the Makefile's GRAD_UNITS), so the units compile in parallel.  Float32 plain: sr_grad.hip.
#include "sr_grad_impl.h"

#ifndef SR_UNIT
#error "compile with -DSR_UNIT=<one of the units below>"
#endif
// the parametric gradient kernels (PARAM): tangent widths 1 - 16 at sr_grad_param_rows rows per lane and at 1
#define SR_GRAD_PARAM(T, GATHER)                                                                                          \
  template hipError_t sr_launch_grad_param_any<T, GATHER>(const SrGradArgs<T>&, const SrGradParamArgs<T>&, int, int, int, \
                                                          hipStream_t);
// the expression-loss gradient kernels (LOSSX): tangent widths 1 - 16 at sr_grad_param_rows rows per lane
#define SR_GRAD_LOSSX(T, GATHER)                                                                                         \
  template hipError_t sr_launch_grad_lossx_any<T, GATHER>(const SrGradArgs<T>&, const SrLossProgArgs<T>&, int, int, int, \
                                                          hipStream_t);
// the per-row tangent kernels (ROWOUT): tangent widths 1 - 16 at the plain kernels' rows per lane
#define SR_GRAD_ROWS(T, GATHER)                                                                                        \
  template hipError_t sr_launch_grad_rows_any<T, GATHER>(const SrGradArgs<T>&, const SrGradRowArgs<T>&, int, int, int, \
                                                         hipStream_t);
// the Float64 forward-mode constant-gradient kernels
#define SR_GRAD_UNIT_f64 template hipError_t sr_launch_grad_any<double>(const SrGradArgs<double>&, int, bool, int, int, hipStream_t);
// full view / gathered row views
#define SR_GRAD_UNIT_param_f32_full SR_GRAD_PARAM(float, false)
#define SR_GRAD_UNIT_param_f32_gather SR_GRAD_PARAM(float, true)
#define SR_GRAD_UNIT_param_f64_full SR_GRAD_PARAM(double, false)
#define SR_GRAD_UNIT_param_f64_gather SR_GRAD_PARAM(double, true)
#define SR_GRAD_UNIT_lossx_f32_full SR_GRAD_LOSSX(float, false)
#define SR_GRAD_UNIT_lossx_f32_gather SR_GRAD_LOSSX(float, true)
#define SR_GRAD_UNIT_lossx_f64_full SR_GRAD_LOSSX(double, false)
#define SR_GRAD_UNIT_lossx_f64_gather SR_GRAD_LOSSX(double, true)
#define SR_GRAD_UNIT_rows_f32_full SR_GRAD_ROWS(float, false)
#define SR_GRAD_UNIT_rows_f32_gather SR_GRAD_ROWS(float, true)
#define SR_GRAD_UNIT_rows_f64_full SR_GRAD_ROWS(double, false)
#define SR_GRAD_UNIT_rows_f64_gather SR_GRAD_ROWS(double, true)

#define SR_GRAD_INST_(unit) SR_GRAD_UNIT_##unit
#define SR_GRAD_INST(unit) SR_GRAD_INST_(unit)
SR_GRAD_INST(SR_UNIT)
