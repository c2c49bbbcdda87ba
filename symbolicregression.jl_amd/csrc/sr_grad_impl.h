// sr_grad_impl.h — batched forward-mode gradient of the loss with respect to tree constants.
//
// What it replaces: the objective/gradient pair BFGS calls in SymbolicRegression's constant
// optimisation (reference src/ConstantOptimization.jl:77-167: Evaluator / GradEvaluator with a
// forward-mode autodiff backend, i.e. value_and_gradient of eval_loss with respect to
// get_scalar_constants(tree)), for many (tree, constant vector) pairs in one launch.
//
// Execution model:
//   * a workgroup = W wave64s = W work items (tree, first tangent k0) x one row block; per tile the
//     X rows (all features), y and w are staged once in LDS and shared by the W waves;
//   * one row per lane; every value carries KT tangents (dual numbers with KT partials, the
//     constants k0 .. k0+KT-1 of the tree in pre-order), all in VGPRs; operand-stack slots
//     (value + tangents) live in a per-wave LDS area;
//   * constants come from a per-tree array (lane k holds constant k), so BFGS updates them without
//     recompiling; a constant leaf with slot c seeds the one-hot tangent e_{c-k0};
//   * per row, d loss / d pred (2(ŷ - y) for L2, sign for L1, times the weight) scales the tangents
//     into per-lane accumulators that live across the row block; one DPP wave reduction per
//     (item, tangent) at the end of the block -> [row block][item][KT] f64 partials.
// Only complete trees are differentiated (the caller evaluates the loss and `complete` with the
// exact loss kernel first: for an incomplete tree eval_loss is the constant L(Inf) and its
// gradient is zero), so this kernel needs no validity checks.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "sr_eval.h"
#include "sr_ops.h"
#include "sr_tile_impl.h"

// Value of lane l of v (l uniform).
template <typename T>
__device__ __forceinline__ T sr_readlane_val(T v, uint32_t l) {
  if constexpr (sizeof(T) == 4) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), int(l)));
  } else {
    const uint64_t b = uint64_t(__double_as_longlong(v));
    const uint32_t lo = uint32_t(__builtin_amdgcn_readlane(int(uint32_t(b)), int(l)));
    const uint32_t hi = uint32_t(__builtin_amdgcn_readlane(int(uint32_t(b >> 32)), int(l)));
    return __longlong_as_double(int64_t((uint64_t(hi) << 32) | lo));
  }
}

// Row callees (noinline: their temporaries live in the callee's own registers, so the kernel's VGPR
// count — and with it its occupancy — is set by the interpreter loop, not by the largest operator body;
// round 3's Float64 kernels inlined every operator into a row-unrolled switch: 256 VGPRs, one wave per
// SIMD).  Value rows, derivative rows, and the operators outside the BASIC set.
template <typename T, int R>
using SrGVec = T __attribute__((ext_vector_type(R)));
template <typename T, int R>
__device__ __attribute__((noinline)) SrGVec<T, R> sr_grad_unary_val(uint32_t u, SrGVec<T, R> x) {
#pragma unroll
  for (int r = 0; r < R; ++r) {
    x[r] = sr_unary<T>(u, x[r]);
    __builtin_amdgcn_sched_barrier(0);
  }
  return x;
}
template <typename T, int R>
__device__ __attribute__((noinline)) SrGVec<T, R> sr_grad_unary_der(uint32_t u, SrGVec<T, R> x, SrGVec<T, R> y) {
#pragma unroll
  for (int r = 0; r < R; ++r) {
    x[r] = sr_unary_deriv<T>(u, x[r], y[r]);
    __builtin_amdgcn_sched_barrier(0);
  }
  return x;
}
template <typename T, int R>
__device__ __attribute__((noinline)) SrGVec<T, R> sr_grad_binary_val(uint32_t b, SrGVec<T, R> x, SrGVec<T, R> y) {
#pragma unroll
  for (int r = 0; r < R; ++r) {
    x[r] = sr_binary<T>(b, x[r], y[r]);
    __builtin_amdgcn_sched_barrier(0);
  }
  return x;
}
// WHICH = 0: d r / d a, 1: d r / d b
template <typename T, int R, int WHICH>
__device__ __attribute__((noinline)) SrGVec<T, R> sr_grad_binary_der(uint32_t b, SrGVec<T, R> x, SrGVec<T, R> y,
                                                                      SrGVec<T, R> res) {
#pragma unroll
  for (int r = 0; r < R; ++r) {
    T pa, pb;
    sr_binary_partials<T>(b, x[r], y[r], res[r], &pa, &pb);
    x[r] = WHICH == 0 ? pa : pb;
    __builtin_amdgcn_sched_barrier(0);
  }
  return x;
}
template <typename T, int R>
__device__ __attribute__((noinline)) SrGVec<T, R> sr_grad_loss_der(int kind, SrGVec<T, R> pred, SrGVec<T, R> y, T p) {
#pragma unroll
  for (int r = 0; r < R; ++r) {
    pred[r] = sr_elem_loss_deriv<T>(kind, pred[r], y[r], p);
    __builtin_amdgcn_sched_barrier(0);
  }
  return pred;
}

// basic_bin's operand variants for a parameter operand (beside SR_V_SL .. SR_V_CR; PARAM builds)
constexpr uint32_t SR_GV_PL = 100u, SR_GV_PR = 101u;

// R: rows per lane (sr_grad_launch_rows: up to 8 for 1-2 tangents, 4 for 4, 2 for 8, 1 for 16): the
// value and its KT tangents of R rows stay in VGPRs, so one dispatch of an instruction covers R x 64
// rows (round 3: one row per lane made every dispatch and operand decode cover 64 rows only).
//
// PARAM (sr_grad_param_kernel, ParametricExpression trees; sr_grad_param*.hip): the tile stages the
// dataset's hidden class row too (a.nf counts it), a parameter leaf p_{k+1} is SR_OP_LOAD_PARAM / a P
// binary operand whose value is the gathered P_tree[k, class[row]], and the tree's tangents are its
// nc constants followed by the parameters it USES, in ascending k (p.tan_par: a compact rank, so an
// unused parameter costs nothing).  There is ONE tangent per used parameter index, not per (k, class):
// the operand is one-hot in its own tangent slot, and d pred / d P[k, c] at a row is that tangent times
// [class[row] == c].  To every other tangent a parameter operand is a feature operand (zero tangent,
// the partial x 0 term kept), so the constants' entries are those of the tree with p_k replaced by a
// feature, bit for bit.  A constant tangent accumulates as in the plain build; a parameter tangent is
// binned by class: per 64-row group (row j of the lane's R: the same 64 rows whatever R), in row
// order, for each class present one fixed-tree wave sum of the masked coef x tangent products, added
// by the wave into its LDS bin [tangent][class]; the bins go out per row block and the row blocks are
// reduced in order (sr_launch_grad_reduce).  No atomics: the same bits run to run, for every R and
// whatever else is in the launch.
//
// LOSSX (sr_grad_lossx_kernel, expression losses; sr_grad_inst.hip): only the per-row coefficient differs —
// d value / d pred from the call's loss program by forward mode (sr_loss_expr.h), the weight handed to the
// program and not multiplied in afterwards.
template <typename T, int KT, int W, bool GATHER, int R>
__global__ void __launch_bounds__(W * 64) sr_grad_kernel(const SrGradArgs<T> a) {
#define SR_GRAD_PARAM 0
#define SR_GRAD_LOSSX 0
#define SR_GRAD_ROWOUT 0
#include "sr_grad_body.h"
#undef SR_GRAD_ROWOUT
#undef SR_GRAD_LOSSX
#undef SR_GRAD_PARAM
}
template <typename T, int KT, int W, bool GATHER, int R>
__global__ void __launch_bounds__(W * 64) sr_grad_param_kernel(const SrGradArgs<T> a, const SrGradParamArgs<T> p) {
#define SR_GRAD_PARAM 1
#define SR_GRAD_LOSSX 0
#define SR_GRAD_ROWOUT 0
#include "sr_grad_body.h"
#undef SR_GRAD_ROWOUT
#undef SR_GRAD_LOSSX
#undef SR_GRAD_PARAM
}
template <typename T, int KT, int W, bool GATHER, int R>
__global__ void __launch_bounds__(W * 64) sr_grad_lossx_kernel(const SrGradArgs<T> a, const SrLossProgArgs<T> lx) {
#define SR_GRAD_PARAM 0
#define SR_GRAD_LOSSX 1
#define SR_GRAD_ROWOUT 0
#include "sr_grad_body.h"
#undef SR_GRAD_ROWOUT
#undef SR_GRAD_LOSSX
#undef SR_GRAD_PARAM
}
// ROWOUT (sr_grad_rows_kernel, sr_eval_grad_tree_array / sr_eval_diff_tree_array; sr_grad_inst.hip): the same
// interpreter and rules, no loss: every valid row's tangents are stored ([tangent][row], rows fastest) and a
// wave ballot records a non-finite one per (row block, item).  d.feat: the tangents are the features' —
// a feature operand is one-hot in its own slot exactly as a constant operand is in the other builds, and a
// constant is what a feature is there (zero tangent, the partial x 0 term kept).  y and w are not staged.
template <typename T, int KT, int W, bool GATHER, int R>
__global__ void __launch_bounds__(W * 64) sr_grad_rows_kernel(const SrGradArgs<T> a, const SrGradRowArgs<T> d) {
#define SR_GRAD_PARAM 0
#define SR_GRAD_LOSSX 0
#define SR_GRAD_ROWOUT 1
#include "sr_grad_body.h"
#undef SR_GRAD_ROWOUT
#undef SR_GRAD_LOSSX
#undef SR_GRAD_PARAM
}

template <typename T, int KT, int W, bool GATHER, int R>
hipError_t sr_launch_grad(const SrGradArgs<T>& a, int n_blocks, hipStream_t s) {
  const size_t lds = sr_grad_lds_bytes(int(sizeof(T)), KT, R, a.nf, a.w != nullptr, a.stack_depth, W);
  const void* fn = reinterpret_cast<const void*>(&sr_grad_kernel<T, KT, W, GATHER, R>);
  if (lds > 65536) {
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, int(lds));
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL((sr_grad_kernel<T, KT, W, GATHER, R>), dim3(n_blocks), dim3(W * 64), lds, s, a);
  return hipGetLastError();
}

// Launch with `rows` rows per lane: the kernels exist for the bucket's default (sr_grad_rows_per_lane),
// its halves down to 2, and 1 (sr_grad_launch_rows picks one; results do not depend on it: the row
// blocks cover the same rows whatever the rows per lane, see sr_capi.cpp eval_grad_impl).
template <typename T, bool GATHER, int KT, int RR>
hipError_t sr_launch_grad_rows_from(const SrGradArgs<T>& a, int rows, int n_blocks, hipStream_t s) {
  if (rows == RR) return sr_launch_grad<T, KT, 4, GATHER, RR>(a, n_blocks, s);
  if constexpr (RR > 1) return sr_launch_grad_rows_from<T, GATHER, KT, RR / 2>(a, rows, n_blocks, s);
  return hipErrorInvalidValue;
}

// The parametric builds: rows per lane sr_grad_param_rows(sizeof(T), KT) and 1 (sr_grad_param_launch_rows
// picks one), one translation unit per element type and gather mode (sr_grad_inst.hip).
template <typename T, int KT, int W, bool GATHER, int R>
hipError_t sr_launch_grad_param(const SrGradArgs<T>& a, const SrGradParamArgs<T>& p, int n_blocks, hipStream_t s) {
  if (p.ptab == nullptr || p.n_classes < 1 || a.nf < 2) return hipErrorInvalidValue;
  const size_t lds = sr_grad_lds_bytes(int(sizeof(T)), KT, R, a.nf - 1, a.w != nullptr, a.stack_depth, W, p.n_classes, p.lane_slots);
  const void* fn = reinterpret_cast<const void*>(&sr_grad_param_kernel<T, KT, W, GATHER, R>);
  if (lds > 65536) {
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, int(lds));
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL((sr_grad_param_kernel<T, KT, W, GATHER, R>), dim3(n_blocks), dim3(W * 64), lds, s, a, p);
  return hipGetLastError();
}
template <typename T, bool GATHER>
hipError_t sr_launch_grad_param_any(const SrGradArgs<T>& a, const SrGradParamArgs<T>& p, int kt, int rows, int n_blocks,
                                    hipStream_t s) {
  auto go = [&](auto ktc) -> hipError_t {
    constexpr int KT = decltype(ktc)::value;
    constexpr int RR = sr_grad_param_rows(int(sizeof(T)), KT);
    if (rows == 1) return sr_launch_grad_param<T, KT, 4, GATHER, 1>(a, p, n_blocks, s);
    if constexpr (RR > 1)
      if (rows == RR) return sr_launch_grad_param<T, KT, 4, GATHER, RR>(a, p, n_blocks, s);
    return hipErrorInvalidValue;
  };
  switch (kt) {
    case 1: return go(std::integral_constant<int, 1>{});
    case 2: return go(std::integral_constant<int, 2>{});
    case 4: return go(std::integral_constant<int, 4>{});
    case 8: return go(std::integral_constant<int, 8>{});
    case 16: return go(std::integral_constant<int, 16>{});
    default: return hipErrorInvalidValue;
  }
}

// The expression-loss builds: one per tangent width, at sr_grad_param_rows rows per lane.
template <typename T, int KT, int W, bool GATHER, int R>
hipError_t sr_launch_grad_lossx(const SrGradArgs<T>& a, const SrLossProgArgs<T>& x, int n_blocks, hipStream_t s) {
  if (x.code == nullptr || x.n < 1 || x.n > SR_LX_MAX_INS || a.loss_kind != SR_LOSS_EXPR) return hipErrorInvalidValue;
  const size_t lds = sr_grad_lds_bytes(int(sizeof(T)), KT, R, a.nf, a.w != nullptr, a.stack_depth, W);
  const void* fn = reinterpret_cast<const void*>(&sr_grad_lossx_kernel<T, KT, W, GATHER, R>);
  if (lds > 65536) {
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, int(lds));
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL((sr_grad_lossx_kernel<T, KT, W, GATHER, R>), dim3(n_blocks), dim3(W * 64), lds, s, a, x);
  return hipGetLastError();
}
template <typename T, bool GATHER>
hipError_t sr_launch_grad_lossx_any(const SrGradArgs<T>& a, const SrLossProgArgs<T>& x, int kt, int rows, int n_blocks,
                                    hipStream_t s) {
  auto go = [&](auto ktc) -> hipError_t {
    constexpr int KT = decltype(ktc)::value;
    constexpr int RR = sr_grad_param_rows(int(sizeof(T)), KT);
    if (rows != RR) return hipErrorInvalidValue;
    return sr_launch_grad_lossx<T, KT, 4, GATHER, RR>(a, x, n_blocks, s);
  };
  switch (kt) {
    case 1: return go(std::integral_constant<int, 1>{});
    case 2: return go(std::integral_constant<int, 2>{});
    case 4: return go(std::integral_constant<int, 4>{});
    case 8: return go(std::integral_constant<int, 8>{});
    case 16: return go(std::integral_constant<int, 16>{});
    default: return hipErrorInvalidValue;
  }
}

// The per-row builds: the plain kernel's set of rows per lane (sr_grad_launch_rows picks one; the stored
// tangents do not depend on it), one translation unit per element type and gather mode (sr_grad_inst.hip).
template <typename T, int KT, int W, bool GATHER, int R>
hipError_t sr_launch_grad_rows(const SrGradArgs<T>& a, const SrGradRowArgs<T>& d, int n_blocks, hipStream_t s) {
  if (d.out == nullptr || d.item_out == nullptr || d.item_nq == nullptr || d.bad == nullptr) return hipErrorInvalidValue;
  const size_t lds = sr_grad_lds_bytes(int(sizeof(T)), KT, R, a.nf, false, a.stack_depth, W);
  const void* fn = reinterpret_cast<const void*>(&sr_grad_rows_kernel<T, KT, W, GATHER, R>);
  if (lds > 65536) {
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, int(lds));
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL((sr_grad_rows_kernel<T, KT, W, GATHER, R>), dim3(n_blocks), dim3(W * 64), lds, s, a, d);
  return hipGetLastError();
}
template <typename T, bool GATHER, int KT, int RR>
hipError_t sr_launch_grad_rows_rows_from(const SrGradArgs<T>& a, const SrGradRowArgs<T>& d, int rows, int n_blocks,
                                         hipStream_t s) {
  if (rows == RR) return sr_launch_grad_rows<T, KT, 4, GATHER, RR>(a, d, n_blocks, s);
  if constexpr (RR > 1) return sr_launch_grad_rows_rows_from<T, GATHER, KT, RR / 2>(a, d, rows, n_blocks, s);
  return hipErrorInvalidValue;
}
template <typename T, bool GATHER>
hipError_t sr_launch_grad_rows_any(const SrGradArgs<T>& a, const SrGradRowArgs<T>& d, int kt, int rows, int n_blocks,
                                   hipStream_t s) {
  if (a.w != nullptr) return hipErrorInvalidValue;  // (the tile holds no weights: sr_launch_grad_rows' LDS size)
  switch (kt) {
    case 1: return sr_launch_grad_rows_rows_from<T, GATHER, 1, sr_grad_rows_per_lane(1)>(a, d, rows, n_blocks, s);
    case 2: return sr_launch_grad_rows_rows_from<T, GATHER, 2, sr_grad_rows_per_lane(2)>(a, d, rows, n_blocks, s);
    case 4: return sr_launch_grad_rows_rows_from<T, GATHER, 4, sr_grad_rows_per_lane(4)>(a, d, rows, n_blocks, s);
    case 8: return sr_launch_grad_rows_rows_from<T, GATHER, 8, sr_grad_rows_per_lane(8)>(a, d, rows, n_blocks, s);
    case 16: return sr_launch_grad_rows_rows_from<T, GATHER, 16, sr_grad_rows_per_lane(16)>(a, d, rows, n_blocks, s);
    default: return hipErrorInvalidValue;
  }
}

template <typename T>
hipError_t sr_launch_grad_any(const SrGradArgs<T>& a, int kt, bool gather, int rows, int n_blocks, hipStream_t s) {
  if (a.loss_kind == SR_LOSS_EXPR) return hipErrorInvalidValue;  // (sr_launch_grad_lossx_any: never sr_elem_loss_deriv's default case)
  auto go = [&](auto g) -> hipError_t {
    constexpr bool G = decltype(g)::value;
    switch (kt) {
      case 1: return sr_launch_grad_rows_from<T, G, 1, sr_grad_rows_per_lane(1)>(a, rows, n_blocks, s);
      case 2: return sr_launch_grad_rows_from<T, G, 2, sr_grad_rows_per_lane(2)>(a, rows, n_blocks, s);
      case 4: return sr_launch_grad_rows_from<T, G, 4, sr_grad_rows_per_lane(4)>(a, rows, n_blocks, s);
      case 8: return sr_launch_grad_rows_from<T, G, 8, sr_grad_rows_per_lane(8)>(a, rows, n_blocks, s);
      case 16: return sr_launch_grad_rows_from<T, G, 16, sr_grad_rows_per_lane(16)>(a, rows, n_blocks, s);
      default: return hipErrorInvalidValue;
    }
  };
  return gather ? go(std::true_type{}) : go(std::false_type{});
}
