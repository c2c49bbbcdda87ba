// sr_loss_expr.h — elementwise losses given as expressions (host + device, no HIP runtime needed).
//
// The reference takes `elementwise_loss = (x, y) -> ...` or `(x, y, w) -> ...` (src/LossFunctions.jl:38-58):
// a Julia closure the device cannot run.  What it can run is an expression over (prediction, target,
// weight) built from the operator catalog of sr_ops.h.  This header holds
//   * the loss program: a short postfix program over a 4-deep stack of live values;
//   * its compiler (host): one pre-order tree (the node fields of sr_tree_batch; leaves: feature 1 =
//     prediction, 2 = target, 3 = weight, and constants) -> program, constant subtrees folded;
//   * two interpreters (host and device, the same text): value = L(pred, y, w), and d value / d pred
//     by forward mode — a (value, tangent) pair per live value, sr_unary_deriv / sr_binary_partials per
//     node, the kink conventions of those functions.
//
// Arithmetic: the tree's constants arrive as Float64 and are rounded to T; every operation, the folding
// of constant subtrees included, is in T — what a type-stable Julia loss on Dataset{T} does.  Nothing is
// fused: every node rounds separately (-ffp-contract=off, as the tree programs).
//
// Program: SrIns<T> instructions (16 bytes; constant in c0 / c1), op word =
//   kind | id << 8 | srcA << 16 | srcB << 20 | DX << 24 | DY << 25
//   kind  SR_LX_PUSH     push A
//         SR_LX_UNARY    s0 <- u(s0)
//         SR_LX_BIN_SS   s0 <- b(s1, s0), pop      (left child evaluated first)
//         SR_LX_BIN_SW   s0 <- b(s0, s1), pop      (right child evaluated first: the swapped-operand form)
//         SR_LX_BIN_SL   s0 <- b(s0, A)            (leaf-operand forms: the leaf costs no live value)
//         SR_LX_BIN_LS   s0 <- b(A, s0)
//         SR_LX_BIN_LL   push b(A, B)
//   id    SrUnaryOp / SrBinaryOp;  src: SR_LX_PRED / _TARGET / _WEIGHT / _CONST (one constant per
//         instruction: a node with two constant operands has been folded)
//   DX / DY: the first / second operand depends on the prediction (forward mode: an operand that does not
//         is a plain number, as the target and weight are in the reference's Dual arithmetic — it adds no
//         partial-times-zero term, so an infinite partial on that side cannot make a NaN)
// The child needing more live values is evaluated first, so a tree needs
//   live(leaf) = 1, live(u(x)) = live(x), live(b(leaf, leaf)) = 1, live(b(x, leaf)) = live(x),
//   live(b(x, y)) = max(hi, lo + 1) for hi >= lo the children's counts
// live values; chains of any length whose nodes have a leaf operand need one.
//
// Limits (checked by sr_lx_compile, never a truncated program): SR_LX_MAX_NODES nodes, SR_LX_MAX_INS
// instructions after folding, SR_LX_MAX_LIVE live values.  Every tree of up to 31 nodes needing at most 4
// live values is inside them.
#pragma once
#include <stdint.h>

#include <string>
#include <utility>
#include <vector>

#include "sr_ops.h"

enum : uint32_t {
  SR_LX_PUSH = 0u, SR_LX_UNARY = 1u, SR_LX_BIN_SS = 2u, SR_LX_BIN_SW = 3u, SR_LX_BIN_SL = 4u, SR_LX_BIN_LS = 5u,
  SR_LX_BIN_LL = 6u,
  SR_LX_PRED = 0u, SR_LX_TARGET = 1u, SR_LX_WEIGHT = 2u, SR_LX_CONST = 3u,
  SR_LX_ID_SHIFT = 8u, SR_LX_A_SHIFT = 16u, SR_LX_B_SHIFT = 20u, SR_LX_DX = 1u << 24, SR_LX_DY = 1u << 25,
};
constexpr int SR_LX_MAX_NODES = 127;
constexpr int SR_LX_MAX_INS = 64;
constexpr int SR_LX_MAX_LIVE = 4;

// A compiled loss (host copy; the device holds `ins` in a buffer of its own).
template <typename T>
struct SrLossProg {
  int32_t n = 0;         // instructions
  int32_t uses_w = 0;    // the expression references the weight
  int32_t max_live = 0;  // live values the program needs (<= SR_LX_MAX_LIVE)
  int32_t grad_ok = 1;   // every operator has a derivative rule (sr_unary_grad_supported / binary)
  SrIns<T> ins[SR_LX_MAX_INS];
};
// What a kernel gets: the program in device memory (read with wave-uniform loads) and its length.
template <typename T>
struct SrLossProgArgs {
  const SrIns<T>* code;
  int n;
};

// R values of one lane (rows of a tile) or of the host's loop: an ext vector where the compiler has them
// (a by-value argument of a device call then travels in registers), a plain struct elsewhere.
#if defined(__clang__)
template <typename T, int R>
using SrLxVec = T __attribute__((ext_vector_type(R)));
#else
template <typename T, int R>
struct SrLxVec {
  T v[R];
  SR_HD T& operator[](int i) { return v[i]; }
  SR_HD const T& operator[](int i) const { return v[i]; }
};
#endif

// ---------------------------------------------------------------------------------------
// Row operations: the host's (and any inlined use's) plain loops; SrLxDevOps below for the kernels.
// ---------------------------------------------------------------------------------------
template <typename T, int R>
struct SrLxPlainOps {
  using V = SrLxVec<T, R>;
  static SR_HD inline V unary_val(uint32_t u, V x) {
    for (int r = 0; r < R; ++r) x[r] = sr_unary<T>(u, x[r]);
    return x;
  }
  static SR_HD inline V unary_der(uint32_t u, V x, V y) {
    for (int r = 0; r < R; ++r) x[r] = sr_unary_deriv<T>(u, x[r], y[r]);
    return x;
  }
  static SR_HD inline V binary_val(uint32_t b, V x, V y) {
    for (int r = 0; r < R; ++r) x[r] = sr_binary<T>(b, x[r], y[r]);
    return x;
  }
  template <int WHICH>
  static SR_HD inline V binary_der(uint32_t b, V x, V y, V res) {
    for (int r = 0; r < R; ++r) {
      T pa, pb;
      sr_binary_partials<T>(b, x[r], y[r], res[r], &pa, &pb);
      x[r] = WHICH == 0 ? pa : pb;
    }
    return x;
  }
};

#if defined(__HIPCC__)
// The kernels' row operations: callees of their own (noinline, as the gradient kernel's row callees: the
// largest operator body does not set the interpreter loop's register count), ONE dispatch on the operator
// per instruction, the lane's R rows inside it.
// (the rows by pack expansion, not a loop: every row's element index is a constant whatever the
//  optimizer makes of the operator body)
template <typename T, uint32_t ID, typename V, int... I>
__device__ __forceinline__ void sr_lx_unary_each(V& x, std::integer_sequence<int, I...>) {
  ((x[I] = sr_unary<T>(ID, x[I]), __builtin_amdgcn_sched_barrier(0)), ...);
}
template <typename T, uint32_t ID, typename V, int... I>
__device__ __forceinline__ void sr_lx_binary_each(V& x, const V& y, std::integer_sequence<int, I...>) {
  ((x[I] = sr_binary<T>(ID, x[I], y[I]), __builtin_amdgcn_sched_barrier(0)), ...);
}
#define SR_LX_UCASE(ID)                                                              \
  case ID:                                                                           \
    sr_lx_unary_each<T, ID>(x, std::make_integer_sequence<int, R>{});                \
    break;
#define SR_LX_BCASE(ID)                                                              \
  case ID:                                                                           \
    sr_lx_binary_each<T, ID>(x, y, std::make_integer_sequence<int, R>{});            \
    break;
template <typename T, int R>
__device__ __attribute__((noinline)) SrLxVec<T, R> sr_lx_unary_rows(uint32_t u, SrLxVec<T, R> x) {
  switch (u) {
    SR_LX_UCASE(SR_U_NEG) SR_LX_UCASE(SR_U_SQUARE) SR_LX_UCASE(SR_U_CUBE) SR_LX_UCASE(SR_U_EXP) SR_LX_UCASE(SR_U_COS)
    SR_LX_UCASE(SR_U_SIN) SR_LX_UCASE(SR_U_TAN) SR_LX_UCASE(SR_U_LOG) SR_LX_UCASE(SR_U_LOG2) SR_LX_UCASE(SR_U_LOG10)
    SR_LX_UCASE(SR_U_LOG1P) SR_LX_UCASE(SR_U_SQRT) SR_LX_UCASE(SR_U_ABS) SR_LX_UCASE(SR_U_SIGN) SR_LX_UCASE(SR_U_TANH)
    SR_LX_UCASE(SR_U_SINH) SR_LX_UCASE(SR_U_COSH) SR_LX_UCASE(SR_U_ATAN) SR_LX_UCASE(SR_U_ASIN) SR_LX_UCASE(SR_U_ACOS)
    SR_LX_UCASE(SR_U_ACOSH) SR_LX_UCASE(SR_U_ATANH) SR_LX_UCASE(SR_U_ASINH) SR_LX_UCASE(SR_U_RELU) SR_LX_UCASE(SR_U_INV)
    SR_LX_UCASE(SR_U_ERF) SR_LX_UCASE(SR_U_ERFC) SR_LX_UCASE(SR_U_GAMMA) SR_LX_UCASE(SR_U_ROUND) SR_LX_UCASE(SR_U_FLOOR)
    SR_LX_UCASE(SR_U_CEIL) SR_LX_UCASE(SR_U_EXP2) SR_LX_UCASE(SR_U_EXPM1)
    default:
#pragma unroll
      for (int r = 0; r < R; ++r) x[r] = sr_qnan<T>();
      break;
  }
  return x;
}
template <typename T, int R>
__device__ __attribute__((noinline)) SrLxVec<T, R> sr_lx_binary_rows(uint32_t b, SrLxVec<T, R> x, SrLxVec<T, R> y) {
  switch (b) {
    SR_LX_BCASE(SR_B_ADD) SR_LX_BCASE(SR_B_SUB) SR_LX_BCASE(SR_B_MUL) SR_LX_BCASE(SR_B_DIV) SR_LX_BCASE(SR_B_POW)
    SR_LX_BCASE(SR_B_MAX) SR_LX_BCASE(SR_B_MIN) SR_LX_BCASE(SR_B_MOD) SR_LX_BCASE(SR_B_GREATER) SR_LX_BCASE(SR_B_LESS)
    SR_LX_BCASE(SR_B_GREATER_EQUAL) SR_LX_BCASE(SR_B_LESS_EQUAL) SR_LX_BCASE(SR_B_COND) SR_LX_BCASE(SR_B_LOGICAL_OR)
    SR_LX_BCASE(SR_B_LOGICAL_AND) SR_LX_BCASE(SR_B_ATAN2)
    default:
#pragma unroll
      for (int r = 0; r < R; ++r) x[r] = sr_qnan<T>();
      break;
  }
  return x;
}
#undef SR_LX_UCASE
#undef SR_LX_BCASE
template <typename T, int R>
__device__ __attribute__((noinline)) SrLxVec<T, R> sr_lx_unary_der_rows(uint32_t u, SrLxVec<T, R> x, SrLxVec<T, R> y) {
#pragma unroll
  for (int r = 0; r < R; ++r) {
    x[r] = sr_unary_deriv<T>(u, x[r], y[r]);
    __builtin_amdgcn_sched_barrier(0);
  }
  return x;
}
template <typename T, int R, int WHICH>
__device__ __attribute__((noinline)) SrLxVec<T, R> sr_lx_binary_der_rows(uint32_t b, SrLxVec<T, R> x, SrLxVec<T, R> y,
                                                                         SrLxVec<T, R> res) {
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
struct SrLxDevOps {
  using V = SrLxVec<T, R>;
  static __device__ __forceinline__ V unary_val(uint32_t u, V x) { return sr_lx_unary_rows<T, R>(u, x); }
  static __device__ __forceinline__ V unary_der(uint32_t u, V x, V y) { return sr_lx_unary_der_rows<T, R>(u, x, y); }
  static __device__ __forceinline__ V binary_val(uint32_t b, V x, V y) { return sr_lx_binary_rows<T, R>(b, x, y); }
  template <int WHICH>
  static __device__ __forceinline__ V binary_der(uint32_t b, V x, V y, V res) {
    return sr_lx_binary_der_rows<T, R, WHICH>(b, x, y, res);
  }
};
#endif  // __HIPCC__

// ---------------------------------------------------------------------------------------
// Interpreters.  The live values are four named R-vectors (s0 = top) shifted by push and pop: no
// runtime-indexed per-lane array (those go to scratch).  `code`, `n` and every branch are uniform.
// ---------------------------------------------------------------------------------------
template <typename T, int R>
SR_HD inline SrLxVec<T, R> sr_lx_leaf(uint32_t src, const SrLxVec<T, R>& p, const SrLxVec<T, R>& y,
                                      const SrLxVec<T, R>& w, T c) {
  if (src == SR_LX_PRED) return p;
  if (src == SR_LX_TARGET) return y;
  if (src == SR_LX_WEIGHT) return w;
  SrLxVec<T, R> v;
  for (int r = 0; r < R; ++r) v[r] = c;
  return v;
}

// value = L(pred, y, w)
template <typename T, int R, typename OPS>
SR_HD inline SrLxVec<T, R> sr_lx_value(const SrIns<T>* code, int n, SrLxVec<T, R> p, SrLxVec<T, R> y, SrLxVec<T, R> w) {
  using V = SrLxVec<T, R>;
  V s0 = p, s1 = p, s2 = p, s3 = p;
  for (int i = 0; i < n; ++i) {
    const SrIns<T> in = code[i];
    const uint32_t kind = in.op & 0xffu, id = (in.op >> SR_LX_ID_SHIFT) & 0xffu;
    const V A = sr_lx_leaf<T, R>((in.op >> SR_LX_A_SHIFT) & 0xfu, p, y, w, in.value());
    if (kind == SR_LX_PUSH) {
      s3 = s2; s2 = s1; s1 = s0; s0 = A;
    } else if (kind == SR_LX_UNARY) {
      s0 = OPS::unary_val(id, s0);
    } else {
      const V B = sr_lx_leaf<T, R>((in.op >> SR_LX_B_SHIFT) & 0xfu, p, y, w, in.value());
      const V X = kind == SR_LX_BIN_SS ? s1 : ((kind == SR_LX_BIN_SW || kind == SR_LX_BIN_SL) ? s0 : A);
      const V Y = kind == SR_LX_BIN_SS ? s0 : (kind == SR_LX_BIN_SW ? s1 : (kind == SR_LX_BIN_SL ? A : (kind == SR_LX_BIN_LS ? s0 : B)));
      const V r = OPS::binary_val(id, X, Y);
      if (kind == SR_LX_BIN_SS || kind == SR_LX_BIN_SW) {
        s1 = s2; s2 = s3;
      } else if (kind == SR_LX_BIN_LL) {
        s3 = s2; s2 = s1; s1 = s0;
      }
      s0 = r;
    }
  }
  return s0;
}

// d value / d pred by forward mode (*value, when given, gets the value)
template <typename T, int R, typename OPS>
SR_HD inline SrLxVec<T, R> sr_lx_deriv(const SrIns<T>* code, int n, SrLxVec<T, R> p, SrLxVec<T, R> y, SrLxVec<T, R> w,
                                       SrLxVec<T, R>* value = nullptr) {
  using V = SrLxVec<T, R>;
  V zero, one;
  for (int r = 0; r < R; ++r) {
    zero[r] = T(0);
    one[r] = T(1);
  }
  V s0 = p, s1 = p, s2 = p, s3 = p;
  V d0 = zero, d1 = zero, d2 = zero, d3 = zero;
  for (int i = 0; i < n; ++i) {
    const SrIns<T> in = code[i];
    const uint32_t kind = in.op & 0xffu, id = (in.op >> SR_LX_ID_SHIFT) & 0xffu;
    const uint32_t sa = (in.op >> SR_LX_A_SHIFT) & 0xfu, sb = (in.op >> SR_LX_B_SHIFT) & 0xfu;
    const V A = sr_lx_leaf<T, R>(sa, p, y, w, in.value());
    const V dA = sa == SR_LX_PRED ? one : zero;
    if (kind == SR_LX_PUSH) {
      s3 = s2; s2 = s1; s1 = s0; s0 = A;
      d3 = d2; d2 = d1; d1 = d0; d0 = dA;
    } else if (kind == SR_LX_UNARY) {
      const V r = OPS::unary_val(id, s0);
      if (in.op & SR_LX_DX) {
        const V g = OPS::unary_der(id, s0, r);
        for (int q = 0; q < R; ++q) d0[q] = g[q] * d0[q];
      }
      s0 = r;
    } else {
      const V B = sr_lx_leaf<T, R>(sb, p, y, w, in.value());
      const V dB = sb == SR_LX_PRED ? one : zero;
      const V X = kind == SR_LX_BIN_SS ? s1 : ((kind == SR_LX_BIN_SW || kind == SR_LX_BIN_SL) ? s0 : A);
      const V Y = kind == SR_LX_BIN_SS ? s0 : (kind == SR_LX_BIN_SW ? s1 : (kind == SR_LX_BIN_SL ? A : (kind == SR_LX_BIN_LS ? s0 : B)));
      const V dX = kind == SR_LX_BIN_SS ? d1 : ((kind == SR_LX_BIN_SW || kind == SR_LX_BIN_SL) ? d0 : dA);
      const V dY = kind == SR_LX_BIN_SS ? d0 : (kind == SR_LX_BIN_SW ? d1 : (kind == SR_LX_BIN_SL ? dA : (kind == SR_LX_BIN_LS ? d0 : dB)));
      const V r = OPS::binary_val(id, X, Y);
      V dr = zero;
      if (in.op & SR_LX_DX) {
        const V g = OPS::template binary_der<0>(id, X, Y, r);
        for (int q = 0; q < R; ++q) dr[q] = g[q] * dX[q];
      }
      if (in.op & SR_LX_DY) {
        const V g = OPS::template binary_der<1>(id, X, Y, r);
        for (int q = 0; q < R; ++q) dr[q] = dr[q] + g[q] * dY[q];
      }
      if (kind == SR_LX_BIN_SS || kind == SR_LX_BIN_SW) {
        s1 = s2; s2 = s3;
        d1 = d2; d2 = d3;
      } else if (kind == SR_LX_BIN_LL) {
        s3 = s2; s2 = s1; s1 = s0;
        d3 = d2; d2 = d1; d1 = d0;
      }
      s0 = r;
      d0 = dr;
    }
  }
  if (value) *value = s0;
  return d0;
}

// ---------------------------------------------------------------------------------------
// Compiler (host).
// ---------------------------------------------------------------------------------------
// The operator lists are SrUnaryOp / SrBinaryOp ids (a tree node's `op` is a 1-based index into them);
// the arrays are one tree's node fields in pre-order, `val` Float64.  0 on success; -1 with *err set for a
// malformed tree, an unknown operator or leaf, or a tree beyond the limits above.
template <typename T>
inline int sr_lx_compile(const uint32_t* unary_ids, int n_unary, const uint32_t* binary_ids, int n_binary,
                         const uint8_t* degree, const uint8_t* op, const uint16_t* feature, const uint8_t* constant,
                         const double* val, int64_t n_nodes, SrLossProg<T>* out, std::string* err) {
  auto fail = [&](const std::string& m) {
    if (err) *err = "loss expression: " + m;
    return -1;
  };
  if (!degree || !op || !feature || !constant || !val) return fail("NULL node arrays");
  if (n_nodes < 1) return fail("empty tree");
  if (n_nodes > SR_LX_MAX_NODES)
    return fail(std::to_string(n_nodes) + " nodes; the limit is " + std::to_string(SR_LX_MAX_NODES));
  const int N = int(n_nodes);
  struct Node {
    int l = -1, r = -1;
    uint32_t id = 0;      // operator id
    uint32_t src = 0;     // leaf source
    bool is_const = false, dep = false;  // constant subtree; depends on the prediction
    T c = T(0);
    int live = 1;
  };
  std::vector<Node> nd(static_cast<size_t>(N));
  // children from the pre-order degrees (explicit stack of nodes still waiting for children)
  {
    std::vector<int> open;
    for (int i = 0; i < N; ++i) {
      if (degree[i] > 2) return fail("node degree " + std::to_string(int(degree[i])));
      if (i > 0) {
        if (open.empty()) return fail("nodes after the end of the tree");
        const int par = open.back();
        if (nd[size_t(par)].l < 0) nd[size_t(par)].l = i;
        else nd[size_t(par)].r = i;
        const int want = degree[par];
        if ((want == 1) || nd[size_t(par)].r >= 0) open.pop_back();
      }
      if (degree[i] > 0) open.push_back(i);
    }
    if (!open.empty()) return fail("tree ends before its last operator has its operands");
  }
  out->uses_w = 0;
  out->grad_ok = 1;
  for (int i = N - 1; i >= 0; --i) {  // children before parents
    Node& x = nd[size_t(i)];
    if (degree[i] == 0) {
      if (constant[i]) {
        x.src = SR_LX_CONST;
        x.is_const = true;
        x.c = T(val[i]);
      } else {
        if (feature[i] < 1 || feature[i] > 3)
          return fail("leaf feature " + std::to_string(int(feature[i])) + " (1 = prediction, 2 = target, 3 = weight)");
        x.src = uint32_t(feature[i]) - 1u;
        x.dep = x.src == SR_LX_PRED;
        if (x.src == SR_LX_WEIGHT) out->uses_w = 1;
      }
      x.live = 1;
    } else if (degree[i] == 1) {
      if (op[i] < 1 || int(op[i]) > n_unary) return fail("unary operator index " + std::to_string(int(op[i])));
      x.id = unary_ids[op[i] - 1];
      if (x.id == SR_U_NONE || x.id >= SR_U_COUNT) return fail("unary operator outside the device catalog");
      if (!sr_unary_grad_supported(x.id)) out->grad_ok = 0;
      const Node& a = nd[size_t(x.l)];
      x.is_const = a.is_const;
      x.dep = a.dep;
      if (x.is_const) x.c = sr_unary<T>(x.id, a.c);
      x.live = a.live;
    } else {
      if (op[i] < 1 || int(op[i]) > n_binary) return fail("binary operator index " + std::to_string(int(op[i])));
      x.id = binary_ids[op[i] - 1];
      if (x.id == SR_B_NONE || x.id >= SR_B_COUNT) return fail("binary operator outside the device catalog");
      const Node& a = nd[size_t(x.l)];
      const Node& b = nd[size_t(x.r)];
      x.is_const = a.is_const && b.is_const;
      x.dep = a.dep || b.dep;
      if (x.is_const) x.c = sr_binary<T>(x.id, a.c, b.c);
    }
  }
  // a folded constant subtree is a constant leaf from here on
  auto is_leaf = [&](int i) { return degree[i] == 0 || nd[size_t(i)].is_const; };
  for (int i = N - 1; i >= 0; --i) {
    Node& x = nd[size_t(i)];
    if (is_leaf(i)) {
      if (x.is_const) x.src = SR_LX_CONST;
      x.live = 1;
    } else if (degree[i] == 1) {
      x.live = nd[size_t(x.l)].live;
    } else {
      const bool ll = is_leaf(x.l), rl = is_leaf(x.r);
      const int a = nd[size_t(x.l)].live, b = nd[size_t(x.r)].live;
      x.live = (ll && rl) ? 1 : (ll ? b : (rl ? a : (a == b ? a + 1 : (a > b ? a : b))));
    }
  }
  if (nd[0].live > SR_LX_MAX_LIVE)
    return fail("needs " + std::to_string(nd[0].live) + " live values; the limit is " + std::to_string(SR_LX_MAX_LIVE));
  // emit (explicit stack: phase 0 = descend, 1 = emit the node's own instruction)
  int n = 0;
  bool overflow = false;
  auto emit = [&](uint32_t kind, uint32_t id, uint32_t sa, uint32_t sb, uint32_t flags, T c) {
    if (n >= SR_LX_MAX_INS) {
      overflow = true;
      return;
    }
    SrIns<T>& in = out->ins[n++];
    in.op = kind | (id << SR_LX_ID_SHIFT) | (sa << SR_LX_A_SHIFT) | (sb << SR_LX_B_SHIFT) | flags;
    in.meta = 0u;
    in.set_value(c);
  };
  struct Frame { int node; int phase; uint32_t kind; };
  std::vector<Frame> st;
  st.push_back({0, 0, 0u});
  while (!st.empty() && !overflow) {
    Frame f = st.back();
    st.pop_back();
    const Node& x = nd[size_t(f.node)];
    if (f.phase == 0) {
      if (is_leaf(f.node)) {
        emit(SR_LX_PUSH, 0u, x.src, 0u, 0u, x.c);
      } else if (degree[f.node] == 1) {
        st.push_back({f.node, 1, SR_LX_UNARY});
        st.push_back({x.l, 0, 0u});
      } else {
        const bool ll = is_leaf(x.l), rl = is_leaf(x.r);
        if (ll && rl) {
          st.push_back({f.node, 1, SR_LX_BIN_LL});
        } else if (rl) {
          st.push_back({f.node, 1, SR_LX_BIN_SL});
          st.push_back({x.l, 0, 0u});
        } else if (ll) {
          st.push_back({f.node, 1, SR_LX_BIN_LS});
          st.push_back({x.r, 0, 0u});
        } else if (nd[size_t(x.l)].live >= nd[size_t(x.r)].live) {
          st.push_back({f.node, 1, SR_LX_BIN_SS});
          st.push_back({x.r, 0, 0u});
          st.push_back({x.l, 0, 0u});  // (popped first: the left child runs first)
        } else {
          st.push_back({f.node, 1, SR_LX_BIN_SW});
          st.push_back({x.l, 0, 0u});
          st.push_back({x.r, 0, 0u});
        }
      }
    } else if (f.kind == SR_LX_UNARY) {
      emit(SR_LX_UNARY, x.id, 0u, 0u, nd[size_t(x.l)].dep ? SR_LX_DX : 0u, T(0));
    } else {
      const Node& a = nd[size_t(x.l)];
      const Node& b = nd[size_t(x.r)];
      // operands as the interpreter names them: X, Y = the operator's first and second argument
      const uint32_t flags = (a.dep ? SR_LX_DX : 0u) | (b.dep ? SR_LX_DY : 0u);
      uint32_t sa = 0u, sb = 0u;
      T c = T(0);
      if (f.kind == SR_LX_BIN_LL) {
        sa = a.src;
        sb = b.src;
        c = a.src == SR_LX_CONST ? a.c : b.c;
      } else if (f.kind == SR_LX_BIN_SL) {
        sa = b.src;
        c = b.c;
      } else if (f.kind == SR_LX_BIN_LS) {
        sa = a.src;
        c = a.c;
      }
      emit(f.kind, x.id, sa, sb, flags, c);
    }
  }
  if (overflow)
    return fail("more than " + std::to_string(SR_LX_MAX_INS) + " instructions after constant folding");
  out->n = n;
  out->max_live = nd[0].live;
  return 0;
}

// The host's interpreter over n elements (w may be NULL: the expression must not reference it).
template <typename T>
inline void sr_lx_host_eval(const SrLossProg<T>& prog, int64_t n, const T* pred, const T* y, const T* w, T* out_value,
                            T* out_dvalue) {
  using V = SrLxVec<T, 1>;
  for (int64_t i = 0; i < n; ++i) {
    V p, t, ww, v;
    p[0] = pred[i];
    t[0] = y[i];
    ww[0] = w ? w[i] : T(1);
    if (out_dvalue) {
      const V d = sr_lx_deriv<T, 1, SrLxPlainOps<T, 1>>(prog.ins, prog.n, p, t, ww, &v);
      out_dvalue[i] = d[0];
    } else {
      v = sr_lx_value<T, 1, SrLxPlainOps<T, 1>>(prog.ins, prog.n, p, t, ww);
    }
    if (out_value) out_value[i] = v[0];
  }
}
