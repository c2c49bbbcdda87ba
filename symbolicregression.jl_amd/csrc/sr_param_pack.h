// sr_param_pack.h — the scalar vector of a ParametricExpression tree (HIP-free; tools/param_grad_check.cpp).
//
// DynamicExpressions' get_scalar_constants(::ParametricExpression) hands the optimiser
//   x = [ constants in pre-order (nc) | vec(parameters) (K x C, column-major: index (k-1) + K (c-1)) ]
// and count_constants_for_optimization is nc + K C (reference src/ParametricExpression.jl:169-171): every
// entry of the matrix is there, used by the tree or not.  sr_param_batch keeps a tree's matrix as
// [n_classes][max_parameters], which is the same linear order, so the parameter part of x, of a gradient
// and of sr_param_batch::parameters all share one layout.  Gradients of a batch are concatenated:
// tree t's nc_t + K C values start at scalar_offsets[t].
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace srpp {

// [n_trees + 1]: where each tree's scalars start in a concatenated gradient / optimiser vector
inline std::vector<int64_t> scalar_offsets(const std::vector<uint32_t>& n_consts, int64_t max_parameters, int64_t n_classes) {
  std::vector<int64_t> off(n_consts.size() + 1, 0);
  for (size_t t = 0; t < n_consts.size(); ++t) off[t + 1] = off[t] + int64_t(n_consts[t]) + max_parameters * n_classes;
  return off;
}

// x = [consts; vec(P)] in Float64
template <typename T>
inline void pack(const T* consts, size_t nc, const T* matrix, size_t kc, std::vector<double>* x) {
  x->resize(nc + kc);
  for (size_t q = 0; q < nc; ++q) (*x)[q] = double(consts[q]);
  for (size_t q = 0; q < kc; ++q) (*x)[nc + q] = double(matrix[q]);
}
// and back, rounded to T (x.size() == nc + kc)
template <typename T>
inline void unpack(const std::vector<double>& x, size_t nc, T* consts, T* matrix, size_t kc) {
  for (size_t q = 0; q < nc; ++q) consts[q] = T(x[q]);
  for (size_t q = 0; q < kc; ++q) matrix[q] = T(x[nc + q]);
}

// One restart point x0 .* (1 + eps / 2), eps = randn(rng, T, size(x0)...) (reference
// src/ConstantOptimization.jl:91-97), in T: one normal draw per entry of the WHOLE vector in its own order,
// the constants first, then the matrix column-major — unused parameters included.
template <typename T, typename Rng>
inline void draw_restart(Rng& rng, const std::vector<double>& x0, std::vector<double>* xt) {
  xt->resize(x0.size());
  for (size_t q = 0; q < x0.size(); ++q) {
    const T eps = T(rng.normal());
    (*xt)[q] = double(T(x0[q]) * (T(1) + T(0.5) * eps));
  }
}

// The parameters (0-based, ascending) that the nodes [b, e) of a batch use: the tree's parameter tangents
// in the gradient kernel's order.
inline void used_parameters(const uint8_t* is_parameter, const uint16_t* parameter, const uint8_t* degree, int64_t b,
                            int64_t e, std::vector<uint32_t>* out) {
  out->clear();
  for (int64_t i = b; i < e; ++i)
    if (degree[i] == 0 && is_parameter[i] && parameter[i] >= 1) out->push_back(uint32_t(parameter[i]) - 1u);
  // (few per tree: an insertion sort, then unique)
  for (size_t i = 1; i < out->size(); ++i)
    for (size_t j = i; j > 0 && (*out)[j - 1] > (*out)[j]; --j) {
      const uint32_t v = (*out)[j];
      (*out)[j] = (*out)[j - 1];
      (*out)[j - 1] = v;
    }
  size_t n = 0;
  for (size_t i = 0; i < out->size(); ++i)
    if (i == 0 || (*out)[i] != (*out)[i - 1]) (*out)[n++] = (*out)[i];
  out->resize(n);
}

}  // namespace srpp
