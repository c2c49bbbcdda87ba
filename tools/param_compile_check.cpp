// param_compile_check.cpp — stand-alone host check of the parametric tree compiler (no GPU, no Python).
//
// Build and run through `make -C symbolicregression.jl_amd param-check`, which compiles this file and
// csrc/sr_compile.cpp with -fsanitize=address,undefined.  It compiles a few hundred random trees with
// parameter leaves in Float32 and Float64 (one batch large enough for the compile workers' pool) and
// checks, per tree, that the static verdict, the operand-stack depth and the number of checked arrays
// equal those of the same tree with every parameter leaf p_k turned into the feature leaf
// x_(nfeatures + k); then that each malformed parameter leaf is refused with SR_ERR_BAD_TREE.
// Exit status 0 and "param_compile_check: ok" on success.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../symbolicregression.jl_amd/csrc/sr_compile.h"

namespace {

struct Rng {
  uint64_t s;
  uint32_t next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return uint32_t(s >> 33);
  }
  int below(int n) { return int(next() % uint32_t(n)); }
};

template <typename T>
struct Batch {
  std::vector<int64_t> offsets{0};
  std::vector<uint8_t> degree, op, constant, is_parameter;
  std::vector<uint16_t> feature, parameter;
  std::vector<T> val;
  sr_tree_batch trees() const {
    return sr_tree_batch{int64_t(offsets.size()) - 1, offsets.data(), degree.data(), op.data(), feature.data(),
                         constant.data(), val.data()};
  }
  void node(int d, int o, int f, bool c, T v, int p) {
    degree.push_back(uint8_t(d));
    op.push_back(uint8_t(o));
    feature.push_back(uint16_t(f));
    constant.push_back(c ? 1 : 0);
    val.push_back(v);
    is_parameter.push_back(p > 0 ? 1 : 0);
    parameter.push_back(uint16_t(p > 0 ? p : 0));
  }
};

constexpr int kNf = 3, kParams = 2, kUnary = 3, kBinary = 4;

// a random tree of about `size` nodes, pre-order
template <typename T>
void gen(Rng& r, Batch<T>& b, int size) {
  if (size <= 1) {
    const int kind = r.below(4);
    if (kind == 0) {
      const T vals[] = {T(1.5), T(-0.25), T(3e30), T(1e-3), T(0)};
      b.node(0, 0, 0, true, vals[r.below(5)], 0);
    } else if (kind == 1) {
      b.node(0, 0, 0, false, T(0), 1 + r.below(kParams));
    } else {
      b.node(0, 0, 1 + r.below(kNf), false, T(0), 0);
    }
    return;
  }
  if (size == 2 || r.below(3) == 0) {
    b.node(1, 1 + r.below(kUnary), 0, false, T(0), 0);
    gen(r, b, size - 1);
    return;
  }
  b.node(2, 1 + r.below(kBinary), 0, false, T(0), 0);
  const int left = 1 + r.below(size - 2);
  gen(r, b, left);
  gen(r, b, size - 1 - left);
}

template <typename T>
int run(const char* name) {
  SrOpset ops;
  for (const char* u : {"cos", "exp", "log"}) ops.unary.push_back(sr_unary_id(u));
  for (const char* o : {"+", "-", "*", "/"}) ops.binary.push_back(sr_binary_id(o));
  Rng r{sizeof(T) == 4 ? 12345u : 98765u};
  Batch<T> b;
  const int n_trees = 400;
  for (int t = 0; t < n_trees; ++t) {
    gen(r, b, 1 + r.below(30));
    b.offsets.push_back(int64_t(b.degree.size()));
  }
  // the substituted batch: parameter leaf p_k -> feature leaf x_(kNf + k)
  Batch<T> s = b;
  for (size_t i = 0; i < s.degree.size(); ++i)
    if (s.is_parameter[i]) s.feature[i] = uint16_t(kNf + s.parameter[i]);
  const SrParamNodes pn{b.is_parameter.data(), b.parameter.data(), kParams};
  SrProgramBatch<T> pp, ps;
  std::string err;
  const sr_tree_batch tb = b.trees(), ts = s.trees();
  int rc = sr_compile_batch<T>(tb, ops, 5000, kNf, false, &pp, &err, nullptr, &pn);
  if (rc != SR_OK) return std::printf("%s: parametric compile failed (%d): %s\n", name, rc, err.c_str()), 1;
  rc = sr_compile_batch<T>(ts, ops, 5000, kNf + kParams, false, &ps, &err);
  if (rc != SR_OK) return std::printf("%s: substituted compile failed (%d): %s\n", name, rc, err.c_str()), 1;
  int n_bad = 0, n_param = 0;
  for (int t = 0; t < n_trees; ++t) {
    if (pp.static_bad[size_t(t)] != ps.static_bad[size_t(t)] || pp.depth[size_t(t)] != ps.depth[size_t(t)] ||
        pp.n_checks[size_t(t)] != ps.n_checks[size_t(t)] ||
        pp.offsets[size_t(t) + 1] - pp.offsets[size_t(t)] < ps.offsets[size_t(t) + 1] - ps.offsets[size_t(t)])
      return std::printf("%s: tree %d differs from its substituted form\n", name, t), 1;
    n_bad += pp.static_bad[size_t(t)];
  }
  for (const auto& in : pp.code) {
    const uint32_t o = in.op & SR_OP_MASK;
    if (o >= SR_OP_LOAD_PARAM && o < SR_OP_PAIR0) {
      ++n_param;
      if ((in.meta & SR_M_INDEX) >= uint32_t(kParams)) return std::printf("%s: parameter index out of range in code\n", name), 1;
    }
  }
  if (pp.max_depth != ps.max_depth) return std::printf("%s: max depth differs\n", name), 1;
  if (n_param == 0) return std::printf("%s: no parameter instructions were emitted\n", name), 1;
  // malformed parameter leaves: index 0, index above max_parameters, on an operator node, with constant
  struct Case {
    const char* what;
    int degree, param, is_param;
    bool constant;
  };
  const Case cases[] = {{"parameter 0", 0, 0, 1, false},
                        {"parameter above max_parameters", 0, kParams + 1, 1, false},
                        {"is_parameter on an operator", 1, 1, 1, false},
                        {"is_parameter with constant", 0, 1, 1, true}};
  for (const Case& c : cases) {
    Batch<T> m;
    m.node(c.degree, 1, 1, c.constant, T(1), 0);
    m.is_parameter[0] = uint8_t(c.is_param);
    m.parameter[0] = uint16_t(c.param);
    if (c.degree == 1) m.node(0, 0, 1, false, T(0), 0);
    m.offsets.push_back(int64_t(m.degree.size()));
    const SrParamNodes mn{m.is_parameter.data(), m.parameter.data(), kParams};
    SrProgramBatch<T> mp;
    const sr_tree_batch mt = m.trees();
    rc = sr_compile_batch<T>(mt, ops, 100, kNf, false, &mp, &err, nullptr, &mn);
    if (rc != SR_ERR_BAD_TREE) return std::printf("%s: %s gave %d, not SR_ERR_BAD_TREE\n", name, c.what, rc), 1;
  }
  std::printf("%s: %d trees, %d statically incomplete, %d parameter instructions, depth %d\n", name, n_trees, n_bad,
              n_param, pp.max_depth);
  return 0;
}

}  // namespace

int main() {
  if (run<float>("float32") || run<double>("float64")) return 1;
  std::printf("param_compile_check: ok\n");
  return 0;
}
