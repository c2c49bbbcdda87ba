// param_grad_check.cpp — stand-alone host check of the parametric GRADIENT programs and of the scalar
// packing (no GPU, no Python).
//
// Build and run through `make -C symbolicregression.jl_amd param-grad-check`, which compiles this file and
// csrc/sr_compile.cpp with -fsanitize=address,undefined.  Over 400 random trees with parameter leaves in
// Float32 and in Float64 it checks that
//   * the with_const_index program of each tree equals that of its plain twin (leaf p_k -> feature
//     x_(nfeatures + k), compiled with nfeatures + K features) in length, operand-stack depth and
//     constant slots, instruction by instruction: the same words apart from LOAD_FEAT <-> LOAD_PARAM
//     (and their PUSH forms), the F <-> P binary operand opcodes, and the operand index (nfeatures + k - 1
//     <-> k - 1) of exactly those instructions;
//   * srpp::pack -> unpack round-trips constants and matrix, the packed order is the constants then the
//     matrix as stored (column-major (k-1) + K (c-1)), scalar_offsets steps by nc + K C, the restart
//     draws one normal per entry in that order, and used_parameters is the sorted set of used indices.
// Exit status 0 and "param_grad_check: ok" on success.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../symbolicregression.jl_amd/csrc/sr_compile.h"
#include "../symbolicregression.jl_amd/csrc/sr_param_pack.h"

namespace {

struct Rng {
  uint64_t s;
  uint32_t next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return uint32_t(s >> 33);
  }
  int below(int n) { return int(next() % uint32_t(n)); }
};

// the draws a restart consumes, in order: the q-th call returns q + 1
struct CountingNormal {
  int calls = 0;
  double normal() { return double(++calls); }
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

constexpr int kNf = 3, kParams = 5, kClasses = 3, kUnary = 4, kBinary = 5;

template <typename T>
void gen(Rng& r, Batch<T>& b, int size) {
  if (size <= 1) {
    const int kind = r.below(3);
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

// the plain opcode a parametric one stands for (LOAD_FEAT(_PUSH), or the F variant of the same operator and
// side); 0xffffffff for an opcode that is not parametric
uint32_t plain_opcode(uint32_t o) {
  if (o == SR_OP_LOAD_PARAM) return SR_OP_LOAD_FEAT;
  if (o == SR_OP_LOAD_PARAM_PUSH) return SR_OP_LOAD_FEAT_PUSH;
  if (o >= SR_OP_PBIN0 && o < SR_OP_PAIR0) {
    const uint32_t b = (o - SR_OP_PBIN0) / 2u + 1u, side = (o - SR_OP_PBIN0) % 2u;
    return SR_BIN_OPC(b, side == SR_V_PL ? SR_V_FL : SR_V_FR);
  }
  return 0xffffffffu;
}

template <typename T>
int check_programs(const char* name) {
  SrOpset ops;
  for (const char* u : {"cos", "exp", "log", "sin"}) ops.unary.push_back(sr_unary_id(u));
  for (const char* o : {"+", "-", "*", "/", "^"}) ops.binary.push_back(sr_binary_id(o));
  for (uint32_t id : ops.unary)
    if (!id) return std::printf("%s: unknown unary operator\n", name), 1;
  for (uint32_t id : ops.binary)
    if (!id) return std::printf("%s: unknown binary operator\n", name), 1;
  Rng r{sizeof(T) == 4 ? 2468u : 13579u};
  Batch<T> b;
  const int n_trees = 400;
  for (int t = 0; t < n_trees; ++t) {
    gen(r, b, 1 + r.below(40));
    b.offsets.push_back(int64_t(b.degree.size()));
  }
  Batch<T> s = b;  // the plain twins
  for (size_t i = 0; i < s.degree.size(); ++i)
    if (s.is_parameter[i]) s.feature[i] = uint16_t(kNf + s.parameter[i]);
  const SrParamNodes pn{b.is_parameter.data(), b.parameter.data(), kParams};
  SrProgramBatch<T> pp, ps;
  std::string err;
  const sr_tree_batch tb = b.trees(), ts = s.trees();
  int rc = sr_compile_batch<T>(tb, ops, 5000, kNf, true, &pp, &err, nullptr, &pn);
  if (rc != SR_OK) return std::printf("%s: parametric gradient compile failed (%d): %s\n", name, rc, err.c_str()), 1;
  rc = sr_compile_batch<T>(ts, ops, 5000, kNf + kParams, true, &ps, &err);
  if (rc != SR_OK) return std::printf("%s: twin gradient compile failed (%d): %s\n", name, rc, err.c_str()), 1;
  if (pp.code.size() != ps.code.size() || pp.max_depth != ps.max_depth)
    return std::printf("%s: total length or depth differs\n", name), 1;
  int n_param = 0, n_pbin = 0;
  for (int t = 0; t < n_trees; ++t) {
    const size_t k = size_t(t);
    if (pp.offsets[k + 1] != ps.offsets[k + 1] || pp.depth[k] != ps.depth[k] || pp.n_consts[k] != ps.n_consts[k] ||
        pp.const_off[k + 1] != ps.const_off[k + 1] || pp.static_bad[k] != ps.static_bad[k])
      return std::printf("%s: tree %d: length, depth, constants or verdict differ from the twin's\n", name, t), 1;
    std::vector<uint32_t> used, seen;
    srpp::used_parameters(b.is_parameter.data(), b.parameter.data(), b.degree.data(), b.offsets[k], b.offsets[k + 1], &used);
    for (size_t i = 0; i < used.size(); ++i)
      if (used[i] >= uint32_t(kParams) || (i > 0 && used[i] <= used[i - 1]))
        return std::printf("%s: tree %d: used_parameters is not a sorted set\n", name, t), 1;
    for (uint32_t i = pp.offsets[k]; i < pp.offsets[k + 1]; ++i) {
      const SrIns<T>& a = pp.code[i];
      const SrIns<T>& c = ps.code[i];
      const uint32_t oa = a.op & SR_OP_MASK, oc = c.op & SR_OP_MASK;
      const uint32_t twin = plain_opcode(oa);
      if (twin == 0xffffffffu) {  // not parametric: the same instruction, word for word
        if (std::memcmp(&a, &c, sizeof(a)) != 0) return std::printf("%s: tree %d: instruction %u differs\n", name, t, i), 1;
        continue;
      }
      ++n_param;
      n_pbin += oa >= SR_OP_PBIN0 ? 1 : 0;
      const uint32_t ka = a.meta & SR_M_INDEX, kc = c.meta & SR_M_INDEX;
      if (twin != oc || (a.op & ~uint32_t(SR_OP_MASK)) != (c.op & ~uint32_t(SR_OP_MASK)) || ka >= uint32_t(kParams) ||
          kc != uint32_t(kNf) + ka || (a.meta & ~uint32_t(SR_M_INDEX)) != (c.meta & ~uint32_t(SR_M_INDEX)) ||
          a.c0 != c.c0 || a.c1 != c.c1)
        return std::printf("%s: tree %d: parametric instruction %u is not its twin's\n", name, t, i), 1;
      seen.push_back(ka);
    }
    if (!pp.static_bad[k])  // every used parameter has an instruction, and only those
      for (uint32_t ka : seen) {
        bool ok = false;
        for (uint32_t u : used) ok |= u == ka;
        if (!ok) return std::printf("%s: tree %d: instruction names an unused parameter\n", name, t), 1;
      }
  }
  if (n_param == 0 || n_pbin == 0) return std::printf("%s: no parameter instructions were emitted\n", name), 1;
  std::printf("%s: %d trees, %d parameter instructions (%d operands), depth %d\n", name, n_trees, n_param, n_pbin,
              pp.max_depth);
  return 0;
}

template <typename T>
int check_packing(const char* name) {
  Rng r{sizeof(T) == 4 ? 77u : 99u};
  const size_t kc = size_t(kParams) * size_t(kClasses);
  std::vector<uint32_t> ncs;
  for (int t = 0; t < 50; ++t) {
    const size_t nc = size_t(r.below(7));
    ncs.push_back(uint32_t(nc));
    std::vector<T> c(nc), m(kc), c2(nc, T(-1)), m2(kc, T(-1));
    for (T& v : c) v = T(r.below(2000) - 1000) / T(7);
    for (T& v : m) v = T(r.below(2000) - 1000) / T(3);
    std::vector<double> x;
    srpp::pack<T>(c.data(), nc, m.data(), kc, &x);
    if (x.size() != nc + kc) return std::printf("%s: packed size\n", name), 1;
    for (size_t q = 0; q < nc; ++q)
      if (x[q] != double(c[q])) return std::printf("%s: constants are not first\n", name), 1;
    // (matrix stored [class][parameter]: entry (k, c) at k + K c, right behind the constants)
    for (int cl = 0; cl < kClasses; ++cl)
      for (int k = 0; k < kParams; ++k)
        if (x[nc + size_t(k) + size_t(kParams) * size_t(cl)] != double(m[size_t(cl) * kParams + size_t(k)]))
          return std::printf("%s: matrix order\n", name), 1;
    srpp::unpack<T>(x, nc, c2.data(), m2.data(), kc);
    if (c2 != c || m2 != m) return std::printf("%s: pack -> unpack does not round-trip\n", name), 1;
    CountingNormal cn;
    std::vector<double> xt;
    srpp::draw_restart<T>(cn, x, &xt);
    if (cn.calls != int(x.size()) || xt.size() != x.size()) return std::printf("%s: restart draw count\n", name), 1;
    for (size_t q = 0; q < x.size(); ++q)
      if (xt[q] != double(T(x[q]) * (T(1) + T(0.5) * T(double(q + 1)))))
        return std::printf("%s: restart draw order\n", name), 1;
  }
  const std::vector<int64_t> off = srpp::scalar_offsets(ncs, kParams, kClasses);
  if (off.size() != ncs.size() + 1 || off[0] != 0) return std::printf("%s: scalar_offsets shape\n", name), 1;
  for (size_t t = 0; t < ncs.size(); ++t)
    if (off[t + 1] - off[t] != int64_t(ncs[t]) + int64_t(kc)) return std::printf("%s: scalar_offsets step\n", name), 1;
  return 0;
}

}  // namespace

int main() {
  if (check_programs<float>("float32") || check_programs<double>("float64")) return 1;
  if (check_packing<float>("float32") || check_packing<double>("float64")) return 1;
  std::printf("param_grad_check: ok\n");
  return 0;
}
