// loss_expr_check.cpp — stand-alone host check of the expression-loss compiler and interpreters
// (csrc/sr_loss_expr.h; no GPU, no HIP, no Python).
//
// Build and run through `make -C symbolicregression.jl_amd loss-expr-check`, which compiles this file with
// -fsanitize=address,undefined.  Over a few hundred random loss trees per element type it checks that
//   * a tree is accepted exactly when it is within the limits (nodes, live values by this file's own
//     count), and a rejected one comes back with an error message;
//   * the compiled program's value equals a direct recursive evaluation of the tree bit for bit;
//   * the program never holds more than its declared live values (<= SR_LX_MAX_LIVE) and ends with one;
//   * on smooth operator sets the forward-mode derivative agrees with central differences in double;
// then that the malformed and oversized trees are refused.  Exit status 0 and "loss_expr_check: ok".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../symbolicregression.jl_amd/csrc/sr_loss_expr.h"

namespace {

struct Rng {
  uint64_t s;
  uint32_t next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return uint32_t(s >> 33);
  }
  int below(int n) { return int(next() % uint32_t(n)); }
  double unit() { return double(next()) / 2147483648.0; }  // [0, 1)
};

struct Tree {
  std::vector<uint8_t> degree, op, constant;
  std::vector<uint16_t> feature;
  std::vector<double> val;
  void node(int d, int o, int f, bool c, double v) {
    degree.push_back(uint8_t(d));
    op.push_back(uint8_t(o));
    feature.push_back(uint16_t(f));
    constant.push_back(c ? 1 : 0);
    val.push_back(v);
  }
  int64_t size() const { return int64_t(degree.size()); }
};

struct Ops {
  std::vector<uint32_t> unary, binary;
};

// a random tree of exactly `size` nodes, pre-order
void gen(Rng& r, const Ops& ops, Tree& t, int size, bool with_w, bool balanced = false) {
  if (balanced && size >= 3) {  // (halves, unary nodes over the leaves: many live values)
    t.node(2, 1 + r.below(int(ops.binary.size())), 0, false, 0.0);
    gen(r, ops, t, (size - 1) / 2, with_w, true);
    gen(r, ops, t, size - 1 - (size - 1) / 2, with_w, true);
    return;
  }
  if (size <= 1) {
    const int k = r.below(4);
    if (k == 0) {
      const double vals[] = {1.5, -0.25, 0.1, 2.0, 0.0, 1.0 / 3.0};
      t.node(0, 0, 0, true, vals[r.below(6)]);
    } else {
      t.node(0, 0, (k == 3 && !with_w) ? 1 : k, false, 0.0);
    }
    return;
  }
  if (size == 2 || r.below(3) == 0) {
    t.node(1, 1 + r.below(int(ops.unary.size())), 0, false, 0.0);
    gen(r, ops, t, size - 1, with_w);
    return;
  }
  t.node(2, 1 + r.below(int(ops.binary.size())), 0, false, 0.0);
  const int left = 1 + r.below(size - 2);
  gen(r, ops, t, left, with_w);
  gen(r, ops, t, size - 1 - left, with_w);
}

// direct recursive evaluation in T (the reference for the compiled program); *is_const: constant subtree
template <typename T>
T eval(const Tree& t, const Ops& ops, int& i, T p, T y, T w, bool* is_const) {
  const int me = i++;
  if (t.degree[me] == 0) {
    *is_const = t.constant[me] != 0;
    if (t.constant[me]) return T(t.val[me]);
    return t.feature[me] == 1 ? p : (t.feature[me] == 2 ? y : w);
  }
  if (t.degree[me] == 1) {
    const T a = eval<T>(t, ops, i, p, y, w, is_const);
    return sr_unary<T>(ops.unary[t.op[me] - 1], a);
  }
  bool ca = false, cb = false;
  const T a = eval<T>(t, ops, i, p, y, w, &ca);
  const T b = eval<T>(t, ops, i, p, y, w, &cb);
  *is_const = ca && cb;
  return sr_binary<T>(ops.binary[t.op[me] - 1], a, b);
}

// live values by the header's rule, counted here on the tree itself; leaf: a leaf or a constant subtree
int live(const Tree& t, int& i, bool* leaf, bool* is_const) {
  const int me = i++;
  if (t.degree[me] == 0) {
    *leaf = true;
    *is_const = t.constant[me] != 0;
    return 1;
  }
  if (t.degree[me] == 1) {
    bool l = false;
    const int a = live(t, i, &l, is_const);
    *leaf = *is_const;
    return *is_const ? 1 : a;
  }
  bool la = false, lb = false, ca = false, cb = false;
  const int a = live(t, i, &la, &ca);
  const int b = live(t, i, &lb, &cb);
  *is_const = ca && cb;
  *leaf = *is_const;
  if (*is_const || (la && lb)) return 1;
  if (la) return b;
  if (lb) return a;
  return a == b ? a + 1 : (a > b ? a : b);
}

template <typename T>
bool same_bits(T a, T b) {
  if (a != a && b != b) return true;
  return std::memcmp(&a, &b, sizeof(T)) == 0;
}

int g_fail = 0;
#define CHECK(cond, ...)                 \
  do {                                   \
    if (!(cond)) {                       \
      std::fprintf(stderr, __VA_ARGS__); \
      std::fprintf(stderr, "\n");        \
      ++g_fail;                          \
    }                                    \
  } while (0)

template <typename T>
int compile(const Tree& t, const Ops& ops, SrLossProg<T>* prog, std::string* err) {
  return sr_lx_compile<T>(ops.unary.data(), int(ops.unary.size()), ops.binary.data(), int(ops.binary.size()),
                          t.degree.data(), t.op.data(), t.feature.data(), t.constant.data(), t.val.data(), t.size(), prog,
                          err);
}

template <typename T>
void random_trees(const char* name, uint64_t seed, int n_trees, bool smooth) {
  Ops ops;
  if (smooth) {
    ops.unary = {SR_U_NEG, SR_U_SQUARE, SR_U_COS, SR_U_SIN, SR_U_TANH, SR_U_ATAN};
    ops.binary = {SR_B_ADD, SR_B_SUB, SR_B_MUL};
  } else {
    for (uint32_t u = 1; u < SR_U_COUNT; ++u) ops.unary.push_back(u);
    for (uint32_t b = 1; b < SR_B_COUNT; ++b) ops.binary.push_back(b);
  }
  Rng r{seed};
  int accepted = 0, rejected = 0, derivs = 0;
  for (int k = 0; k < n_trees; ++k) {
    Tree t;
    const int size = 1 + r.below(k % 8 >= 6 ? 100 : 31);
    gen(r, ops, t, size, k % 2 == 0, k % 8 == 6);
    int i = 0;
    bool leaf = false, is_const = false;
    const int need = live(t, i, &leaf, &is_const);
    SrLossProg<T> prog;
    std::string err;
    const int rc = compile<T>(t, ops, &prog, &err);
    if (need > SR_LX_MAX_LIVE) {
      CHECK(rc != 0 && !err.empty(), "%s tree %d: needs %d live values but was accepted", name, k, need);
      ++rejected;
      continue;
    }
    if (rc != 0) {  // (only the instruction limit is left: large trees)
      CHECK(!err.empty() && size > SR_LX_MAX_INS, "%s tree %d (%d nodes, %d live) refused: %s", name, k, size, need, err.c_str());
      ++rejected;
      continue;
    }
    ++accepted;
    CHECK(prog.max_live == need, "%s tree %d: max_live %d, expected %d", name, k, prog.max_live, need);
    CHECK(prog.n >= 1 && prog.n <= SR_LX_MAX_INS, "%s tree %d: %d instructions", name, k, prog.n);
    int depth = 0, top = 0;
    for (int q = 0; q < prog.n; ++q) {
      const uint32_t kind = prog.ins[q].op & 0xffu;
      if (kind == SR_LX_PUSH || kind == SR_LX_BIN_LL) ++depth;
      if (kind == SR_LX_BIN_SS || kind == SR_LX_BIN_SW) --depth;
      CHECK(depth >= 1, "%s tree %d: stack underflow at %d", name, k, q);
      top = depth > top ? depth : top;
    }
    CHECK(depth == 1 && top <= prog.max_live && top <= SR_LX_MAX_LIVE, "%s tree %d: depth %d at the end, %d at most, %d declared",
          name, k, depth, top, prog.max_live);
    for (int e = 0; e < 8; ++e) {
      const T p = T(2.0 * r.unit() - 1.0), y = T(2.0 * r.unit() - 1.0), w = T(0.5 + r.unit());
      T v = T(0), d = T(0);
      sr_lx_host_eval<T>(prog, 1, &p, &y, &w, &v, nullptr);
      int j = 0;
      bool c = false;
      const T ref = eval<T>(t, ops, j, p, y, w, &c);
      CHECK(same_bits(v, ref), "%s tree %d: value %.17g, direct evaluation %.17g", name, k, double(v), double(ref));
      T v2 = T(0);
      sr_lx_host_eval<T>(prog, 1, &p, &y, &w, &v2, &d);
      CHECK(same_bits(v, v2), "%s tree %d: the derivative pass's value differs", name, k);
      if (smooth && sizeof(T) == 8) {
        // central differences at h and h / 2: their difference is 3/4 of the first one's truncation error
        // (h^2 f''' / 6), so twice it bounds the second one's; the rounding error of a difference quotient
        // is at most 2 eps max|f| / (2 h) per evaluation pair, taken four times over
        auto at = [&](double q) {
          int j1 = 0;
          return double(eval<T>(t, ops, j1, T(q), y, w, &c));
        };
        const double h = 1e-4;
        const double f1p = at(double(p) + h), f1m = at(double(p) - h), f2p = at(double(p) + h / 2), f2m = at(double(p) - h / 2);
        const double fmax = std::fmax(std::fmax(std::fabs(f1p), std::fabs(f1m)), std::fmax(std::fabs(f2p), std::fabs(f2m)));
        if (!(fmax < 1e6)) continue;
        const double fd1 = (f1p - f1m) / (2.0 * h), fd2 = (f2p - f2m) / h;
        const double tol = 2.0 * std::fabs(fd1 - fd2) + 4.0 * 2.3e-16 * fmax / (h / 2) + 1e-12;
        CHECK(std::fabs(double(d) - fd2) <= tol, "%s tree %d: derivative %.12g, central difference %.12g (bound %.3g)", name, k,
              double(d), fd2, tol);
        ++derivs;
      }
    }
  }
  std::printf("%s: %d accepted, %d rejected, %d derivative checks\n", name, accepted, rejected, derivs);
  CHECK(accepted > n_trees / 2, "%s: too few accepted trees", name);
}

template <typename T>
void fixed_cases() {
  Ops ops;
  ops.unary = {SR_U_NEG, SR_U_ABS};
  ops.binary = {SR_B_ADD, SR_B_SUB};
  SrLossProg<T> prog;
  std::string err;
  {  // a 31-node right-deep chain: p + (t + (p + ...)): accepted, one live value
    Tree t;
    for (int i = 0; i < 15; ++i) {
      t.node(2, 1, 0, false, 0.0);
      t.node(0, 0, 1 + i % 2, false, 0.0);
    }
    t.node(0, 0, 1, false, 0.0);
    CHECK(t.size() == 31 && compile<T>(t, ops, &prog, &err) == 0 && prog.max_live <= 2, "right-deep chain refused: %s", err.c_str());
  }
  {  // the smallest tree needing 5 live values: a perfect binary tree over 16 unary(leaf) subtrees
    Tree t;
    auto rec = [&](auto&& self, int level) -> void {
      if (level == 0) {
        t.node(1, 2, 0, false, 0.0);
        t.node(0, 0, 1, false, 0.0);
        return;
      }
      t.node(2, 1, 0, false, 0.0);
      self(self, level - 1);
      self(self, level - 1);
    };
    rec(rec, 4);
    err.clear();
    CHECK(compile<T>(t, ops, &prog, &err) != 0 && err.find("live values") != std::string::npos, "5 live values accepted (%s)", err.c_str());
    Tree t4;
    std::swap(t, t4);
    rec(rec, 3);  // 4 live values: accepted
    CHECK(compile<T>(t, ops, &prog, &err) == 0 && prog.max_live == 4, "4 live values refused: %s", err.c_str());
  }
  {  // 200 nodes
    Tree t;
    for (int i = 0; i < 199; ++i) t.node(1, 1, 0, false, 0.0);
    t.node(0, 0, 1, false, 0.0);
    err.clear();
    CHECK(compile<T>(t, ops, &prog, &err) != 0 && !err.empty(), "200-node tree accepted");
  }
  auto refused = [&](const Tree& t, const char* what) {
    err.clear();
    CHECK(compile<T>(t, ops, &prog, &err) != 0 && !err.empty(), "%s accepted", what);
  };
  {
    Tree t;
    t.node(2, 1, 0, false, 0.0);
    t.node(0, 0, 1, false, 0.0);
    refused(t, "a truncated tree");
    t.node(0, 0, 2, false, 0.0);
    t.node(0, 0, 2, false, 0.0);
    refused(t, "a tree with a trailing node");
  }
  {
    Tree t;
    t.node(0, 0, 4, false, 0.0);
    refused(t, "feature 4");
    Tree u;
    u.node(0, 0, 0, false, 0.0);
    refused(u, "feature 0");
    Tree v;
    v.node(1, 3, 0, false, 0.0);
    v.node(0, 0, 1, false, 0.0);
    refused(v, "a unary operator index past the list");
    Tree x;
    x.node(3, 1, 0, false, 0.0);
    refused(x, "degree 3");
    Tree e;
    refused(e, "an empty tree");
  }
  {  // constants are rounded to T, folded in T: (0.1 + 0.2) - p
    Tree t;
    t.node(2, 2, 0, false, 0.0);
    t.node(2, 1, 0, false, 0.0);
    t.node(0, 0, 0, true, 0.1);
    t.node(0, 0, 0, true, 0.2);
    t.node(0, 0, 1, false, 0.0);
    err.clear();  // (the constant becomes the subtraction's leaf operand: one instruction)
    CHECK(compile<T>(t, ops, &prog, &err) == 0 && prog.n == 1, "constant folding: %d instructions (%s)", prog.n, err.c_str());
    const T p = T(0.25), y = T(0);
    T v = T(0);
    sr_lx_host_eval<T>(prog, 1, &p, &y, nullptr, &v, nullptr);
    CHECK(same_bits(v, T((T(0.1) + T(0.2)) - p)), "constant folding is not in T");
  }
}

}  // namespace

int main() {
  random_trees<float>("float, whole catalog", 11, 400, false);
  random_trees<double>("double, whole catalog", 12, 400, false);
  random_trees<float>("float, smooth", 13, 300, true);
  random_trees<double>("double, smooth", 14, 300, true);
  fixed_cases<float>();
  fixed_cases<double>();
  if (g_fail) {
    std::fprintf(stderr, "loss_expr_check: %d failures\n", g_fail);
    return 1;
  }
  std::printf("loss_expr_check: ok\n");
  return 0;
}
