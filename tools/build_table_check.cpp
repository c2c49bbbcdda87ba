// build_table_check.cpp — stand-alone host check of the tile kernels' build table (csrc/sr_builds.h; no GPU,
// no HIP, no Python).
//
// Build and run through `make -C symbolicregression.jl_amd build-check`, which compiles this file with
// -fsanitize=address,undefined.  Four checks:
//   1. every row's key is unique, and the Makefile's UNITS list names exactly the header's units;
//   2. sr_resolve_build over the whole request domain equals the recorded rule.  The record was produced once
//      from the four hand-written launchers this table replaced (one per family: nested ifs, each ending in
//      a hand-typed sr_launch_tile<...>), with sr_launch_tile stubbed to return its template arguments: per
//      family the count of accepted requests, and an FNV-1a digest of the ordered listing.
//      profiles/build_table_resolve.txt states the recorded rule (the accepted requests, merged into products
//      of axis sets); `build_table_check --dump` prints this build's full listing, so a mismatch can be diffed
//      against the dump of a commit that passes;
//   3. every build the rule can name is in the table (and the rows no request reaches are printed);
//   4. every request the host can form (sr_launch_shape over the knobs, crossed with type, mode, tier, view,
//      family and the probe's gathered variant) names a build of the table, or is one of the refusals
//      listed in host_refusal below; and the build has the rows per lane and waves the host planned its grid
//      with, or the request is one of the divergences listed in host_divergence.
// Exit status 0 and "build_table_check: ok" on success.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "../symbolicregression.jl_amd/csrc/sr_builds.h"

namespace {

int g_failed = 0;
#define CHECK(cond)                                                                      \
  do {                                                                                   \
    if (!(cond)) {                                                                       \
      std::fprintf(stderr, "build_table_check: %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      if (++g_failed > 20) std::exit(1);                                                 \
    }                                                                                    \
  } while (0)

// the recorded rule (see above): accepted requests per family, and the listing's digest
constexpr int kAccepted[4] = {1934, 124, 128, 32};
constexpr uint64_t kListingDigest = 0x961d873fdecacee8ull;
constexpr int kOtherLoss = SR_LOSS_HUBER;  // "one other catalog loss"

// compile-time findings: the rule's answers for the default calls are rows of the table
static_assert(sr_build_exists(sr_resolve_build({4, SR_MODE_LOSS, false, SR_TIER_BASIC, 8, 4, false, SR_LOSS_L2, SR_FAMILY_PLAIN})), "");
static_assert(sr_build_exists(sr_resolve_build({4, SR_MODE_LOSS, false, SR_TIER_BASIC, 16, 4, true, SR_LOSS_L2, SR_FAMILY_CAND})), "");
static_assert(!sr_build_exists(SrBuildKey{}), "");

void check_table() {
  std::set<uint32_t> seen;
  for (const SrBuildKey k : kSrBuildKeys) {
    CHECK(k.ok());
    CHECK(seen.insert(k.v).second);  // no duplicate keys
    // the packing keeps every field
    CHECK(sr_build_key(k.elem_size(), k.R(), k.mode(), k.gather(), k.tier(), k.W(), k.lk(), k.vstk()) == k);
  }
#define SR_UNIT_NAME(unit, _) #unit " "
  std::string units = SR_UNITS(SR_UNIT_NAME, _);
#undef SR_UNIT_NAME
  units.pop_back();
#ifdef SR_MAKE_UNITS
  if (units != SR_MAKE_UNITS) std::fprintf(stderr, "header units: %s\nMakefile UNITS: %s\n", units.c_str(), SR_MAKE_UNITS);
  CHECK(units == SR_MAKE_UNITS);
#endif
}

// The whole request domain in the record's order; returns the accepted keys.
std::set<uint32_t> check_resolve(bool dump) {
  const int Rs[] = {1, 2, 4, 8, 16, 32, 3}, Ws[] = {1, 4, 8}, Ls[] = {SR_LOSS_L1, SR_LOSS_L2, kOtherLoss, SR_LOSS_EXPR};
  const int modes[] = {SR_MODE_LOSS, SR_MODE_PRED, SR_MODE_EXACT, SR_MODE_FOLD};
  uint64_t h = 0xcbf29ce484222325ull;
  int accepted[4] = {0, 0, 0, 0};
  std::set<uint32_t> keys;
  char line[128];
  for (int fam = 0; fam < 4; ++fam)
    for (int es : {4, 8})
      for (int mode : modes)
        for (int gather = 0; gather < 2; ++gather)
          for (int tier : {int(SR_TIER_BASIC), int(SR_TIER_FULL)})
            for (int R : Rs)
              for (int W : Ws)
                for (int vstk = 0; vstk < 2; ++vstk)
                  for (int lk : Ls) {
                    const SrBuildKey k = sr_resolve_build({es, mode, gather != 0, tier, R, W, vstk != 0, lk, SrBuildFamily(fam)});
                    int n = std::snprintf(line, sizeof line, "%d %d %d %d %d %d %d %d %d :", fam, es, mode, gather, tier, R, W, vstk, lk);
                    if (k.ok()) {
                      n += std::snprintf(line + n, sizeof line - size_t(n), " %d %d %d %d %d %d %d %d\n", k.elem_size(), k.R(), k.mode(),
                                         int(k.gather()), k.tier(), k.W(), k.lk(), int(k.vstk()));
                      ++accepted[fam];
                      keys.insert(k.v);
                      if (!sr_build_exists(k)) std::fprintf(stderr, "resolved, but no row: %s", line);
                      CHECK(sr_build_exists(k));
                    } else {
                      n += std::snprintf(line + n, sizeof line - size_t(n), " -\n");
                    }
                    if (dump) std::fputs(line, stdout);
                    for (int i = 0; i < n; ++i) h = (h ^ uint8_t(line[i])) * 0x100000001b3ull;
                  }
  for (int fam = 0; fam < 4; ++fam) {
    if (accepted[fam] != kAccepted[fam]) std::fprintf(stderr, "family %d: %d accepted, recorded %d\n", fam, accepted[fam], kAccepted[fam]);
    CHECK(accepted[fam] == kAccepted[fam]);
  }
  if (h != kListingDigest) std::fprintf(stderr, "listing digest %016llx, recorded %016llx\n", (unsigned long long)h, (unsigned long long)kListingDigest);
  CHECK(h == kListingDigest);
  return keys;
}

// A request the host forms and the rule refuses.  Each is a call that fails at this launch today
// (hipErrorInvalidValue from the launcher, reported as SR_ERR_HIP); nothing refuses it earlier:
//   - SR_AMD_WAVES=8 with the in-order fold's FOLD pass (path 2): the classic BASIC FOLD build has 4 waves only.
bool host_refusal(const SrBuildRequest& q) {
  return q.family == SR_FAMILY_PLAIN && q.elem_size == 4 && q.mode == SR_MODE_FOLD && q.tier == SR_TIER_BASIC && !q.vstk &&
         q.R == 8 && q.waves == 8;
}

// A request the host forms whose build has other rows per lane or waves than the host planned with
// ("Known divergences"); the candidate launch states its shape itself.
//   - the dead-tree probe of a full-view f32 BASIC call under "rows_per_lane" 4 / 16: the gathered build, 8 rows
//     per lane (only hints come out of the probe; its n_rows bounds what it reads);
//   - SR_AMD_WAVES=8: only the classic full-view L2 loss launch has an 8-wave build; the probe and every other loss
//     run 4 waves (the register-stack builds ignore waves) under a GridSpec sized for 8.
bool host_divergence(const SrBuildRequest& q, SrBuildKey k) {
  const bool f32_basic = q.elem_size == 4 && q.tier == SR_TIER_BASIC && q.family == SR_FAMILY_PLAIN;
  if (f32_basic && q.mode == SR_MODE_LOSS && q.gather && !q.vstk && (q.R == 4 || q.R == 16) && k.R() == 8 && k.W() == 4) return true;
  // (the register-stack FOLD launch of such a call too; its classic FOLD launch is host_refusal's)
  if (f32_basic && (q.mode == SR_MODE_LOSS || (q.mode == SR_MODE_FOLD && q.vstk)) && q.waves == 8 && k.W() == 4 && k.R() == q.R) return true;
  return false;
}

int g_host_requests = 0, g_host_refused = 0;
void host_request(const SrBuildRequest& q) {
  ++g_host_requests;
  const SrBuildKey k = sr_resolve_build(q);
  if (!k.ok()) {
    ++g_host_refused;
    if (!host_refusal(q))
      std::fprintf(stderr, "host request refused: es %d mode %d gather %d tier %d R %d W %d vstk %d lk %d family %d\n", q.elem_size,
                   q.mode, int(q.gather), q.tier, q.R, q.waves, int(q.vstk), q.loss_kind, int(q.family));
    CHECK(host_refusal(q));
    return;
  }
  CHECK(sr_build_exists(k));
  // the host sized its grid and LDS with the request's rows per lane and waves: the build's are the same,
  // but for the divergences that are listed
  if (q.family == SR_FAMILY_CAND || host_divergence(q, k)) return;
  if (k.R() != q.R || k.W() != q.waves)
    std::fprintf(stderr, "planned R %d W %d, build R %d W %d: es %d mode %d gather %d tier %d vstk %d lk %d family %d\n", q.R, q.waves, k.R(),
                 k.W(), q.elem_size, q.mode, int(q.gather), q.tier, int(q.vstk), q.loss_kind, int(q.family));
  CHECK(k.R() == q.R && k.W() == q.waves);
}

// What sr_capi.cpp launches for one call: choose_kernels' shape, then launch_region (classic and
// register-stack regions, the candidate launch), launch_probe, fold_steps and run_exact.
void check_host() {
  const int knob[] = {-8, -4, -1, 0, 1, 2, 3, 4, 5, 8, 12, 16, 24, 32, 33, 64};  // rows_per_lane / vstk_rows / waves: stored as given
  const int losses[] = {SR_LOSS_L2, SR_LOSS_L1, kOtherLoss, SR_LOSS_EXPR};
  for (int es : {4, 8})
    for (int mode : {int(SR_MODE_LOSS), int(SR_MODE_PRED)})  // (a call's mode; EXACT and FOLD launches follow a LOSS call)
      for (int tier : {int(SR_TIER_BASIC), int(SR_TIER_FULL)})
        for (int gather = 0; gather < 2; ++gather)
          for (int parametric = 0; parametric < 2; ++parametric)
            for (int lk : losses)
              for (int64_t n_eval : {int64_t(1000), int64_t(1) << 17})
                for (int rows : knob)
                  for (int waves : knob)
                    for (int vrows : knob) {
                      const bool lexpr = lk == SR_LOSS_EXPR;
                      if (lexpr && (parametric || mode != SR_MODE_LOSS)) continue;  // (plain LOSS calls only: kLossExprOnly)
                      const SrBuildFamily call = parametric ? SR_FAMILY_PARAM : (lexpr ? SR_FAMILY_LOSSX : SR_FAMILY_PLAIN);
                      const SrLaunchShape sh = sr_launch_shape(es, mode, tier, gather != 0, call, n_eval, rows, waves, vrows);
                      SrBuildRequest q{es, mode, gather != 0, tier, sh.R, sh.W, false, lk, parametric ? SR_FAMILY_PARAM : SR_FAMILY_PLAIN};
                      host_request(q);  // the classic region
                      if (mode != SR_MODE_LOSS) continue;
                      SrBuildRequest probe = q;  // the dead-tree probe: gather || stress_probe
                      probe.gather = true;
                      host_request(probe);
                      SrBuildRequest qv = q;  // the register-stack region
                      qv.R = sh.Rv;
                      qv.vstk = true;
                      if (sh.Rv > 0) host_request(qv);
                      // the in-order fold's FOLD pass (sr_fold_plan path 2: Float32, never an expression loss)
                      const bool fold_builds = tier == SR_TIER_BASIC ? (sh.R == 8 && (sh.Rv == 0 || sh.Rv == 16)) : sh.R == 4;
                      if (es == 4 && !lexpr && fold_builds) {
                        SrBuildRequest f = q;
                        f.mode = SR_MODE_FOLD;
                        host_request(f);
                        f.R = sh.Rv;
                        f.vstk = true;
                        if (sh.Rv > 0) host_request(f);
                        // the candidate launch: plain, BASIC, full view, the register-stack region at 16 rows, 4 waves
                        if (!parametric && tier == SR_TIER_BASIC && !gather && sh.Rv == 16 && sh.W == 4) {
                          SrBuildRequest c = qv;
                          c.family = SR_FAMILY_CAND;
                          host_request(c);
                        }
                      }
                      // the exact-sum pass (run_exact): FULL-tier rows per lane, 1 or 4 waves (parametric: 4, the FULL-tier build)
                      const int Rx = es == 4 ? sr_rows_per_lane<float>(SR_MODE_EXACT, SR_TIER_FULL, 0) : sr_rows_per_lane<double>(SR_MODE_EXACT, SR_TIER_FULL, 0);
                      for (int Wx : {1, 4})
                        for (int etier : {int(SR_TIER_BASIC), int(SR_TIER_FULL)}) {
                          if (parametric && (Wx != 4 || etier != SR_TIER_FULL)) continue;
                          host_request({es, SR_MODE_EXACT, gather != 0, etier, Rx, Wx, false, SR_LOSS_L2,
                                        parametric ? SR_FAMILY_PARAM : SR_FAMILY_PLAIN});
                        }
                    }
}

}  // namespace

int main(int argc, char** argv) {
  const bool dump = argc > 1 && std::strcmp(argv[1], "--dump") == 0;
  check_table();
  const std::set<uint32_t> reached = check_resolve(dump);
  check_host();
  if (dump) return g_failed ? 1 : 0;
  int unreached = 0;
  for (const SrBuildKey k : kSrBuildKeys)
    if (!reached.count(k.v)) {
      ++unreached;
      std::printf("no request resolves to: es %d R %d mode %d gather %d tier %d W %d lk %d vstk %d\n", k.elem_size(), k.R(), k.mode(),
                  int(k.gather()), k.tier(), k.W(), k.lk(), int(k.vstk()));
    }
  CHECK(unreached == 0);
  std::printf("build_table_check: %d builds, %zu reached by the rule; %d host requests, %d of them refusals that are listed\n",
              kSrBuildCount, reached.size(), g_host_requests, g_host_refused);
  if (g_failed) {
    std::fprintf(stderr, "build_table_check: %d check(s) failed\n", g_failed);
    return 1;
  }
  std::printf("build_table_check: ok\n");
  return 0;
}
