// sr_builds.h — the builds of sr_tile_kernel, stated once: ONE table with a row per build, grouped by the
// translation unit that compiles it, and the rule that maps a launch's request onto a row.  The
// instantiations (sr_inst.hip, once per unit), the launcher's pointer table (sr_aux.hip), the host's
// requests (sr_capi.cpp) and the host check (tools/build_table_check.cpp, `make build-check`) all come from
// here.  Host-only like sr_plan.h: no HIP.
#pragma once
#include <stdint.h>

#include "sr_ops.h"   // SrLossKind
#include "sr_plan.h"  // SR_MODE_*, SR_TIER_*

// ---------------------------------------------------------------- the table
// A row is X(T, R, MODE, GATHER, TIER, W, LK, VSTK), the template arguments of sr_tile_kernel / sr_launch_tile:
// element type, rows per lane, mode, row view, tier (| SR_TIER_PARAM: the build for parametric calls, |
// SR_TIER_CAND: the candidate-composing loss build), waves per workgroup, the elementwise loss the build
// folds in (SR_LK_ANY: the generic build, loss chosen at run time), operand stack in VGPRs.
// D(T) rows are the sr_launch_derived instantiations that ride in two of the units.
// The units exist so that the kernels compile in parallel (profiles/r04_compile_scaling.txt); the Makefile's
// UNITS list names them again and build-check compares the two.
constexpr int SR_LK_ANY = -1;

// BASIC-tier loss builds come one per elementwise loss (the loss code folds away): L2, L1, generic
#define SR_ROWS_BASIC_LOSS(X, T, R, GATHER, VSTK)                          \
  X(T, R, SR_MODE_LOSS, GATHER, SR_TIER_BASIC, 4, SR_LOSS_L2, VSTK) \
  X(T, R, SR_MODE_LOSS, GATHER, SR_TIER_BASIC, 4, SR_LOSS_L1, VSTK) \
  X(T, R, SR_MODE_LOSS, GATHER, SR_TIER_BASIC, 4, SR_LK_ANY, VSTK)

// f32 loss over the full dataset: BASIC tier at 8 rows/lane (4 rows/lane and the 8-wave L2 build for
// tuning), FULL tier at 4 rows/lane
#define SR_BUILDS_f32_loss(X, D)                                          \
  SR_ROWS_BASIC_LOSS(X, float, 8, false, false)                           \
  X(float, 4, SR_MODE_LOSS, false, SR_TIER_BASIC, 4, SR_LK_ANY, false)    \
  X(float, 4, SR_MODE_LOSS, false, SR_TIER_FULL, 4, SR_LK_ANY, false)     \
  X(float, 8, SR_MODE_LOSS, false, SR_TIER_BASIC, 8, SR_LOSS_L2, false)
// f32 BASIC loss at 16 rows/lane: twice the rows per dispatched instruction of the 8-rows/lane kernels, for
// large views
#define SR_BUILDS_f32_r16(X, D) SR_ROWS_BASIC_LOSS(X, float, 16, false, false)
// f32 register-stack loss (BASIC tier, operand stack in VGPRs): 8, 16 and 32 rows per lane
#define SR_BUILDS_f32_vstk(X, D)               \
  SR_ROWS_BASIC_LOSS(X, float, 8, false, true)  \
  SR_ROWS_BASIC_LOSS(X, float, 16, false, true) \
  SR_ROWS_BASIC_LOSS(X, float, 32, false, true)
// f32 loss over a row view (SubDataset / minibatch)
#define SR_BUILDS_f32_gather(X, D)             \
  SR_ROWS_BASIC_LOSS(X, float, 8, true, false) \
  X(float, 4, SR_MODE_LOSS, true, SR_TIER_FULL, 4, SR_LK_ANY, false)
// f32 prediction and exact-check (Julia-order range sum) kernels (FULL tier, 4 rows/lane); EXACT with 1 or 4
// waves per workgroup, sharing the staged rows
#define SR_BUILDS_f32_aux(X, D)                                        \
  X(float, 4, SR_MODE_PRED, false, SR_TIER_FULL, 4, SR_LK_ANY, false)  \
  X(float, 4, SR_MODE_PRED, true, SR_TIER_FULL, 4, SR_LK_ANY, false)   \
  X(float, 4, SR_MODE_EXACT, false, SR_TIER_FULL, 1, SR_LK_ANY, false) \
  X(float, 4, SR_MODE_EXACT, true, SR_TIER_FULL, 1, SR_LK_ANY, false)  \
  X(float, 4, SR_MODE_EXACT, false, SR_TIER_FULL, 4, SR_LK_ANY, false) \
  X(float, 4, SR_MODE_EXACT, true, SR_TIER_FULL, 4, SR_LK_ANY, false)  \
  D(float)
// f32 FOLD mode (the complete trees' loss programs again, composing the reference's in-order loss fold per
// row tile, sr_fold_dev.h): the register-stack builds of the large-call path
#define SR_BUILDS_f32_fold(X, D)                                       \
  X(float, 16, SR_MODE_FOLD, false, SR_TIER_BASIC, 4, SR_LOSS_L2, true) \
  X(float, 16, SR_MODE_FOLD, false, SR_TIER_BASIC, 4, SR_LK_ANY, true)
// f32 FOLD mode, the classic LDS-stack builds: full view and gathered views, BASIC tier at 8 rows per lane,
// FULL tier at 4
#define SR_BUILDS_f32_fold2(X, D)                                       \
  X(float, 8, SR_MODE_FOLD, false, SR_TIER_BASIC, 4, SR_LOSS_L2, false) \
  X(float, 8, SR_MODE_FOLD, false, SR_TIER_BASIC, 4, SR_LK_ANY, false)  \
  X(float, 8, SR_MODE_FOLD, true, SR_TIER_BASIC, 4, SR_LK_ANY, false)   \
  X(float, 4, SR_MODE_FOLD, false, SR_TIER_FULL, 4, SR_LK_ANY, false)   \
  X(float, 4, SR_MODE_FOLD, true, SR_TIER_FULL, 4, SR_LK_ANY, false)
// f32 register-stack loss builds that also compose each row block's in-order fold steps under candidate
// binades (SR_TIER_CAND): the loss launch of a large plain call under the in-order fold, 16 rows per lane
#define SR_BUILDS_f32_cand(X, D)                                                       \
  X(float, 16, SR_MODE_LOSS, false, SR_TIER_BASIC | SR_TIER_CAND, 4, SR_LOSS_L2, true) \
  X(float, 16, SR_MODE_LOSS, false, SR_TIER_BASIC | SR_TIER_CAND, 4, SR_LK_ANY, true)
// f64 loss over the full dataset: BASIC tier at 4 rows/lane, FULL tier at 2
#define SR_BUILDS_f64_loss(X, D)                \
  SR_ROWS_BASIC_LOSS(X, double, 4, false, false) \
  X(double, 2, SR_MODE_LOSS, false, SR_TIER_FULL, 4, SR_LK_ANY, false)
// f64 register-stack loss: 8 rows per lane is twice the classic f64 build's; and a 4-row build
// (SR_AMD_VSTK_ROWS=-4)
#define SR_BUILDS_f64_vstk(X, D)               \
  SR_ROWS_BASIC_LOSS(X, double, 8, false, true) \
  SR_ROWS_BASIC_LOSS(X, double, 4, false, true)
// f64 loss over a row view (SubDataset / minibatch)
#define SR_BUILDS_f64_gather(X, D)              \
  SR_ROWS_BASIC_LOSS(X, double, 4, true, false) \
  X(double, 2, SR_MODE_LOSS, true, SR_TIER_FULL, 4, SR_LK_ANY, false)
// f64 prediction and exact-check kernels (FULL tier, 2 rows/lane)
#define SR_BUILDS_f64_aux(X, D)                                         \
  X(double, 2, SR_MODE_PRED, false, SR_TIER_FULL, 4, SR_LK_ANY, false)  \
  X(double, 2, SR_MODE_PRED, true, SR_TIER_FULL, 4, SR_LK_ANY, false)   \
  X(double, 2, SR_MODE_EXACT, false, SR_TIER_FULL, 1, SR_LK_ANY, false) \
  X(double, 2, SR_MODE_EXACT, true, SR_TIER_FULL, 1, SR_LK_ANY, false)  \
  X(double, 2, SR_MODE_EXACT, false, SR_TIER_FULL, 4, SR_LK_ANY, false) \
  X(double, 2, SR_MODE_EXACT, true, SR_TIER_FULL, 4, SR_LK_ANY, false)  \
  D(double)
// BASIC EXACT without the FULL tier's 38 further operators in the dispatch (f32: 121 -> 84 VGPRs)
#define SR_BUILDS_exact_basic(X, D)                                      \
  X(float, 4, SR_MODE_EXACT, false, SR_TIER_BASIC, 1, SR_LK_ANY, false)  \
  X(float, 4, SR_MODE_EXACT, true, SR_TIER_BASIC, 1, SR_LK_ANY, false)   \
  X(float, 4, SR_MODE_EXACT, false, SR_TIER_BASIC, 4, SR_LK_ANY, false)  \
  X(float, 4, SR_MODE_EXACT, true, SR_TIER_BASIC, 4, SR_LK_ANY, false)   \
  X(double, 2, SR_MODE_EXACT, false, SR_TIER_BASIC, 1, SR_LK_ANY, false) \
  X(double, 2, SR_MODE_EXACT, true, SR_TIER_BASIC, 1, SR_LK_ANY, false)  \
  X(double, 2, SR_MODE_EXACT, false, SR_TIER_BASIC, 4, SR_LK_ANY, false) \
  X(double, 2, SR_MODE_EXACT, true, SR_TIER_BASIC, 4, SR_LK_ANY, false)
// f32 loss for parametric calls (LOAD_PARAM / P operands): BASIC tier at 8 rows/lane, the L2 and the
// generic-loss build over the full dataset, the generic one over a row view
#define SR_BUILDS_f32_param_loss(X, D)                                                   \
  X(float, 8, SR_MODE_LOSS, false, SR_TIER_BASIC | SR_TIER_PARAM, 4, SR_LOSS_L2, false) \
  X(float, 8, SR_MODE_LOSS, false, SR_TIER_BASIC | SR_TIER_PARAM, 4, SR_LK_ANY, false)  \
  X(float, 8, SR_MODE_LOSS, true, SR_TIER_BASIC | SR_TIER_PARAM, 4, SR_LK_ANY, false)
// f32 register-stack loss for parametric calls: BASIC tier at 16 rows/lane (L2 and generic loss)
#define SR_BUILDS_f32_param_vstk(X, D)                                                   \
  X(float, 16, SR_MODE_LOSS, false, SR_TIER_BASIC | SR_TIER_PARAM, 4, SR_LOSS_L2, true) \
  X(float, 16, SR_MODE_LOSS, false, SR_TIER_BASIC | SR_TIER_PARAM, 4, SR_LK_ANY, true)
// f32 FULL-tier loss and prediction for parametric calls (4 rows/lane)
#define SR_BUILDS_f32_param_full(X, D)                                                \
  X(float, 4, SR_MODE_LOSS, false, SR_TIER_FULL | SR_TIER_PARAM, 4, SR_LK_ANY, false) \
  X(float, 4, SR_MODE_LOSS, true, SR_TIER_FULL | SR_TIER_PARAM, 4, SR_LK_ANY, false)  \
  X(float, 4, SR_MODE_PRED, false, SR_TIER_FULL | SR_TIER_PARAM, 4, SR_LK_ANY, false) \
  X(float, 4, SR_MODE_PRED, true, SR_TIER_FULL | SR_TIER_PARAM, 4, SR_LK_ANY, false)
// f32 exact-check (4 waves, FULL-tier build for every operator set) and FULL-tier FOLD for parametric calls
#define SR_BUILDS_f32_param_aux(X, D)                                                  \
  X(float, 4, SR_MODE_EXACT, false, SR_TIER_FULL | SR_TIER_PARAM, 4, SR_LK_ANY, false) \
  X(float, 4, SR_MODE_EXACT, true, SR_TIER_FULL | SR_TIER_PARAM, 4, SR_LK_ANY, false)  \
  X(float, 4, SR_MODE_FOLD, false, SR_TIER_FULL | SR_TIER_PARAM, 4, SR_LK_ANY, false)  \
  X(float, 4, SR_MODE_FOLD, true, SR_TIER_FULL | SR_TIER_PARAM, 4, SR_LK_ANY, false)
// f32 BASIC-tier FOLD for parametric calls (generic loss): the shapes of their loss launches
#define SR_BUILDS_f32_param_fold(X, D)                                                 \
  X(float, 16, SR_MODE_FOLD, false, SR_TIER_BASIC | SR_TIER_PARAM, 4, SR_LK_ANY, true) \
  X(float, 8, SR_MODE_FOLD, false, SR_TIER_BASIC | SR_TIER_PARAM, 4, SR_LK_ANY, false) \
  X(float, 8, SR_MODE_FOLD, true, SR_TIER_BASIC | SR_TIER_PARAM, 4, SR_LK_ANY, false)
// f64 BASIC-tier loss for parametric calls: 4 rows/lane (L2 / generic over the full dataset, generic over a
// row view) and the 8-rows/lane register-stack build
#define SR_BUILDS_f64_param_loss(X, D)                                                    \
  X(double, 4, SR_MODE_LOSS, false, SR_TIER_BASIC | SR_TIER_PARAM, 4, SR_LOSS_L2, false) \
  X(double, 4, SR_MODE_LOSS, false, SR_TIER_BASIC | SR_TIER_PARAM, 4, SR_LK_ANY, false)  \
  X(double, 4, SR_MODE_LOSS, true, SR_TIER_BASIC | SR_TIER_PARAM, 4, SR_LK_ANY, false)   \
  X(double, 8, SR_MODE_LOSS, false, SR_TIER_BASIC | SR_TIER_PARAM, 4, SR_LOSS_L2, true)  \
  X(double, 8, SR_MODE_LOSS, false, SR_TIER_BASIC | SR_TIER_PARAM, 4, SR_LK_ANY, true)
// f64 FULL-tier loss and prediction for parametric calls (2 rows/lane)
#define SR_BUILDS_f64_param_full(X, D)                                                 \
  X(double, 2, SR_MODE_LOSS, false, SR_TIER_FULL | SR_TIER_PARAM, 4, SR_LK_ANY, false) \
  X(double, 2, SR_MODE_LOSS, true, SR_TIER_FULL | SR_TIER_PARAM, 4, SR_LK_ANY, false)  \
  X(double, 2, SR_MODE_PRED, false, SR_TIER_FULL | SR_TIER_PARAM, 4, SR_LK_ANY, false) \
  X(double, 2, SR_MODE_PRED, true, SR_TIER_FULL | SR_TIER_PARAM, 4, SR_LK_ANY, false)
// f64 exact-check for parametric calls (4 waves, FULL-tier build for every operator set)
#define SR_BUILDS_f64_param_aux(X, D)                                                   \
  X(double, 2, SR_MODE_EXACT, false, SR_TIER_FULL | SR_TIER_PARAM, 4, SR_LK_ANY, false) \
  X(double, 2, SR_MODE_EXACT, true, SR_TIER_FULL | SR_TIER_PARAM, 4, SR_LK_ANY, false)
// f32 BASIC-tier loss of expression-loss calls (SR_LOSS_EXPR, sr_loss_expr.h): 8 rows/lane, over the full
// dataset and over a row view (several views ride on the latter)
#define SR_BUILDS_f32_lossx(X, D)                                         \
  X(float, 8, SR_MODE_LOSS, false, SR_TIER_BASIC, 4, SR_LOSS_EXPR, false) \
  X(float, 8, SR_MODE_LOSS, true, SR_TIER_BASIC, 4, SR_LOSS_EXPR, false)
// f32 FULL-tier (per-node checks, every operator) loss of expression-loss calls: 4 rows/lane
#define SR_BUILDS_f32_lossx_full(X, D)                                   \
  X(float, 4, SR_MODE_LOSS, false, SR_TIER_FULL, 4, SR_LOSS_EXPR, false) \
  X(float, 4, SR_MODE_LOSS, true, SR_TIER_FULL, 4, SR_LOSS_EXPR, false)
// f64 BASIC-tier loss of expression-loss calls: 4 rows/lane
#define SR_BUILDS_f64_lossx(X, D)                                          \
  X(double, 4, SR_MODE_LOSS, false, SR_TIER_BASIC, 4, SR_LOSS_EXPR, false) \
  X(double, 4, SR_MODE_LOSS, true, SR_TIER_BASIC, 4, SR_LOSS_EXPR, false)
// f64 FULL-tier loss of expression-loss calls: 2 rows/lane
#define SR_BUILDS_f64_lossx_full(X, D)                                    \
  X(double, 2, SR_MODE_LOSS, false, SR_TIER_FULL, 4, SR_LOSS_EXPR, false) \
  X(double, 2, SR_MODE_LOSS, true, SR_TIER_FULL, 4, SR_LOSS_EXPR, false)

// every unit, U(unit, arg) each
#define SR_UNITS(U, A)                                                                                        \
  U(f32_loss, A) U(f32_r16, A) U(f32_vstk, A) U(f32_gather, A) U(f32_aux, A) U(f32_fold, A) U(f32_fold2, A)   \
  U(f32_cand, A) U(f64_loss, A) U(f64_vstk, A) U(f64_gather, A) U(f64_aux, A) U(exact_basic, A)               \
  U(f32_param_loss, A) U(f32_param_vstk, A) U(f32_param_full, A) U(f32_param_aux, A) U(f32_param_fold, A)     \
  U(f64_param_loss, A) U(f64_param_full, A) U(f64_param_aux, A) U(f32_lossx, A) U(f32_lossx_full, A)          \
  U(f64_lossx, A) U(f64_lossx_full, A)
#define SR_NO_ROW(T)
#define SR_UNIT_ROWS(unit, X) SR_BUILDS_##unit(X, SR_NO_ROW)
// every build of sr_tile_kernel, X(T, R, MODE, GATHER, TIER, W, LK, VSTK) each
#define SR_ALL_BUILDS(X) SR_UNITS(SR_UNIT_ROWS, X)

// ---------------------------------------------------------------- keys
// A build's template arguments packed into one word; 0 is no build (a refused request).
struct SrBuildKey {
  uint32_t v = 0;
  constexpr bool ok() const { return v != 0; }
  constexpr int elem_size() const { return (v & 1u) ? 8 : 4; }
  constexpr int R() const { return int((v >> 1) & 63u); }
  constexpr int mode() const { return int((v >> 7) & 3u); }
  constexpr bool gather() const { return ((v >> 9) & 1u) != 0; }
  constexpr int tier() const { return int((v >> 10) & 7u); }
  constexpr int W() const { return int((v >> 13) & 15u); }
  constexpr int lk() const { return int((v >> 17) & 31u) - 1; }
  constexpr bool vstk() const { return ((v >> 22) & 1u) != 0; }
};
constexpr bool operator==(SrBuildKey a, SrBuildKey b) { return a.v == b.v; }
constexpr SrBuildKey sr_build_key(int elem_size, int R, int mode, bool gather, int tier, int W, int lk, bool vstk) {
  return SrBuildKey{(elem_size == 8 ? 1u : 0u) | uint32_t(R & 63) << 1 | uint32_t(mode & 3) << 7 | (gather ? 1u : 0u) << 9 |
                    uint32_t(tier & 7) << 10 | uint32_t(W & 15) << 13 | uint32_t((lk + 1) & 31) << 17 | (vstk ? 1u : 0u) << 22};
}
#define SR_BUILD_KEY_ROW(T, R, MODE, GATHER, TIER, W, LK, VSTK) sr_build_key(int(sizeof(T)), R, MODE, GATHER, TIER, W, LK, VSTK),
constexpr SrBuildKey kSrBuildKeys[] = {SR_ALL_BUILDS(SR_BUILD_KEY_ROW)};
constexpr int kSrBuildCount = int(sizeof(kSrBuildKeys) / sizeof(kSrBuildKeys[0]));

constexpr bool sr_build_exists(SrBuildKey k) {
  for (int i = 0; i < kSrBuildCount; ++i)
    if (kSrBuildKeys[i] == k) return k.ok();
  return false;
}

// ---------------------------------------------------------------- requests
// The kernel family of a launch.  PLAIN with loss kind SR_LOSS_EXPR in LOSS mode is LOSSX (sr_resolve_build
// routes it): no generic-loss build, whose default case is L2, ever runs an expression loss.
enum SrBuildFamily : int { SR_FAMILY_PLAIN = 0, SR_FAMILY_PARAM = 1, SR_FAMILY_CAND = 2, SR_FAMILY_LOSSX = 3 };
// What a launch asks for: what the host planned its grid and LDS with.  R: sr_rows_per_lane, or sr_vstk_rows
// with vstk (operand stack in VGPRs, programs of <= SR_VSTK_SLOTS stack slots); waves: sr_waves_per_block.
struct SrBuildRequest {
  int elem_size = 4, mode = SR_MODE_LOSS;
  bool gather = false;
  int tier = SR_TIER_BASIC, R = 0, waves = 4;
  bool vstk = false;
  int loss_kind = SR_LOSS_L2;
  SrBuildFamily family = SR_FAMILY_PLAIN;
};

// The build a request runs, or SrBuildKey{} (refused).  Where the build's R or W is not the request's, the
// step that substitutes it says so: the host sized its grid with the request's (DESIGN.md §4.8 lists these
// divergences).  Shapes outside the table are refused, never approximated by a step that is not written here.
constexpr SrBuildKey sr_resolve_build(SrBuildRequest q) {
  const bool f32 = q.elem_size == 4;
  if (!f32 && q.elem_size != 8) return {};
  const int RB = f32 ? 8 : 4;   // BASIC classic rows per lane
  const int RV = f32 ? 16 : 8;  // BASIC register-stack rows per lane of the parametric builds
  const int RF = f32 ? 4 : 2;   // FULL tier / PRED / EXACT rows per lane
  const bool l2 = q.loss_kind == SR_LOSS_L2;
  const int lk3 = (l2 || q.loss_kind == SR_LOSS_L1) ? q.loss_kind : SR_LK_ANY;  // L2, L1 or the generic build
  const int lk2 = l2 ? int(SR_LOSS_L2) : SR_LK_ANY;                              // L2 or the generic build

  // a plain launch with an expression loss: LOSS runs the expression-loss builds, FOLD has none; PRED and
  // EXACT read no loss
  if (q.family == SR_FAMILY_PLAIN && q.loss_kind == SR_LOSS_EXPR) {
    if (q.mode == SR_MODE_FOLD) return {};
    if (q.mode == SR_MODE_LOSS) q.family = SR_FAMILY_LOSSX;
  }

  if (q.family == SR_FAMILY_LOSSX) {
    // the classic kernel at its default rows per lane, 4 waves, per tier, full view or gathered; always a
    // LOSS launch (the launch takes no mode)
    if (q.loss_kind != SR_LOSS_EXPR || q.vstk || q.waves != 4) return {};
    if (q.R != (q.tier == SR_TIER_BASIC ? RB : RF)) return {};
    return sr_build_key(q.elem_size, q.R, SR_MODE_LOSS, q.gather, q.tier == SR_TIER_BASIC ? SR_TIER_BASIC : SR_TIER_FULL, 4,
                        SR_LOSS_EXPR, false);
  }

  if (q.family == SR_FAMILY_CAND) {
    // one shape: Float32, BASIC tier, full view, register stack at 16 rows per lane, 4 waves; always a LOSS
    // launch (the launch takes neither mode, view, tier nor stack); L1 runs the generic build
    if (!f32 || q.R != 16 || q.waves != 4) return {};
    return sr_build_key(4, 16, SR_MODE_LOSS, false, SR_TIER_BASIC | SR_TIER_CAND, 4, lk2, true);
  }

  if (q.family == SR_FAMILY_PARAM) {
    // a smaller set, nothing substituted but the loss: 4 waves everywhere; L1 runs the generic build
    if (q.waves != 4) return {};
    const bool basic = q.tier == SR_TIER_BASIC;
    if (basic && (q.mode == SR_MODE_LOSS || q.mode == SR_MODE_FOLD)) {
      if (q.mode == SR_MODE_FOLD && !f32) return {};  // (Float64: small calls only, from stored losses)
      // classic at RB rows per lane (full view or gathered), register stack at RV (full view)
      if (q.vstk ? (q.R != RV || q.gather) : q.R != RB) return {};
      // FOLD and the gathered loss launch: the generic-loss build only
      const int lk = (q.mode == SR_MODE_FOLD || q.gather) ? SR_LK_ANY : lk2;
      return sr_build_key(q.elem_size, q.R, q.mode, q.gather, SR_TIER_BASIC | SR_TIER_PARAM, 4, lk, q.vstk);
    }
    if (q.mode == SR_MODE_FOLD && !f32) return {};
    // FULL-tier loss and FOLD, PRED, EXACT: the FULL-tier build for every operator set, at RF rows per lane
    if (q.vstk || q.R != RF) return {};
    return sr_build_key(q.elem_size, RF, q.mode, q.gather, SR_TIER_FULL | SR_TIER_PARAM, 4, SR_LK_ANY, false);
  }

  if (q.family != SR_FAMILY_PLAIN) return {};
  if (q.mode == SR_MODE_FOLD && !f32) return {};  // (Float64: small calls only, from stored losses)

  if (q.vstk) {
    // register-stack builds: BASIC tier over the full view; LOSS at 8 / 16 / 32 rows per lane (f64: 4 / 8),
    // FOLD (f32) at 16 with the L2 or the generic build.  They ignore the request's waves: 4.
    if (q.tier != SR_TIER_BASIC || q.gather) return {};
    if (q.mode == SR_MODE_LOSS) {
      if (f32 ? (q.R != 8 && q.R != 16 && q.R != 32) : (q.R != 4 && q.R != 8)) return {};
      return sr_build_key(q.elem_size, q.R, SR_MODE_LOSS, false, SR_TIER_BASIC, 4, lk3, true);
    }
    if (q.mode != SR_MODE_FOLD || q.R != 16) return {};
    return sr_build_key(4, 16, SR_MODE_FOLD, false, SR_TIER_BASIC, 4, lk2, true);
  }

  if (q.mode == SR_MODE_FOLD) {
    // f32 classic FOLD: BASIC at 8 rows per lane and 4 waves (gathered: the generic build only), FULL at 4
    // rows per lane, whatever the request's waves
    if (q.tier == SR_TIER_BASIC) {
      if (q.R != 8 || q.waves != 4) return {};
      return sr_build_key(4, 8, SR_MODE_FOLD, q.gather, SR_TIER_BASIC, 4, q.gather ? SR_LK_ANY : lk2, false);
    }
    if (q.R != 4) return {};
    return sr_build_key(4, 4, SR_MODE_FOLD, q.gather, SR_TIER_FULL, 4, SR_LK_ANY, false);
  }

  // PRED: the FULL-tier build for every operator set; whatever R and waves
  if (q.mode == SR_MODE_PRED) return sr_build_key(q.elem_size, RF, SR_MODE_PRED, q.gather, SR_TIER_FULL, 4, SR_LK_ANY, false);

  // EXACT: per tier, whatever R; 4 waves, and every other request runs the 1-wave build
  if (q.mode == SR_MODE_EXACT)
    return sr_build_key(q.elem_size, RF, SR_MODE_EXACT, q.gather, q.tier == SR_TIER_BASIC ? SR_TIER_BASIC : SR_TIER_FULL,
                        q.waves == 4 ? 4 : 1, SR_LK_ANY, false);

  // FULL-tier loss: one build per view, whatever R and waves
  if (q.tier != SR_TIER_BASIC) return sr_build_key(q.elem_size, RF, SR_MODE_LOSS, q.gather, SR_TIER_FULL, 4, SR_LK_ANY, false);

  // BASIC loss, classic kernel.  f64: one build per view and loss, 4 rows per lane, whatever R and waves
  if (!f32) return sr_build_key(8, 4, SR_MODE_LOSS, q.gather, SR_TIER_BASIC, 4, lk3, false);
  // gathered f32 BASIC loss: one build per loss, 8 rows per lane, whatever R and waves
  if (q.gather) return sr_build_key(4, 8, SR_MODE_LOSS, true, SR_TIER_BASIC, 4, lk3, false);
  // 16 rows per lane: per loss, whatever waves
  if (q.R == 16) return sr_build_key(4, 16, SR_MODE_LOSS, false, SR_TIER_BASIC, 4, lk3, false);
  // 4 rows per lane: the generic build for every loss, whatever waves
  if (q.R == 4) return sr_build_key(4, 4, SR_MODE_LOSS, false, SR_TIER_BASIC, 4, SR_LK_ANY, false);
  // every other R runs 8 rows per lane; the 8-wave build exists for L2 only, every other loss runs 4 waves
  if (q.waves == 8 && l2) return sr_build_key(4, 8, SR_MODE_LOSS, false, SR_TIER_BASIC, 8, SR_LOSS_L2, false);
  return sr_build_key(4, 8, SR_MODE_LOSS, false, SR_TIER_BASIC, 4, lk3, false);
}

// ---------------------------------------------------------------- the host's launch shape
// What a scoring call plans its grids with (sr_capi.cpp choose_kernels): rows per lane of the classic kernel
// (R), waves per workgroup (W), and rows per lane of the register-stack kernel that takes the chunks whose
// programs need <= SR_VSTK_SLOTS stack slots (Rv; 0: none).  A parametric call's builds and an
// expression-loss call's (family LOSSX here: the call's, not a launch's) are smaller sets — the classic
// kernel at its default rows per lane, 4 waves, one register-stack build per type or none — so their
// "rows_per_lane" / "waves" / register-stack knobs map onto those.
struct SrLaunchShape {
  int R, W, Rv;
};
inline SrLaunchShape sr_launch_shape(int elem_size, int mode, int tier, bool gather, SrBuildFamily family, int64_t n_eval,
                                     int rows_override, int waves_override, int vstk_rows) {
  const bool small_set = family == SR_FAMILY_PARAM || family == SR_FAMILY_LOSSX;
  // (a row view has one classic build per tier, at the default rows per lane: "rows_per_lane" maps onto it.  Planned
  //  at 4 or 16 rows per lane, the 8-row build ran under a grid and a stored-loss layout of another tile size:
  //  it skipped rows, or wrote a tile past its position's rows)
  const int rq = (small_set || gather) ? 0 : rows_override;
  SrLaunchShape out;
  out.R = elem_size == 4 ? sr_rows_per_lane<float>(mode, tier, rq) : sr_rows_per_lane<double>(mode, tier, rq);
  out.W = small_set ? 4 : sr_waves_per_block(elem_size, mode, tier, out.R, waves_override);
  out.Rv = (mode == SR_MODE_LOSS && tier == SR_TIER_BASIC && !gather) ? sr_vstk_rows(elem_size, n_eval, vstk_rows ? vstk_rows : rows_override)
                                                                      : 0;
  if (family == SR_FAMILY_PARAM && out.Rv > 0) out.Rv = elem_size == 4 ? 16 : 8;  // (the one register-stack build of a parametric call)
  if (family == SR_FAMILY_LOSSX) out.Rv = 0;
  return out;
}
