// sr_knobs.h — the context's tuning knobs: their fields and defaults (SrKnobs, which sr_ctx derives from) and
// ONE table that states, per knob, its sr_set_tuning name, its environment variable and its range.
// sr_set_tuning (sr_knob_set) and sr_init (sr_knobs_from_env) both go through the table, so a knob has one
// range: sr_set_tuning clamps an out-of-range value into it, or refuses it where the row carries a message;
// the environment always clamps (sr_init never fails over a variable).  Host-only: no HIP
// (tools/knob_check.cpp checks it without a GPU).  include/sr_amd.h and DESIGN.md §4.7 describe the knobs
// for callers; this file is the authority on names, defaults and ranges.
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "sr_plan.h"  // kTailTwelfths, kFoldListWgsMax

struct SrKnobs {
  // SR_AMD_TAIL_CHUNK / "tail_chunk": a plain path-2 call whose loss launch composes candidates (C2's) runs
  // three chunks {1 / first_chunk, the rest, tail_chunk / 12} of the trees (sr_chunk_plan): the last two loss
  // launches end close together and their fold chains — latency-bound, each on its chunk's stream — run
  // side by side instead of one chain of 5/6 of the trees alone; 0: the two-chunk schedule
  int tail_chunk = 4;
  // SR_AMD_EXACT_EARLY / "exact_early": a multi-chunk loss call under the in-order fold copies its flags to
  // pinned memory behind the last chunk's reduce (every chunk's flags are final there) and records ev_flags;
  // eval_loss_finish waits for that event alone, lists the BIG trees and enqueues the exact-sum pass on a
  // third stream, which no chain occupies, so the pass runs beside the last chains; the call's one full
  // synchronisation follows.  0: the pass after that synchronisation, as before
  int exact_early = 1;
  int64_t fold_seg = -1;  // SR_AMD_FOLD_SEG / "fold_seg": -1 automatic, 0 one scan per tree
  // Small calls with several row blocks (round 5, SR_AMD_HOST_REDUCE / "host_reduce"): the
  // interpreter writes its per-(row block, tree) partials straight into pinned host memory (h_part)
  // and the host reduces them after the one stream synchronisation, in the reduce kernel's own order
  // (sr_reduce_positions: lane l folds row blocks l, l + 64, ...; a shfl_xor butterfly over the 64
  // lanes), so the bits are the reduce launch's; a C3 scoring call loses that launch and its gap.
  // The bound is on the call's partials (trees x row blocks): a C3 / C5 scoring call has ~1,600; a
  // 1,250-tree x 256-row-block call (320k partials) wrote 3.8 MB over PCIe and spent ~1 ms reducing on
  // the host (tools/share_probe.py: 2.47 ms per call against 1.1 with the reduce launch).
  int64_t host_reduce = 8192;
  // Small single-chunk LOSS calls (the search's regime: tens of trees, ~100 rows) are latency-bound:
  // SR_AMD_HOST_IO = 1 (default) lets the kernel write the per-tree results straight into pinned
  // host memory (no copy back); 0 copies them.  (Round 5's 2 — programs read from the pinned staging
  // buffer — was measured without payoff and removed in round 6.)
  int host_io = 1;
  int debug_hint_regrow = 0;  // tests ("debug_hint_regrow"): grow the hint array in place
  int exact_g = 0;            // SR_AMD_EXACT_G / "exact_g": listed trees per workgroup of the EXACT pass (0: heuristic)
  int exact_w = 4;            // SR_AMD_EXACT_W / "exact_w": waves per EXACT workgroup (4, or 1)
  // SR_AMD_DERIVED (default 1): nodes unary(feature) shared by several trees of a large LOSS call
  // are evaluated once per call into derived columns (LOAD_DERIVED); 0 disables
  int derived = 1;
  int stress_probe = 1;  // SR_AMD_STRESS_PROBE: the probe runs the dataset's stress rows
  int code_cache = 1;    // SR_AMD_CODE_CACHE: LDS program cache of the register-stack launches (0: off)
  int vstk_rows = 0;        // SR_AMD_VSTK_ROWS / "vstk_rows": rows per lane of the register-stack kernel (0: default)
  int grad_rows_force = 0;  // SR_AMD_GRAD_ROWS / "grad_rows": the gradient kernel's rows per lane (0: chosen per call)
  int grad_sort = 1;        // SR_AMD_GRAD_SORT / "grad_sort": gradient work items ordered by program cost
  int grad_lane_bins = 1;   // "grad_lane_bins": parametric gradients bin small slots x classes per lane (sr_eval.h)
  // "grad_stage_bytes": device staging of the per-row derivative calls (sr_eval_grad_tree_array / _diff_): work
  // items go out in chunks whose tangents stay within this many bytes, one item's own output when that is
  // larger; results do not depend on it
  int64_t grad_stage_bytes = int64_t(256) << 20;
  int first_chunk = 6;       // SR_AMD_FIRST_CHUNK: the two-chunk pipeline's first chunk is 1/first_chunk
  int64_t chunk_min = 1024;  // SR_AMD_CHUNK_MIN: the two-chunk pipeline runs when its first chunk holds this many trees
  int inject_fail = 0;         // tests ("inject_failure"): the next k collective-buffer growths fail
  int inject_post = 0;         // tests ("inject_failure_post"): a HIP failure right after the sharded all-reduce
  int inject_post_exact = 0;   // tests ("inject_failure_post_exact"): ... after the exact-sum all-gather
  int inject_post_gather = 0;  // tests ("inject_failure_post_gather" k): this rank's copy of the k-th fold gather fails
  int inject_post_wsum = 0;    // tests ("inject_failure_post_wsum"): this rank's copy of the weights' sum gather fails
  int timing = 1;           // 0: no timing events at all ("timing"; the search engine's calls)
  int rows_override = 0;    // SR_AMD_ROWS_PER_LANE (tuning): 4 selects the f32 BASIC 4-rows/lane kernel
  int tree_group = 0;       // SR_AMD_TREES_PER_BLOCK override (0 = heuristic)
  int waves_override = 0;   // SR_AMD_WAVES (tuning): 8 selects the 8-wave f32 BASIC L2 loss kernel
  bool cost_order = true;   // launch trees in decreasing estimated cost (SR_AMD_NO_SORT=1 disables)
  bool balance_groups = true;  // deal the cost order round-robin over tree groups (SR_AMD_BALANCE=0: contiguous)
  bool dead_hints = true;   // share dead-tree hints across row blocks (SR_AMD_NO_HINT=1 disables)
  // SR_AMD_MAX_ROW_BLOCKS (tuning): upper bound on row blocks per tree.  512 since round 5 (A/B, three
  // alternating passes on one box, profiles/r05_ab_row_blocks.txt): C2 4.47 vs 4.51 ms per step, C4
  // 1,520 vs 1,533 ms, the tree-sharding share (1,250 trees) 1.03 vs 1.09 ms: a small population keeps
  // 128 trees per workgroup instead of halving it to fill the GPU.  Results do not depend on it only
  // up to the f64 summation order of the partials (row blocks are a function of the rows alone).
  int max_row_blocks = 512;
  int chunks = 2;           // SR_AMD_CHUNKS: pipeline compile/launch over this many tree chunks (1 = off)
  int probe = 2;            // dead-tree probe launch (SR_AMD_PROBE): 0 off, 1 before every chunk,
                            // 2 (default) only before the chunks after the first, whose probe
                            // overlaps the first chunk's kernel (profiles/r01_ab_probe_modes.txt)
  // The reference's in-order loss fold for EVERY complete tree (round 6; sr_fold_dev.h, sr_aux.hip): a
  // complete tree's loss is LossFunctions' left-to-right fold in T of its elementwise losses
  // (src/LossFunctions.jl:38-58), divided in T, not the device's f64 sum.  SR_AMD_REF_FOLD / "ref_fold":
  // 1 (default) single-GPU loss calls with weights >= 0; 0 the f64 sums (rounds 1-5).  Small calls
  // (every tree's losses fit fold_store_mb) keep the loss launch's losses; larger Float32 calls run the
  // complete trees again in FOLD mode (slow segments' losses in up to fold_slot_mb of slots); larger
  // Float64 calls, and calls whose row blocks pass fold_seg_max rows (C4: 2^26 rows per GPU), keep the f64
  // sum (Float64: within ~1e-13 of the fold, north_star's f64 bar is 1e-10).
  int ref_fold = 1;
  int64_t fold_store_mb = 512;
  int64_t fold_slot_mb = 24576;  // (allocated as needed: ~24 slots per tree; C4's 2^26 rows take ~21 GB)
  // the plan's window: the fold within 2^-8 of the f64 prefix, else the tree fails (C2's trees: the fold is
  // within 2.1e-3 of the f64 sum at 2^20 rows; 2^-6 kept twice the slow segments)
  int fold_delta_log2 = 8;
  int64_t fold_seg_max = 16384;  // SR_AMD_FOLD_SEG_MAX: calls whose row blocks are longer keep the f64 sum
  int64_t fold_rows_max = int64_t(1) << 24;  // SR_AMD_FOLD_ROWS_MAX: longer folds keep the f64 sum
  int fold_debug_fail = 0;   // (tests: "fold_debug_fail")
  // SR_AMD_FOLD_SINGLE_PASS / "fold_single_pass": the loss launch of a FOLD-mode call (path 2) composes each
  // row block's steps under candidate binades, and the plan takes the blocks whose binade is among
  // them, so the FOLD pass runs only what is left (0: every block of every complete tree again).  Plain
  // single-GPU Float32 BASIC calls over the full view, register-stack launch; every other call keeps the
  // two passes.
  int fold_single_pass = 1;
  // SR_AMD_FOLD_COMPACT / "fold_compact": the FOLD pass of a plain path-2 call runs over per-row-block lists
  // of the positions the plan left it (sr_fold_compact_kernel), G per workgroup, instead of the loss
  // launch's (row block, tree group) grid (0).  Gathered, parametric and row-sharded calls keep the grid.
  int fold_compact = 1;
  // SR_AMD_FOLD_LIST_WGS / "fold_list_wgs": the live workgroups a compacted FOLD launch aims for.  Its list's
  // entries per workgroup g is chosen on the device from the row blocks' counts (sr_fold_compact_scan_kernel,
  // sr_plan.h's sr_fold_list_g): the smallest multiple of the 4 waves that keeps the launch within this many
  // workgroups and within its grid.  0: g = G, the launch's trees per workgroup — C2's row blocks list ~100
  // positions each, so one workgroup per row block, ~27 trees a wave in turn on half the GPU's wave slots.
  // Smaller g: more workgroups stage a row block's tiles for fewer trees each.
  int64_t fold_list_wgs = 2048;
  // SR_AMD_LOSS_COMPACT / "loss_compact": the candidate-composing loss launch of such a call runs over the
  // launch positions its chunk's dead-tree probe left alive, less the statically incomplete trees
  // (sr_loss_compact_kernel: one list per launch, dealt over the launch's tree groups, the live workgroups
  // first), and the reduce gives the excluded positions their result without reading a partial (0: every
  // position, the launch sequence before the list).
  int loss_compact = 1;
  // SR_AMD_LOSS_LIST_GROUPS / "loss_list_groups": the most tree groups a listed launch deals its list over (0,
  // the default: all of its grid's; sr_loss_compact_kernel: fewer groups = fewer workgroups to stage tiles,
  // but the candidates' guess from the running prefix lags by resident workgroups / groups row blocks, and
  // which of a call's overlapping launches ends last moves with it: DESIGN.md §12)
  int loss_list_groups = 0;
  // SR_AMD_FOLD_CAND_EST / "fold_cand_est": the candidates' guess from the tree's running prefix (the row
  // blocks other workgroups have finished; 0: the block's first tile only); usable from fold_cand_est_min
  // finished blocks on (SR_AMD_FOLD_CAND_EST_MIN; tools/fold_cand_sim.py)
  int fold_cand_est = 1;
  int fold_cand_est_min = 4;
  int fold_stats = 0;  // SR_AMD_FOLD_STATS=1: per-tree walk statistics to stderr after each call (analysis)
};

// What a row does to a value before it is stored: RANGE clamps into [lo, hi]; FLAG stores value != 0;
// EXACT_W stores 1 for 1 and 4 for anything else.
enum SrKnobNorm : uint8_t { SR_KNOB_RANGE, SR_KNOB_FLAG, SR_KNOB_EXACT_W };

struct SrKnobRow {
  const char* name;  // sr_set_tuning's name (NULL: the environment only)
  const char* env;   // the environment variable (NULL: sr_set_tuning only)
  int SrKnobs::*i32;      // the member: exactly one of the three is set
  int64_t SrKnobs::*i64;
  bool SrKnobs::*flag;
  SrKnobNorm norm;
  int64_t lo, hi;      // RANGE: the range (the value is clamped in int64, then converted to the member's type)
  const char* refuse;  // non-NULL: sr_set_tuning refuses a value outside [lo, hi] with this message
  bool env_inverse;    // the variable has the inverse sense (SR_AMD_NO_SORT=1 clears cost_order)

  constexpr SrKnobRow(const char* n, const char* e, int SrKnobs::*m, SrKnobNorm nm = SR_KNOB_RANGE, int64_t l = INT64_MIN,
                      int64_t h = INT64_MAX, const char* r = nullptr)
      : name(n), env(e), i32(m), i64(nullptr), flag(nullptr), norm(nm), lo(l), hi(h), refuse(r), env_inverse(false) {}
  constexpr SrKnobRow(const char* n, const char* e, int64_t SrKnobs::*m, int64_t l = INT64_MIN, int64_t h = INT64_MAX)
      : name(n), env(e), i32(nullptr), i64(m), flag(nullptr), norm(SR_KNOB_RANGE), lo(l), hi(h), refuse(nullptr),
        env_inverse(false) {}
  constexpr SrKnobRow(const char* n, const char* e, bool SrKnobs::*m, bool inverse = false)
      : name(n), env(e), i32(nullptr), i64(nullptr), flag(m), norm(SR_KNOB_FLAG), lo(0), hi(1), refuse(nullptr),
        env_inverse(inverse) {}
};

constexpr int64_t kKnobMax = INT64_MAX;

// One row per knob.  A row without bounds stores the value as given (converted to the member's type).
constexpr SrKnobRow kSrKnobs[] = {
    // kernel build and grid
    {"rows_per_lane", "SR_AMD_ROWS_PER_LANE", &SrKnobs::rows_override},
    {"trees_per_block", "SR_AMD_TREES_PER_BLOCK", &SrKnobs::tree_group, SR_KNOB_RANGE, 0, 256,
     "trees_per_block: 0, or 1..256 (4 waves of 64 slots)"},
    {nullptr, "SR_AMD_WAVES", &SrKnobs::waves_override},
    {"vstk_rows", "SR_AMD_VSTK_ROWS", &SrKnobs::vstk_rows},
    {"max_row_blocks", "SR_AMD_MAX_ROW_BLOCKS", &SrKnobs::max_row_blocks, SR_KNOB_RANGE, 1, 1 << 16},
    {"code_cache", "SR_AMD_CODE_CACHE", &SrKnobs::code_cache, SR_KNOB_FLAG},
    {"derived", "SR_AMD_DERIVED", &SrKnobs::derived, SR_KNOB_FLAG},
    // launch order, dead-tree probe and hints
    {nullptr, "SR_AMD_NO_SORT", &SrKnobs::cost_order, true},
    {"balance", "SR_AMD_BALANCE", &SrKnobs::balance_groups},
    {nullptr, "SR_AMD_NO_HINT", &SrKnobs::dead_hints, true},
    {"probe", "SR_AMD_PROBE", &SrKnobs::probe},
    {"stress_probe", "SR_AMD_STRESS_PROBE", &SrKnobs::stress_probe, SR_KNOB_FLAG},
    // the chunked pipeline
    {nullptr, "SR_AMD_CHUNKS", &SrKnobs::chunks},
    {"first_chunk", "SR_AMD_FIRST_CHUNK", &SrKnobs::first_chunk, SR_KNOB_RANGE, 2, 64},
    {"chunk_min", "SR_AMD_CHUNK_MIN", &SrKnobs::chunk_min, 1, kKnobMax},
    {"tail_chunk", "SR_AMD_TAIL_CHUNK", &SrKnobs::tail_chunk, SR_KNOB_RANGE, 0, kTailTwelfths,
     "tail_chunk: 0, or the last chunk's twelfths 1..6"},
    // small calls
    {"host_io", "SR_AMD_HOST_IO", &SrKnobs::host_io, SR_KNOB_RANGE, 0, 1, "host_io must be 0 or 1"},
    {"host_reduce", "SR_AMD_HOST_REDUCE", &SrKnobs::host_reduce, 0, kKnobMax},
    {"timing", nullptr, &SrKnobs::timing, SR_KNOB_FLAG},
    // the exact-sum pass
    {"exact_g", "SR_AMD_EXACT_G", &SrKnobs::exact_g, SR_KNOB_RANGE, 0, 64},
    {"exact_w", "SR_AMD_EXACT_W", &SrKnobs::exact_w, SR_KNOB_EXACT_W},
    {"exact_early", "SR_AMD_EXACT_EARLY", &SrKnobs::exact_early, SR_KNOB_FLAG},
    // gradients
    {"grad_rows", "SR_AMD_GRAD_ROWS", &SrKnobs::grad_rows_force},
    {"grad_sort", "SR_AMD_GRAD_SORT", &SrKnobs::grad_sort, SR_KNOB_FLAG},
    {"grad_lane_bins", nullptr, &SrKnobs::grad_lane_bins, SR_KNOB_FLAG},
    {"grad_stage_bytes", nullptr, &SrKnobs::grad_stage_bytes, 1, kKnobMax},
    // the in-order loss fold
    {"ref_fold", "SR_AMD_REF_FOLD", &SrKnobs::ref_fold, SR_KNOB_FLAG},
    {"fold_seg", "SR_AMD_FOLD_SEG", &SrKnobs::fold_seg, -1, kKnobMax},
    {"fold_store_mb", "SR_AMD_FOLD_STORE_MB", &SrKnobs::fold_store_mb, 0, kKnobMax},
    {"fold_slot_mb", "SR_AMD_FOLD_SLOT_MB", &SrKnobs::fold_slot_mb, 1, kKnobMax},
    {"fold_delta_log2", "SR_AMD_FOLD_DELTA_LOG2", &SrKnobs::fold_delta_log2, SR_KNOB_RANGE, 1, 40},
    {"fold_seg_max", "SR_AMD_FOLD_SEG_MAX", &SrKnobs::fold_seg_max, 0, kKnobMax},
    {"fold_rows_max", "SR_AMD_FOLD_ROWS_MAX", &SrKnobs::fold_rows_max, 0, kKnobMax},
    {"fold_single_pass", "SR_AMD_FOLD_SINGLE_PASS", &SrKnobs::fold_single_pass, SR_KNOB_FLAG},
    {"fold_compact", "SR_AMD_FOLD_COMPACT", &SrKnobs::fold_compact, SR_KNOB_FLAG},
    {"fold_list_wgs", "SR_AMD_FOLD_LIST_WGS", &SrKnobs::fold_list_wgs, 0, kFoldListWgsMax},
    {"loss_compact", "SR_AMD_LOSS_COMPACT", &SrKnobs::loss_compact, SR_KNOB_FLAG},
    {"loss_list_groups", "SR_AMD_LOSS_LIST_GROUPS", &SrKnobs::loss_list_groups, SR_KNOB_RANGE, 0, 1 << 20},
    {"fold_cand_est", "SR_AMD_FOLD_CAND_EST", &SrKnobs::fold_cand_est, SR_KNOB_FLAG},
    {"fold_cand_est_min", "SR_AMD_FOLD_CAND_EST_MIN", &SrKnobs::fold_cand_est_min, SR_KNOB_RANGE, 1, 1 << 30},
    {nullptr, "SR_AMD_FOLD_STATS", &SrKnobs::fold_stats},
    // tests only
    {"fold_debug_fail", nullptr, &SrKnobs::fold_debug_fail, SR_KNOB_RANGE, 0, kKnobMax},
    {"debug_hint_regrow", nullptr, &SrKnobs::debug_hint_regrow, SR_KNOB_FLAG},
    {"inject_failure", nullptr, &SrKnobs::inject_fail},
    {"inject_failure_post", nullptr, &SrKnobs::inject_post},
    {"inject_failure_post_exact", nullptr, &SrKnobs::inject_post_exact},
    {"inject_failure_post_gather", nullptr, &SrKnobs::inject_post_gather},
    {"inject_failure_post_wsum", nullptr, &SrKnobs::inject_post_wsum},
};

// Stores v through the row.  `clamp`: an out-of-range value of a refusing row is clamped (the environment's
// rule) instead of refused.  Returns false, and leaves the member alone, when the row refuses the value.
inline bool sr_knob_store(SrKnobs& k, const SrKnobRow& r, int64_t v, bool clamp) {
  if (r.refuse && !clamp && (v < r.lo || v > r.hi)) return false;
  switch (r.norm) {
    case SR_KNOB_FLAG: v = v != 0 ? 1 : 0; break;
    case SR_KNOB_EXACT_W: v = v == 1 ? 1 : 4; break;
    case SR_KNOB_RANGE: v = v < r.lo ? r.lo : (v > r.hi ? r.hi : v); break;
  }
  if (r.i32) k.*r.i32 = int(v);
  else if (r.i64) k.*r.i64 = v;
  else k.*r.flag = v != 0;
  return true;
}

// sr_set_tuning's body: 0 when the knob took the value; 1 with *err set for an unknown name or a refused
// value (the member keeps its value).
inline int sr_knob_set(SrKnobs& k, const char* name, int64_t v, std::string* err) {
  for (const SrKnobRow& r : kSrKnobs) {
    if (!r.name || strcmp(name, r.name) != 0) continue;
    if (sr_knob_store(k, r, v, false)) return 0;
    if (err) *err = r.refuse;
    return 1;
  }
  if (err) *err = std::string("unknown tuning knob '") + name + "'";
  return 1;
}

// sr_init's part: every row's variable that `get` (getenv) returns a value for, parsed as a decimal integer
// and clamped into the row's range.
inline void sr_knobs_from_env(SrKnobs& k, const char* (*get)(const char*)) {
  for (const SrKnobRow& r : kSrKnobs) {
    const char* s = r.env ? get(r.env) : nullptr;
    if (!s) continue;
    const int64_t v = atoll(s);
    (void)sr_knob_store(k, r, r.env_inverse ? (v == 0 ? 1 : 0) : v, true);
  }
}
