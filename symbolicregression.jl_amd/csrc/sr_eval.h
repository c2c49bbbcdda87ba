// sr_eval.h — kernel argument block and launchers shared by the kernels and the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sr_ops.h"
#include "sr_loss_expr.h"  // the expression-loss program and its interpreters (HIP-free)
#include "sr_plan.h"  // modes, tiers, SrSegment, SrDerivedSpec, the launch-shape functions (HIP-free)
#include "sr_builds.h"  // the builds of sr_tile_kernel, SrBuildRequest and the rule that resolves one (HIP-free)
#include "../../include/sr_amd.h"

// The deferred checks leave bounded outputs untracked (sr_tile_impl.h sr_untracked_u / _b; round 5:
// C2 kernel -4 %, arithmetic-only -9 %, profiles/r05_ab_track_lite.txt); -DSR_TRACK_FULL tracks all.
#ifndef SR_TRACK_FULL
#define SR_TRACK_LITE 1
#endif
// Per-tree reduction of [row block][position] partials, one wave per tree: lane l folds row blocks
// l, l + 64, ... in order, then a fixed shfl_xor butterfly adds the 64 lane sums; lane 0 writes the
// tree's Σ and OR of flags (static_bad ORed in) at perm[position].  The wave handles `count`
// positions pos0, pos0 + step, ...; K of them at a time, so their loads are in flight together.
template <int K>
__device__ inline void sr_reduce_positions(const double* part_sum, const uint32_t* part_flag, int n_trees,
                                           int n_row_blocks, int pos0, int step, int count,
                                           const uint32_t* perm, const uint8_t* static_bad, double* out_sum,
                                           uint32_t* out_flag, int lane) {
  for (int j0 = 0; j0 < count; j0 += K) {
    double s[K];
    uint32_t f[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      s[k] = 0.0;
      f[k] = 0u;
    }
    for (int i = lane; i < n_row_blocks; i += 64) {
#pragma unroll
      for (int k = 0; k < K; ++k) {
        if (j0 + k < count) {
          const size_t o = size_t(i) * size_t(n_trees) + size_t(pos0 + (j0 + k) * step);
          s[k] += part_sum[o];
          f[k] |= part_flag[o];
        }
      }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) {
        s[k] += __shfl_xor(s[k], off, 64);
        f[k] |= __shfl_xor(f[k], off, 64);
      }
    }
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < K; ++k) {
        if (j0 + k < count) {
          const int pos = pos0 + (j0 + k) * step;
          const int tree = perm ? int(perm[pos]) : pos;
          uint32_t fl = f[k];
          if (static_bad && static_bad[tree]) fl |= SR_FLAG_STATIC | SR_FLAG_NONFINITE;
          out_sum[tree] = s[k];
          out_flag[tree] = fl;
        }
      }
    }
  }
}

template <typename T>
struct SrEvalArgs {
  // programs
  const SrIns<T>* code;
  const uint32_t* offsets;     // [n_trees + 1], indexed by the caller's tree index
  const uint32_t* ends;        // [n_trees] end of each tree's program (NULL: offsets[t + 1]); programs are
                               // staged in launch order, so a tree group's code is one contiguous span
  const uint32_t* perm;        // launch position -> caller's tree index (NULL: identity); EXACT: tree list
  uint32_t* hint;              // [n_trees] per position: dead-tree hints across row blocks (LOSS; may be NULL)
  uint32_t hint_epoch;         // a position is dead when its hint equals this call's epoch (no reset pass)
  int n_trees;                 // trees (or listed trees in EXACT mode)
  int trees_per_block;         // G
  // data (per-feature rows, leading dimension ld; padded rows replicate row 0)
  const T* X;
  const T* y;                  // may be NULL (prediction only)
  const T* w;                  // NULL -> unweighted
  const int64_t* row_idx;      // GATHER mode: rows of the SubDataset
  int64_t ld;
  const T* derived;            // LOAD_DERIVED columns [k][dld] over the rows of the view (NULL: none)
  int64_t dld;
  int64_t n_rows;              // rows evaluated
  int nf;
  int tiles_per_block;
  int n_row_blocks;
  int n_groups;                // tree groups (blockIdx = row_block * n_groups + group)
  int stack_depth;             // LDS operand-stack slots per wave (>= 1)
  int code_lds;                // LOSS: instructions of LDS program cache per workgroup (0: windows
                               // stream from global memory); a group whose span exceeds it streams too
  T tbig;                      // |v| >= tbig may overflow the array-sum check
  double big_budget;           // a tile holding |v| >= tbig is BIG only when its lanes' Σ max|v| passes this
                               // (64 x floatmax / (1.01 x the view's padded rows, every shard)): below it,
                               // no checked array's Julia-order sum can reach floatmax (sr_tile_impl.h)
  int track_x;                 // the data holds |x| >= tbig or non-finite values: checked feature
                               // loads join the deferred checks (FAST path)
  int loss_kind;               // SrLossKind
  T loss_param;                // its parameter (HuberLoss delta, QuantileLoss tau, ...)
  // outputs
  double* part_sum;            // [n_row_blocks][n_trees], per launch position
  uint32_t* part_flag;         // [n_row_blocks][n_trees], per launch position
  // single row block (n_row_blocks == 1): the per-tree results go straight to out_sum / out_flag
  // (tree order, static_bad ORed in) and no reduce launch follows; NULL otherwise
  double* out_sum;
  uint32_t* out_flag;
  const uint8_t* static_bad;
  T* pred;                   // PRED: [n_trees][pred_ld]
  int64_t pred_ld;
  // EXACT mode (perm = listed trees): row block rb = row range [range_lo[rb], range_hi[rb]] of the
  // view; range_sums[list position][check][rb] (T) = Julia-order sum of the checked array over it
  int max_checks;
  const int64_t* range_lo;
  const int64_t* range_hi;
  void* range_sums;
  // several row views in one launch (GATHER LOSS; NULL: one view, blockIdx = row_block * n_groups + group)
  const SrSegment* segs;
  int n_segs;
  // the reference's in-order loss fold (round 6, sr_fold_dev.h).  LOSS: fold_loss non-NULL stores every
  // evaluated tree's elementwise losses at fold_loss[position * fold_pos_stride + row] (small calls: the
  // fold's tables are composed from them).  FOLD: fold_code [n_row_blocks][n_trees] per position (the
  // plan), fold_tab the same shape of composed-step pairs (SrFoldTab<T>::Pair, written for steps
  // segments), fold_loss the slow segments' losses, slot (code - SR_FCODE_SLOT0) x fold_slot_rows.
  // fold_sq / fold_tab2 (same shape): a slow segment's lower window binade, and the composed steps of
  // its rows under that binade (in fold_tab) and the next (fold_tab2), so that the walk advances a slow
  // segment the running value does not actually leave a binade in without reading its rows
  T* fold_loss;
  int64_t fold_pos_stride;
  const int32_t* fold_code;
  void* fold_tab;
  int64_t fold_slot_rows;
  const int32_t* fold_sq;
  void* fold_tab2;
  // -DSR_STAMPS builds only (latency analysis, tools/stamps.py): per wave, SR_NSTAMPS wall-clock
  // stamps at fixed points of the kernel, [block][wave][SR_NSTAMPS]; NULL otherwise
  uint64_t* stamps;
  // the builds for parametric calls (SR_TIER_PARAM; no other kernel reads these): the call's table,
  // ptab[tree * p_stride + k * n_classes + class] at the caller's tree index (as `offsets`).  The rows' 0-based
  // classes are the last staged X row (the dataset's hidden row: nf counts it).
  const T* ptab;
  int p_stride;
  int n_classes;
  // SR_TIER_CAND loss builds (last: every other kernel's argument offsets stay as they were):
  // [n_row_blocks][n_trees] per position, {q0, the block's step under q0, q0 + 1, q0 + 2} (sr_fold_dev.h);
  // the plan takes a steps block's pair from here when its binade is one of them, and the FOLD pass then
  // skips the block
  int4* fold_cand;
  // FOLD, the compacted launch (NULL: workgroup = (row block, tree group) as in the loss launch): per row
  // block rb the launch positions the FOLD pass must run, in launch order, fold_list[rb * n_trees + k],
  // k < fold_cnt[rb]; workgroups fold_wg0[rb] .. fold_wg0[rb + 1] - 1 take g <= G of them each
  // (fold_wg0[n_row_blocks]: the total; workgroups past it return at once; fold_wg0[n_row_blocks + 1]: g,
  // chosen on the device from the counts).  sr_fold_compact_kernel, sr_fold_compact_scan_kernel.
  // LOSS, the SR_TIER_CAND build's listed launch (NULL: every position): ONE list for the launch, the
  // positions the dead-tree probe left alive (statically incomplete trees left out too), in launch order, fold_list[k], k < fold_cnt[0]; workgroup b
  // takes entries [tg g, tg g + g) of row block rb, g = fold_cnt[1] <= G, tg = b % fold_cnt[2], rb = b / that,
  // and returns at once past the last row block (the grid is the region's); every per-position array
  // keeps its [row block][position] layout.  sr_loss_compact_kernel.
  const int32_t* fold_list;
  const int32_t* fold_cnt;
  const int32_t* fold_wg0;
  // SR_TIER_CAND loss builds, the candidates' guess from the running prefix (NULL: the first-tile guess
  // only): per position, the f64 sum of the row blocks finished so far and their count (relaxed
  // agent-scope adds at a workgroup's end; a workgroup reads its trees' pair at its start: only ever a
  // guess), usable from fold_est_min blocks on.  Zeroed by the host before the call.
  double* fold_est_sum;
  uint32_t* fold_est_cnt;
  uint32_t fold_est_min;
  // SR_LOSS_EXPR loss builds (last again, no other kernel reads them): the loss
  // program (sr_loss_expr.h) in a device buffer of the context — not in the argument block, which is host
  // memory here — read with wave-uniform loads, and its length
  const SrIns<T>* lx_code;
  int lx_n;
};
constexpr int SR_NSTAMPS = 8;

template <typename T, int R, int MODE, bool GATHER, int TIER, int W = 4, int LK = -1, bool VSTK = false>
hipError_t sr_launch_tile(const SrEvalArgs<T>& a, int n_blocks, hipStream_t s);
// The one launcher of the tile kernels: resolves the request (sr_builds.h: sr_resolve_build) and launches
// the build it names; hipErrorInvalidValue for a refused request, a build that is not in the table, a
// request whose element size or loss kind is not the arguments', and arguments the build needs but lacks
// (SR_TIER_CAND: fold_cand; SR_LOSS_EXPR: the loss program; SR_TIER_PARAM: the table, in sr_launch_tile).
template <typename T>
hipError_t sr_launch_eval(const SrEvalArgs<T>& a, const SrBuildRequest& req, int n_blocks, hipStream_t s);
template <typename T>
hipError_t sr_launch_derived(const T* X, int64_t ld, const int64_t* row_idx, int64_t n_view, int64_t n_pad,
                             const SrDerivedSpec& spec, T* out, int64_t dld, hipStream_t s);

hipError_t sr_launch_reduce(const double* part_sum, const uint32_t* part_flag, int n_trees, int n_row_blocks,
                            const uint32_t* perm, const uint8_t* static_bad, double* out_sum, uint32_t* out_flag,
                            hipStream_t s);
// The listed loss launch (SrEvalArgs::fold_list in a SR_TIER_CAND loss launch): the region's np launch
// positions whose hint is not `epoch` and whose tree (perm[position]) is not static_bad, in launch order,
// list[0 .. cnt[0]); cnt[1] entries per workgroup, cnt[2] workgroups per row block (the list dealt over the
// launch's grid_groups groups of G, or over want_groups > 0 of them); excl[p] = 1 for the others.  And
// the reduce behind it: sr_launch_reduce for the listed positions, Σ 0 | SR_FLAG_NONFINITE (| SR_FLAG_STATIC)
// for an excluded one.
hipError_t sr_launch_loss_compact(const uint32_t* hint, uint32_t epoch, int np, const uint32_t* perm,
                                  const uint8_t* static_bad, int G, int grid_groups, int want_groups, int32_t* list,
                                  int32_t* cnt, uint8_t* excl, hipStream_t s);
hipError_t sr_launch_reduce_excl(const double* part_sum, const uint32_t* part_flag, int n_trees, int n_row_blocks,
                                 const uint32_t* perm, const uint8_t* static_bad, const uint8_t* excl, double* out_sum,
                                 uint32_t* out_flag, hipStream_t s);
// isfinite(Julia pairwise sum) of n_arrays arrays from their leaf folds [n_arrays][n_leaves] (T),
// combined by the post-order program `prog` (leaf index: push; -1: add the top two).
template <typename T>
hipError_t sr_launch_jsum_levels(const T* leaf_sums, int64_t n_arrays, int n_leaves, const int2* nodes, int n_internal,
                                 const int32_t* level_off, int n_levels, T* scratch, uint8_t* out, hipStream_t s);
hipError_t sr_launch_pack_partials(const double* sum, const uint32_t* flag, int n, double* out, hipStream_t s);
// comp codes of the row-sharded finalize: 0 incomplete, 1 complete, 2 BIG only (exact check pending),
// | SR_COMP_FOLD: the loss fold is computed in order (sr_fold.h)
constexpr int SR_COMP_FOLD = 4;
template <typename T>
hipError_t sr_launch_finalize_packed(const double* packed, int n, double denom, int64_t n_terms, T* loss, uint8_t* comp,
                                     hipStream_t s);
template <typename T>
hipError_t sr_launch_transpose(const T* Xh_dev, int64_t nf, int64_t n, int64_t ld, T* Xd, hipStream_t s);
template <typename T>
hipError_t sr_launch_pad(T* v, int64_t n, int64_t ld, T pad_value, int replicate_first, hipStream_t s);

// Arguments of the forward-mode constant-gradient kernel (csrc/sr_grad_impl.h).
template <typename T>
struct SrGradArgs {
  const SrIns<T>* code;
  const uint32_t* offsets;   // [n_trees + 1]
  const T* consts;           // pre-order constants of every tree
  const uint32_t* const_off; // [n_trees + 1]
  const uint32_t* item_tree; // work item -> tree
  const uint32_t* item_k0;   // work item -> first tangent (constant index)
  int n_items;
  const T* X;
  const T* y;
  const T* w;
  const int64_t* row_idx;    // GATHER: rows of the SubDataset
  int64_t ld;
  int64_t n_rows;
  int nf;
  int tiles_per_block;
  int n_row_blocks;
  int n_groups;
  int stack_depth;
  int loss_kind;
  T loss_param;
  double* part;              // [n_row_blocks][n_items][KT]
  const SrSegment* segs;     // several row views (GATHER; positions = work items); NULL: one view
  int n_segs;
};

// rows: rows per lane, sr_grad_rows_per_lane(kt) or 1 (sr_grad_launch_rows)
template <typename T>
hipError_t sr_launch_grad_any(const SrGradArgs<T>& a, int kt, bool gather, int rows, int n_blocks, hipStream_t s);
// Largest rows per lane of the gradient kernel for KT tangents (a staged tile is 64 x that many rows);
// kernels exist for it, its halves down to 2, and 1.
constexpr int sr_grad_rows_per_lane(int kt) { return kt <= 2 ? 8 : (kt <= 4 ? 4 : (kt <= 8 ? 2 : 1)); }
// Rows of a staged gradient tile at `rows` rows per lane: 256, or one program pass when that is longer
// (a divisor of the host's 512-row units)
constexpr int sr_grad_tile_rows(int rows) { return 64 * rows > 256 ? 64 * rows : 256; }
// LDS of one gradient workgroup (W waves): the X / y / w tile and the waves' operand stacks (value +
// KT tangents per row, stack_depth slots)
// n_classes > 0: a parametric launch — the hidden class row is staged too, and every wave keeps f64 class
// bins behind the stacks: [kt][n_classes], or with lane_slots > 0 one accumulator per lane,
// [lane_slots][n_classes][64] (sr_grad_param_lane_slots)
inline size_t sr_grad_lds_bytes(int elem_size, int kt, int rows, int nf, bool weighted, int stack_depth, int waves,
                                int n_classes = 0, int lane_slots = 0) {
  return (size_t(nf) + 1 + (weighted ? 1 : 0) + (n_classes > 0 ? 1 : 0)) * size_t(sr_grad_tile_rows(rows)) * size_t(elem_size) +
         size_t(waves) * size_t(stack_depth) * size_t(1 + kt) * size_t(rows) * 64 * size_t(elem_size) +
         size_t(waves) * size_t(lane_slots > 0 ? lane_slots * 64 : kt) * size_t(n_classes > 0 ? n_classes : 0) * sizeof(double);
}
// Rows per lane a bucket of KT tangents runs with (results do not depend on it): `force` when it is
// one the kernels exist for and fits; otherwise the preferred count (Float32: the largest; Float64:
// half of it — the f64 value and tangents of 8 rows need ~190 VGPRs, two waves per SIMD), halved
// while the workgroup's LDS (tile + operand stacks, which grow with the bucket's deepest program)
// passes lds_max / 2, so that two workgroups share a CU; 0 when even one row per lane does not fit.
inline int sr_grad_launch_rows(int elem_size, int kt, int nf, bool weighted, int stack_depth, int waves, size_t lds_max,
                               int force = 0) {
  const int rmax = sr_grad_rows_per_lane(kt);
  auto fits = [&](int r, size_t cap) { return sr_grad_lds_bytes(elem_size, kt, r, nf, weighted, stack_depth, waves) <= cap; };
  auto valid = [&](int r) { return r == 1 || (r <= rmax && r >= 2 && (r & (r - 1)) == 0); };
  if (force > 0 && valid(force) && fits(force, lds_max)) return force;
  int r = elem_size == 8 && rmax > 1 ? rmax / 2 : rmax;
  while (r > 1 && !fits(r, lds_max / 2)) r /= 2;
  if (fits(r, lds_max)) return r;
  return fits(1, lds_max) ? 1 : 0;
}
hipError_t sr_launch_grad_reduce(const double* part, int n_row_blocks, int n_vals, double* out, hipStream_t s);
// The parametric build of the gradient kernel (sr_grad_param_kernel: ParametricExpression trees).  A tree's
// tangents are its constants, then the parameters it uses in ascending index (tan_par[tan_off[t] ..
// tan_off[t + 1])); work items are windows of that list.  A parameter tangent's per-class sums go to
// ppart[row block][n_bins] at item_bin[item] + (its rank among the window's parameter tangents) x n_classes
// + class; SrGradArgs::nf counts the staged hidden class row.
template <typename T>
struct SrGradParamArgs {
  const T* ptab;              // [tree][parameter][class], as SrEvalArgs::ptab
  int p_stride;
  int n_classes;
  const uint32_t* tan_off;    // [n_trees + 1]
  const uint32_t* tan_par;    // used parameter indices (0-based)
  const uint32_t* item_bin;   // [n_items]
  double* ppart;
  int n_bins;
  int lane_slots;             // > 0: per-lane class accumulators for that many parameter tangents per window
};
// The binning scheme of a parametric launch of kt tangents: 0 = per 64-row group one masked wave sum per
// class present (any n_classes); s > 0 = per-lane accumulators [s][n_classes][64], s = min(kt,
// max_parameters) the most parameter tangents a window can hold, taken for Float32 while s x n_classes <= 16
// (32 KiB of LDS at 4 waves; measured: at 8 classes the Float32 kernels run 19 % shorter with it, the Float64
// ones 22 % longer — DESIGN.md 13.1 — so Float64 keeps the wave sums).  The two sum in different orders, so which one runs must not depend on the launch: it
// follows from the element type, the tree's own width, the batch's max_parameters and the dataset's classes alone (and the
// "grad_lane_bins" knob, which results therefore depend on).
constexpr int sr_grad_param_lane_slots(int elem_size, int kt, int max_parameters, int n_classes, bool allowed = true) {
  const int s = kt < max_parameters ? kt : max_parameters;
  return allowed && elem_size == 4 && s > 0 && s * n_classes <= 16 ? s : 0;
}
// Rows per lane of the parametric builds: this (the plain kernel's preferred count) and 1.
constexpr int sr_grad_param_rows(int elem_size, int kt) {
  return elem_size == 8 && sr_grad_rows_per_lane(kt) > 1 ? sr_grad_rows_per_lane(kt) / 2 : sr_grad_rows_per_lane(kt);
}
// As sr_grad_launch_rows over that set (class row and bins in the LDS): `force` when it is one of the
// two and fits; the preferred count while two workgroups share a CU, else 1; 0 when 1 does not fit.
inline int sr_grad_param_launch_rows(int elem_size, int kt, int nf, bool weighted, int stack_depth, int waves,
                                     size_t lds_max, int n_classes, int lane_slots, int force = 0) {
  const int pref = sr_grad_param_rows(elem_size, kt);
  auto fits = [&](int r, size_t cap) {
    return sr_grad_lds_bytes(elem_size, kt, r, nf, weighted, stack_depth, waves, n_classes, lane_slots) <= cap;
  };
  if (force > 0 && (force == 1 || force == pref) && fits(force, lds_max)) return force;
  if (fits(pref, lds_max / 2)) return pref;
  return fits(1, lds_max) ? 1 : 0;
}
template <typename T, bool GATHER>
hipError_t sr_launch_grad_param_any(const SrGradArgs<T>& a, const SrGradParamArgs<T>& p, int kt, int rows, int n_blocks,
                                    hipStream_t s);
// The expression-loss build of the gradient kernel (sr_grad_lossx_kernel, sr_grad_inst.hip): d loss / d
// pred from the loss program, the weight handed to it.  One build per tangent width, at sr_grad_param_rows
// rows per lane (the plain kernel's preferred count); hipErrorInvalidValue for any other.
template <typename T, bool GATHER>
hipError_t sr_launch_grad_lossx_any(const SrGradArgs<T>& a, const SrLossProgArgs<T>& x, int kt, int rows, int n_blocks,
                                    hipStream_t s);
// The per-row build of the gradient kernel (sr_grad_rows_kernel: sr_eval_grad_tree_array,
// sr_eval_diff_tree_array).  Item i stores tangent k0 + q (q < item_nq[i]) of row r at
// out[item_out[i] + q * n_rows + r]; bad[row block][item] is 1 when a stored tangent was not finite.
template <typename T>
struct SrGradRowArgs {
  T* out;
  const uint64_t* item_out;   // [n_items]
  const uint32_t* item_nq;    // [n_items] the window's tangents that are the tree's (<= KT)
  uint32_t* bad;              // [n_row_blocks][n_items]
  int feat;                   // 0: the constants' tangents; 1: the features' (k0 counts features)
};
// rows: as sr_launch_grad_any's (sr_grad_launch_rows with weighted = false: y and w are not staged, the
// tile keeps y's place)
template <typename T, bool GATHER>
hipError_t sr_launch_grad_rows_any(const SrGradArgs<T>& a, const SrGradRowArgs<T>& d, int kt, int rows, int n_blocks,
                                   hipStream_t s);
// The reference's loss fold in row order for listed trees (sr_fold.h; sr_aux.hip): predictions
// pred[b][pred_ld] of n rows, losses against y (and w) at row_idx (or the row itself).
// sr_launch_fold_segsum: per segment of seg_len rows, segsum[b][seg] = the f64 sum of its losses;
// sr_launch_fold_segtab: the segment's composed steps tq / tab for the binades around the f64 prefix
// (carry_est[b]: the f64 sum of the rows before this shard, or NULL).
template <typename T>
hipError_t sr_launch_fold_segsum(const T* pred, int64_t pred_ld, int n_trees, const T* y, const T* w,
                                 const int64_t* row_idx, int64_t n, int loss_kind, T loss_param, int64_t seg_len,
                                 double* segsum, hipStream_t s);
template <typename T>
hipError_t sr_launch_fold_segtab(const T* pred, int64_t pred_ld, int n_trees, const T* y, const T* w,
                                 const int64_t* row_idx, int64_t n, int loss_kind, T loss_param, int64_t seg_len,
                                 const double* segsum, const double* carry_est, int2* tq, int64_t* tab, hipStream_t s);
// Every complete tree's fold (round 6; sr_aux.hip): the plan of a large call (codes per (row block,
// position), slots for the FOLD mode's slow segments), the stored-loss tables of a small call, and the
// walk (per position: the fold's value and status at the caller's tree index perm[position]).
struct SrFoldWho;  // (sr_fold_dev.h)
// a region's plan arrays, [row block][position] each: codes, composed-step pairs (steps segments; a slow
// segment's under its lower window binade sq), sq (slow segments; SR_FCODE_SKIP: none), and a slow
// segment's pair under sq + 1
struct SrFoldTabs {
  int32_t* code;
  void* tab;
  int32_t* sq;
  void* tab2;
};
template <typename T>
hipError_t sr_launch_fold_plan(const double* part, int np, int n_rb, const uint32_t* perm, const SrFoldWho& who,
                               double delta, SrFoldTabs ft, int* slot_next, int slot_cap, const int4* cand,
                               hipStream_t s);
// The compacted FOLD launch's lists from a region's plan (SrEvalArgs::fold_list / fold_cnt / fold_wg0; G:
// the launch's trees per workgroup): list [n_rb][np], cnt [n_rb], wg0 [n_rb + 2].  target_wgs > 0: the list's
// entries per workgroup g is the smallest that keeps the launch within target_wgs live workgroups and within
// grid_wgs, the launch's grid (sr_plan.h, sr_fold_list_g); 0: g = G.
hipError_t sr_launch_fold_compact(const SrFoldTabs& ft, int np, int n_rb, int G, int target_wgs, int grid_wgs,
                                  int32_t* list, int32_t* cnt, int32_t* wg0, hipStream_t s);
template <typename T>
hipError_t sr_launch_fold_stab(const double* part, int np, int n_rb, int64_t rb_rows, int64_t n, const uint32_t* perm,
                               const SrFoldWho& who, double delta, const T* losses, SrFoldTabs ft,
                               const uint32_t* part_flag, const uint8_t* static_bad, double* red_sum,
                               uint32_t* red_flag, hipStream_t s);
template <typename T>
hipError_t sr_launch_fold_walk(SrFoldTabs ft, const SrFoldWho& who, int np, int n_rb, int64_t rb_rows, int64_t n,
                               const T* losses, int64_t slot_rows, const uint32_t* perm, const T* carry, T* out_val,
                               int32_t* out_st, void* dbg, int all_rows, hipStream_t s);
template <typename T>
hipError_t sr_launch_fold(const T* pred, int64_t pred_ld, int n_trees, const T* y, const T* w, const int64_t* row_idx,
                          int64_t n, int loss_kind, T loss_param, int64_t seg_len, const int2* tq, const int64_t* tab,
                          const T* carry, T* out, int* n_slow, hipStream_t s);
