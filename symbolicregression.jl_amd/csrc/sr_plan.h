// sr_plan.h — the host-only launch plan of a batched scoring call (sr_capi.cpp's batch engine): the
// launch-shape functions of the tile kernels, the work decomposition (Grid / GridSpec), the tree chunks,
// the derived-column choice, a chunk's launch order, code layout and view segments, and the in-order
// fold's path decision.  Integer arithmetic on host arrays: no HIP, so tools/plan_check.cpp checks it on
// any machine (`make plan-check`).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "sr_compile.h"
#include "../../include/sr_amd.h"

// SR_MODE_FOLD (round 6): the loss programs of complete trees again, composing each row tile's steps of
// the reference's in-order loss fold for the binades of the call's fold plan (sr_fold_dev.h), no checks
enum { SR_MODE_LOSS = 0, SR_MODE_PRED = 1, SR_MODE_EXACT = 2, SR_MODE_FOLD = 3 };
// operand-stack slots the register-stack kernels hold in VGPRs (1: trees needing a second slot —
// 6 % of C2's — run on the LDS-stack kernel instead)
#ifndef SR_VSTK_SLOTS
#define SR_VSTK_SLOTS 2
#endif
enum { SR_TIER_BASIC = 0, SR_TIER_FULL = 1 };
// a flag on the tile kernel's tier template argument: the build for parametric calls (sr_tile_impl.h)
enum { SR_TIER_PARAM = 2 };
// another flag there: the loss build that also composes each row block's in-order fold steps under
// candidate binades (SrEvalArgs::fold_cand; Float32, BASIC, register stack, 16 rows per lane only)
enum { SR_TIER_CAND = 4 };

// One row view's launch positions in a several-view launch (sr_eval_loss_batch_views): positions
// [pos0, pos0 + n_pos) in tree groups of trees_per_block, blocks [block0, block0 + groups x row blocks),
// rows row_idx[row_off .. row_off + n_rows).
struct SrSegment {
  int block0, pos0, n_pos, groups;
  int64_t row_off;
};

// Derived columns of a call (LOAD_DERIVED): column k = op[k](X[feat[k]]) over the view's rows.
constexpr int SR_MAX_DERIVED = 32;
struct SrDerivedSpec {
  int n;
  uint8_t op[SR_MAX_DERIVED];
  uint16_t feat[SR_MAX_DERIVED];  // 0-based feature
};

// ---------------------------------------------------------------- launch shapes of the tile kernels
// Rows per lane of each instantiated kernel (sr_builds.h): f32 BASIC 8 (4 for tuning), f32 FULL 4,
// f64 BASIC 4, f64 FULL 2.  `rows_per_lane` <= 0 picks the default.
template <typename T>
inline int sr_rows_per_lane(int mode, int tier, int requested) {
  const bool basic = mode == SR_MODE_LOSS && tier == SR_TIER_BASIC;
  if (sizeof(T) == 4) {
    if (basic) return (requested == 4 || requested == 16) ? requested : 8;
    return 4;
  }
  return basic ? 4 : 2;
}

// LDS bytes one workgroup (W waves) of the tile kernel needs.
inline size_t sr_tile_lds_bytes(int elem_size, int nf, int rows_per_lane, int stack_depth, int trees_per_block,
                                int max_checks, int waves, bool weighted, int code_lds = 0) {
  // = SrLdsPlan (sr_tile_impl.h): X tile, y (+ w), LDS stack, EXACT checked values + running sums,
  // program cache (16-byte instructions)
  const size_t rows = size_t(64) * rows_per_lane;
  return size_t(nf) * rows * elem_size + (weighted ? 2 : 1) * rows * elem_size +
         size_t(waves) * stack_depth * rows * elem_size + size_t(waves) * size_t(max_checks) * rows * elem_size +
         (size_t(trees_per_block) * size_t(max_checks) * elem_size + 15) / 16 * 16 + size_t(code_lds) * 16;
}

// Waves per workgroup: the f32 BASIC loss kernel has 4- and 8-wave (L2) builds (SR_AMD_WAVES selects);
// every other kernel runs 4 waves.
inline int sr_waves_per_block(int elem_size, int mode, int tier, int rows_per_lane, int requested) {
  if (elem_size == 4 && mode == SR_MODE_LOSS && tier == SR_TIER_BASIC && rows_per_lane == 8 && requested == 8)
    return 8;
  return 4;
}

// Register-stack kernels (f32 BASIC loss over the full dataset, operand stack in VGPRs): rows per
// lane for a view of n rows, or 0 when the classic LDS-stack kernel should run.  Larger tiles halve
// the per-tree epilogues and dispatches per row and, with no LDS stack, keep the workgroup's LDS at
// the X tile (C2 kernel -5 %, its complete trees -12 %, arithmetic-only -18 %); below
// 2^17 rows the padding and the loss of parallelism cost more.  requested: SR_AMD_ROWS_PER_LANE
// (16 / 32 force a register-stack kernel, 4 / 8 the classic one; f64: 8 selects its register-stack
// build).
#ifndef SR_VSTK_DEFAULT_ROWS
#define SR_VSTK_DEFAULT_ROWS 16
#endif
inline int sr_vstk_rows(int elem_size, int64_t n_rows, int requested) {
  // f64: the 8-rows/lane register-stack build (181 VGPRs, 2 waves per SIMD) against the classic
  // 4-rows/lane build (100, 5 waves): round 2 measured it 3 % slower; with the launch order dealt over
  // tree groups it is faster (C2 in f64 13.45 -> 12.69 ms per step, arithmetic-only -19 %,
  // profiles/r03_ab_f64_vstk.txt), so it is the default for large views too
  if (elem_size == 8) {
    if (requested == 8 || requested == -4) return requested == 8 ? 8 : 4;  // (-4: the 4-row register-stack build)
    if (requested == 4 || requested == 2) return 0;
    return n_rows >= (int64_t(1) << 17) ? 8 : 0;
  }
  if (requested == 16 || requested == 32) return requested;
  if (requested == 4 || requested == 8) return 0;
  return n_rows >= (int64_t(1) << 17) ? SR_VSTK_DEFAULT_ROWS : 0;
}

// ---------------------------------------------------------------- work decomposition
// Row tiles of 64*R rows (one LDS image each), `tiles` per block; trees grouped G per block (the
// block's 4 waves share the G trees of a tile).
struct Grid {
  int G = 32, tiles = 1, n_row_blocks = 1, n_groups = 1, R = 8, W = 4;
  int64_t n_blocks = 1;
  size_t lds = 0;
  int64_t rb_rows() const { return int64_t(tiles) * 64 * R; }  // rows of one row block
};
constexpr size_t kLdsMax = 160 * 1024;
inline Grid make_grid(int elem_size, int64_t n_rows, int64_t n_trees, int R, int W, int nf, int depth, int max_checks,
                      bool weighted, int g_override = 0, int64_t max_row_blocks = 256) {
  const int64_t rows_per_tile = 64 * int64_t(R);
  Grid g;
  g.R = R;
  g.W = W;
  const int64_t n_tiles = (n_rows + rows_per_tile - 1) / rows_per_tile;
  int64_t tiles = (n_tiles + max_row_blocks - 1) / max_row_blocks;  // keep <= max row blocks per tree
  if (tiles < 1) tiles = 1;
  g.tiles = int(tiles);
  g.n_row_blocks = int((n_tiles + tiles - 1) / tiles);
  if (g.n_row_blocks < 1) g.n_row_blocks = 1;
  // more trees per tile amortise the tile's LDS staging and barriers (G 16 -> 128: -29% kernel time
  // on the C2 population); shrink only to keep >= 4096 workgroups for small populations
  int G = 128;
  while (G > 4 && int64_t(g.n_row_blocks) * ((n_trees + G - 1) / G) < 4096) G /= 2;
  if (g_override > 0) G = g_override;
  if (G < W) G = W;  // at least one tree per wave
  if (n_trees > 0 && G > n_trees) G = int(n_trees);
  if (G < 1) G = 1;
  g.G = G;
  g.n_groups = int((n_trees + G - 1) / G);
  g.n_blocks = int64_t(g.n_row_blocks) * g.n_groups;
  g.lds = sr_tile_lds_bytes(elem_size, nf, R, depth, G, max_checks, W, weighted);
  return g;
}

// What every grid of one call shares: built once per call, so that the fold-path choice, the launch-order
// deal, the view segments and the launch compute the same grid for the same launch.
struct GridSpec {
  int elem_size = 4;
  int64_t n_rows = 0;   // rows of the view
  int W = 4;            // waves per workgroup
  int nfk = 0;          // X rows a launch stages (a parametric call's hidden class row included)
  bool weighted = false;
  int tree_group = 0;   // sr_ctx::tree_group override (0: heuristic)
  int64_t max_row_blocks = 256;
  // the grid of n_trees launch positions at R rows per lane and `depth` LDS operand-stack slots
  Grid grid(int64_t n_trees, int R, int depth) const {
    return make_grid(elem_size, n_rows, n_trees, R, W, nfk, depth, 0, weighted, tree_group, max_row_blocks);
  }
  // the same call over another row count and row-block bound (the fold-path choice's largest shard)
  GridSpec over(int64_t rows, int64_t bound) const {
    GridSpec s = *this;
    s.n_rows = rows;
    s.max_row_blocks = bound;
    return s;
  }
};

// ---------------------------------------------------------------- tree chunks
// chunking (SR_AMD_CHUNKS, default 2; LOSS mode only — PRED writes rows by caller tree index).
// Default: a first chunk of 1/6 of the trees runs while the host compiles the rest (exposed compile
// 0.72 -> 0.27 ms on C2, every test population's step faster).  k > 2 equal chunks (>= 2048 trees
// each) alternate over the two streams; they cost kernel time on complete-heavy populations.
constexpr int kMaxChunks = 4;
constexpr int64_t kChunkTrees = 2048;
inline int sr_chunk_count(int64_t nt, int chunks, int first_chunk, int64_t chunk_min, bool multi, int mode) {
  int n_chunks = 1;
  if (multi) {
    // (one chunk: the segments cover the whole launch)
  } else if (mode == SR_MODE_LOSS && chunks == 2) {
    n_chunks = nt / first_chunk >= chunk_min ? 2 : 1;  // the small first chunk holds >= chunk_min trees
  } else if (mode == SR_MODE_LOSS && chunks > 2) {
    const int64_t k = nt / kChunkTrees;
    const int64_t cap = chunks < kMaxChunks ? chunks : kMaxChunks;
    n_chunks = int(k < 1 ? 1 : (k > cap ? cap : k));
  }
  return n_chunks;
}
// first tree of chunk k (k = n_chunks: the tree count).  two chunks: a small first one (1/6) runs while
// the host compiles the rest, so the exposed compile time is the small chunk's; more chunks: equal pieces
inline int64_t sr_chunk_bound(int k, int n_chunks, int64_t nt, int first_chunk) {
  if (k <= 0) return 0;
  if (k >= n_chunks) return nt;
  return n_chunks == 2 ? nt / first_chunk : nt * k / n_chunks;
}
// A call's chunks: bound[k] = first tree of chunk k, bound[n] = the tree count.
struct ChunkPlan {
  int n = 1;
  int64_t bound[kMaxChunks + 1] = {0, 0, 0, 0, 0};
};
// The three-chunk schedule (sr_ctx::tail_chunk; the caller passes tail = 0 for every call but a plain
// single-GPU path-2 call whose loss launch composes candidates: a fold chain — plan, compact, scan, FOLD
// re-run, walk — follows each chunk's loss launch on the chunk's stream): {1 / first_chunk, the rest,
// tail / 12} of the trees (tail 1..6).  The first chunk still hides the compile; the other two loss launches
// share the GPU and end close together, so their chains, which are latency-bound, run side by side
// instead of one chain over 5/6 of the trees alone.  Every chunk holds at least chunk_min trees, else — and
// with tail = 0, or chunks != 2 — the bounds are sr_chunk_count / sr_chunk_bound's exactly.
constexpr int kTailTwelfths = 6;
inline ChunkPlan sr_chunk_plan(int64_t nt, int chunks, int first_chunk, int64_t chunk_min, bool multi, int mode,
                               int tail) {
  ChunkPlan p;
  const int a = tail > 0 ? std::min(tail, kTailTwelfths) : 0;
  if (a > 0 && !multi && mode == SR_MODE_LOSS && chunks == 2 && nt > 0) {
    const int64_t lo = std::max<int64_t>(chunk_min, 1);
    const int64_t first = nt / first_chunk, last = nt * a / 12;
    if (first >= lo && last >= lo && nt - first - last >= lo) {
      p.n = 3;
      p.bound[1] = first;
      p.bound[2] = nt - last;
      p.bound[3] = nt;
      return p;
    }
  }
  p.n = sr_chunk_count(nt, chunks, first_chunk, chunk_min, multi, mode);
  for (int k = 0; k <= p.n; ++k) p.bound[k] = sr_chunk_bound(k, p.n, nt, first_chunk);
  return p;
}

// ---------------------------------------------------------------- the staging image
// programs + per-tree metadata of a call: ONE device allocation and ONE pinned staging buffer with the
// same layout (code | offsets | static_bad | launch order | ends | view segments), 256-byte aligned parts,
// so a single-chunk call uploads with one DMA.  A program has at most one instruction per node.
inline size_t sr_align256(size_t x) { return (x + 255) & ~size_t(255); }
struct ProgImage {
  size_t code_cap = 0;  // instructions
  size_t o_off = 0, o_bad = 0, o_perm = 0, o_end = 0, o_seg = 0, bytes = 0;  // byte offsets; the whole image
};
inline ProgImage sr_prog_image(int64_t total_nodes, int64_t nt, size_t ins_size, size_t n_seg_cap) {
  ProgImage m;
  m.code_cap = size_t(total_nodes) + 16;
  m.o_off = sr_align256(m.code_cap * ins_size);
  m.o_bad = sr_align256(m.o_off + (size_t(nt) + 1) * sizeof(uint32_t));
  m.o_perm = sr_align256(m.o_bad + size_t(nt) + 16);
  m.o_end = sr_align256(m.o_perm + (size_t(nt) + 1) * sizeof(uint32_t));
  m.o_seg = sr_align256(m.o_end + (size_t(nt) + 1) * sizeof(uint32_t));
  m.bytes = m.o_seg + n_seg_cap * sizeof(SrSegment);
  return m;
}

// ---------------------------------------------------------------- derived columns
// Derived columns of a LOSS call: the unary(feature) nodes of the batch's transcendental operators
// (exp / cos / sin / safe_log / safe_sqrt) that at least kDerivedMinUses trees of a sample share,
// most used first, at most SR_MAX_DERIVED.  dmap: [SR_U_COUNT][nf] -> column or -1.
constexpr int64_t kDerivedMinRows = 16384;  // below this the per-call column pass does not pay
constexpr int kDerivedMinUses = 4;
constexpr double kDerivedMinWork = 33554432.0;  // trees x rows (2^25) below which the column pass does not pay
constexpr int64_t kDerivedSample = 1024;    // trees scanned
inline void choose_derived(const sr_tree_batch& trees, const SrOpset& ops, int64_t nf, SrDerivedSpec* spec,
                           std::vector<int16_t>* dmap) {
  spec->n = 0;
  dmap->assign(size_t(SR_U_COUNT) * size_t(nf), int16_t(-1));
  auto eligible = [](uint32_t u) {
    return u == SR_U_EXP || u == SR_U_COS || u == SR_U_SIN || u == SR_U_LOG || u == SR_U_SQRT;
  };
  std::vector<int32_t> uses(size_t(SR_U_COUNT) * size_t(nf), 0);
  const int64_t ns = trees.n_trees < kDerivedSample ? trees.n_trees : kDerivedSample;
  for (int64_t k = 0; k < ns; ++k) {
    const int64_t b = trees.offsets[k], e = trees.offsets[k + 1];
    // pre-order: node i (degree 1) has its child at i + 1
    for (int64_t i = b; i + 1 < e; ++i) {
      if (trees.degree[i] != 1 || trees.degree[i + 1] != 0 || trees.constant[i + 1]) continue;
      const int oi = int(trees.op[i]) - 1;
      const int f = int(trees.feature[i + 1]) - 1;
      if (oi < 0 || oi >= int(ops.unary.size()) || f < 0 || f >= nf) continue;
      const uint32_t u = ops.unary[size_t(oi)];
      if (eligible(u)) ++uses[size_t(u) * size_t(nf) + size_t(f)];
    }
  }
  std::vector<std::pair<int32_t, size_t>> cand;
  for (size_t q = 0; q < uses.size(); ++q)
    if (uses[q] >= kDerivedMinUses) cand.push_back({uses[q], q});
  std::stable_sort(cand.begin(), cand.end(), [](const auto& x, const auto& y) { return x.first > y.first; });
  for (const auto& c : cand) {
    if (spec->n >= SR_MAX_DERIVED) break;
    const int k = spec->n++;
    spec->op[k] = uint8_t(c.second / size_t(nf));
    spec->feat[k] = uint16_t(c.second % size_t(nf));
    (*dmap)[c.second] = int16_t(k);
  }
}

// ---------------------------------------------------------------- a chunk's launch order
// Trees whose programs fit the register stack (<= 2 slots: every tree of < 23 nodes, most of the
// rest) run on the register-stack kernel; the few deeper ones follow in a second launch of the
// LDS-stack kernel over the tail of the launch order.  Returns the count of the former (0 with the
// register stack off): launch positions [0, n_vs) -> register-stack kernel.
inline int64_t sr_count_vstk(const uint8_t* depth, int64_t nc, bool vstk) {
  int64_t n_vs = 0;
  if (vstk)
    for (int64_t i = 0; i < nc; ++i) n_vs += depth[i] <= SR_VSTK_SLOTS ? 1 : 0;
  return n_vs;
}
// launch order: register-stack trees first, each class in decreasing estimated cost so every
// block's waves get similar work (counting sort: costs are small integers; ties keep order).
// several views (tree_view non-NULL, the chunk's trees): the view first (each view's trees contiguous:
// its own segment of tree groups)
inline void sr_cost_sort(const uint32_t* cost, const uint8_t* depth, int64_t nc, const int32_t* tree_view, int n_views,
                         bool sort, bool vstk, uint32_t* perm) {
  uint32_t cmax = 0;
  if (sort)
    for (int64_t i = 0; i < nc; ++i) cmax = cost[i] > cmax ? cost[i] : cmax;
  const size_t nkey = size_t(cmax) + 1;
  const size_t n_cls = tree_view ? size_t(n_views) : 2;
  std::vector<uint32_t> start(n_cls * nkey + 1, 0);
  auto key = [&](int64_t i) -> size_t {
    const size_t cls = tree_view ? size_t(tree_view[i]) : ((vstk && depth[i] > SR_VSTK_SLOTS) ? 1 : 0);
    return cls * nkey + (sort ? size_t(cmax - cost[i]) : 0);
  };
  for (int64_t i = 0; i < nc; ++i) ++start[key(i) + 1];
  for (size_t k = 1; k < start.size(); ++k) start[k] += start[k - 1];
  for (int64_t i = 0; i < nc; ++i) perm[start[key(i)]++] = uint32_t(i);
}
// Deal the cost-ordered trees of each class round-robin over that launch's tree groups (group
// g takes ranks g, g + n_groups, ...; each group's positions stay in decreasing cost, so its
// waves still get equal work).  Contiguous cost ranks made the first groups' workgroups several
// times longer than the last groups' and the launch ended on a tail of heavy workgroups (C2's
// complete trees: 4.36 ms with contiguous groups of 128, 3.32 unsorted).
// perm: the launch's np positions, ranked by cost; G, n_groups: its grid's.
inline void sr_deal_groups(uint32_t* perm, int64_t np, int64_t G, int64_t ng) {
  if (np <= 1 || ng <= 1) return;
  std::vector<uint32_t> ranked(perm, perm + np);
  int64_t k = 0;
  for (int64_t j = 0; j < G; ++j)
    for (int64_t gi = 0; gi < ng; ++gi) {
      const int64_t size = gi + 1 < ng ? G : np - (ng - 1) * G;
      if (j < size) perm[gi * G + j] = ranked[size_t(k++)];
    }
}
// A launch's tree groups, as the deal needs them (Grid::G, Grid::n_groups).
struct GroupShape {
  int64_t G = 1, n_groups = 1;
};
// The chunk's whole order: sort, then (sort && balance, one view) the deal of each class over its
// launch's groups — vs: the register-stack launch's grid over sr_count_vstk positions, ls: the LDS-stack
// launch's over the rest.  Writes perm[0, nc) and returns n_vs.
inline int64_t sr_launch_order(const uint32_t* cost, const uint8_t* depth, int64_t nc, const int32_t* tree_view,
                               int n_views, bool sort, bool balance, bool vstk, GroupShape vs, GroupShape ls,
                               uint32_t* perm) {
  const int64_t n_vs = sr_count_vstk(depth, nc, vstk);
  sort = sort && nc > 1;
  sr_cost_sort(cost, depth, nc, tree_view, n_views, sort, vstk, perm);
  if (sort && balance && !tree_view) {
    if (n_vs > 0) sr_deal_groups(perm, n_vs, vs.G, vs.n_groups);
    if (n_vs < nc) sr_deal_groups(perm + n_vs, nc - n_vs, ls.G, ls.n_groups);
  }
  return n_vs;
}

// ---------------------------------------------------------------- code layout, segments, group spans
// programs in launch order: a tree group's code is one contiguous span (the kernel's LDS program
// cache copies it in one pass); offsets / ends stay indexed by tree.  prog_off: [nc + 1] the compiled
// chunk's offsets; destinations: a prefix over the launch order from code_base.  Returns the end.
inline uint32_t sr_code_layout(const uint32_t* perm, const uint32_t* prog_off, int64_t nc, uint32_t code_base,
                               uint32_t* off, uint32_t* end) {
  uint32_t at = code_base;
  for (int64_t p = 0; p < nc; ++p) {
    const uint32_t i = perm[p];
    const uint32_t len = prog_off[size_t(i) + 1] - prog_off[size_t(i)];
    off[i] = at;
    end[i] = at + len;
    at += len;
  }
  return at;
}
// several views: one segment per view present (launch positions in view order), tree groups of the
// launch's G, blocks in segment order.  Fills segs (at most one per view) and *n_seg; returns the blocks.
inline int64_t sr_view_segments(const int32_t* tree_view, const uint32_t* perm, int64_t nc, int G, int n_row_blocks,
                                int64_t n_idx, SrSegment* segs, int* n_seg) {
  int64_t seg_blocks = 0;
  *n_seg = 0;
  for (int64_t p = 0; p < nc;) {
    const int v = tree_view[perm[p]];
    int64_t q = p;
    while (q < nc && tree_view[perm[q]] == v) ++q;
    SrSegment sg{};
    sg.block0 = int(seg_blocks);
    sg.pos0 = int(p);
    sg.n_pos = int(q - p);
    sg.groups = int((q - p + G - 1) / G);
    sg.row_off = int64_t(v) * n_idx;
    segs[(*n_seg)++] = sg;
    seg_blocks += int64_t(sg.groups) * n_row_blocks;
    p = q;
  }
  return seg_blocks;
}
// the longest code span of a tree group of the launch over positions [p0, p0 + np) (the LDS program cache
// is sized for it)
inline int64_t sr_max_group_span(const uint32_t* perm, const uint32_t* off, const uint32_t* end, int64_t p0,
                                 int64_t np, int G, int n_groups) {
  int64_t maxspan = 0;
  for (int64_t q = 0; q < n_groups; ++q) {
    const int64_t pf = p0 + q * G, pl = std::min<int64_t>(p0 + np, pf + G) - 1;
    const int64_t sp = int64_t(end[perm[pl]]) - int64_t(off[perm[pf]]);
    maxspan = std::max(maxspan, sp);
  }
  return maxspan;
}

// ---------------------------------------------------------------- the in-order fold's path
// rows of the largest shard of a row-sharded call (offs: sr_dataset::shard_offs), at least n_eval
inline int64_t sr_max_shard_rows(const std::vector<int64_t>& offs, int64_t n_eval) {
  int64_t m = n_eval;
  for (size_t r = 0; r + 1 < offs.size(); ++r) m = std::max(m, offs[r + 1] - offs[r]);
  return m;
}
struct FoldPlanIn {
  int64_t nt = 0, n_eval = 0;  // trees, the view's rows
  int64_t max_shard = 0;       // the largest shard's rows (one GPU: n_eval)
  int64_t fold_len = 0;        // the fold's total length (a row-sharded call: the global rows)
  int elem_size = 4, tier = 0, R = 8, Rv = 0;
  int64_t fold_store_mb = 0, fold_slot_mb = 0, fold_seg_max = 0, fold_rows_max = 0;  // sr_ctx's knobs
  Grid g_ls, g_vs;  // the call's grids at R rows per lane (depth 1) and, Rv > 0, at Rv (depth 0), nt trees
  Grid g_big;       // the grid over the largest shard's rows, bound max(512, rows / fold_seg_max)
};
struct FoldPlan {
  int path = 0;  // 0 none, 1 = the loss launch stores every tree's losses, 2 = the FOLD-mode pass
  int64_t pos_rows = 0;     // rows a position's store covers under either kernel's grid (>= the view)
  int64_t slot_rows = 0;    // rows of a slot (path 2; the longer row block of the two kernels)
  int64_t slot_budget = 0;  // path 2: the slots fold_slot_mb allows
  int64_t slots = 0;        // path 2: the slots to allocate
};
// The reference's in-order loss fold of every complete tree (sr_ctx::ref_fold): 1 = the loss launch
// stores every tree's losses (they fit fold_store_mb), 2 = the FOLD-mode pass over the complete trees.
// Decides only; the caller allocates from the result.
inline FoldPlan sr_fold_plan(const FoldPlanIn& in) {
  FoldPlan out;
  const int64_t rbr = in.g_ls.rb_rows(), rbv = in.Rv > 0 ? in.g_vs.rb_rows() : 0;
  int64_t pos_rows = int64_t(in.g_ls.n_row_blocks) * rbr;
  if (in.Rv > 0) pos_rows = std::max(pos_rows, int64_t(in.g_vs.n_row_blocks) * rbv);
  out.pos_rows = pos_rows;
  out.slot_rows = std::max(rbr, rbv);
  const bool fold_mode_builds = in.tier == SR_TIER_BASIC ? (in.R == 8 && (in.Rv == 0 || in.Rv == 16)) : in.R == 4;
  // Float64: only with stored losses (no FOLD build), decided on the largest shard so every rank agrees
  const bool f64_off = in.elem_size == 8 && double(in.nt) * double(pos_rows) * double(in.max_shard) / double(in.n_eval) *
                                                    double(in.elem_size) > double(in.fold_store_mb) * 1048576.0;
  // segments (row blocks) past fold_seg_max rows on the largest shard: no fold (a slow segment's rows
  // are kept whole).  The launch already takes enough row blocks for fold_seg_max (up to 16,384
  // blocks); decided on that grid whatever max_row_blocks says, so the knob never changes a result.
  const int64_t rb_big = in.g_big.rb_rows();
  // folds longer than fold_rows_max (2^24) keep the f64 sum: past ~2^23 rows the reference's Float32
  // fold stalls (a loss below half an ulp of the running sum adds nothing; C4's 2^26 rows: up to 50 %
  // below the exact mean) and drifts out of every window the f64 prefix gives the plan, so the walks
  // fail and the fallback's prediction pass takes the call (C4 folded: 26.6k trees, 37.7 s a step)
  if (f64_off || rb_big > in.fold_seg_max || in.fold_len > in.fold_rows_max) {
  } else if (double(in.nt) * double(pos_rows) * double(in.elem_size) <= double(in.fold_store_mb) * 1048576.0) {
    out.path = 1;
  } else if (in.elem_size == 4 && fold_mode_builds) {
    out.path = 2;
    // (slots for ~24 slow segments per tree — C2 averages 10; a handful of trees over many row blocks
    //  can need more each: at least 1,024 — up to fold_slot_mb, which caps the call's slots whatever an
    //  earlier call left allocated: the buffer only ever grows)
    out.slot_budget = std::max<int64_t>(1, in.fold_slot_mb * 1048576 / (out.slot_rows * int64_t(in.elem_size)));
    out.slots = std::min<int64_t>(std::max<int64_t>(int64_t(in.nt) * 24, 1024), out.slot_budget);
  }
  return out;
}
// The compacted FOLD launch (sr_ctx::fold_compact): a call has at most two launches per chunk (register
// stack, LDS stack), each with its own counters {cnt [n_rb] | wg0 [n_rb + 1] | g}; region r's start, in words,
// for a call of n_rb row blocks per position, and the call's words.
inline int sr_fold_region(int chunk, bool vstk) { return 2 * chunk + (vstk ? 0 : 1); }
inline size_t sr_fold_wg_off(int region, int64_t n_rb) { return size_t(region) * (2 * size_t(n_rb) + 2); }
inline size_t sr_fold_wg_words(int64_t n_rb) { return sr_fold_wg_off(2 * kMaxChunks, n_rb); }
// The entries per workgroup g of a compacted FOLD launch (sr_ctx::fold_list_wgs), from its row blocks' counts:
// the live workgroups are the sum of ceil(cnt[rb] / g).  target 0: G, the launch's trees per workgroup.  Else
// the smallest multiple of the 4 waves, at least 4 and at most G, whose workgroups stay within the target and
// within the launch's grid; G when none does (the grid is the region's groups x row blocks: G always fits it).
// The host's statement of sr_fold_compact_scan_kernel's rule, which finds the same g by bisection (the sum
// does not grow with g); region r keeps g in the word after its wg0 [n_rb + 1].
inline int64_t sr_fold_list_wgs(const int32_t* cnt, int n_rb, int g) {
  int64_t s = 0;
  for (int r = 0; r < n_rb; ++r) s += (int64_t(cnt[r]) + g - 1) / g;
  return s;
}
inline int sr_fold_list_g(const int32_t* cnt, int n_rb, int G, int64_t target, int64_t grid) {
  if (target <= 0 || G < 4) return G;
  const int64_t lim = std::min(target, grid);
  for (int g = 4; g <= G; g += 4)
    if (sr_fold_list_wgs(cnt, n_rb, g) <= lim) return g;
  return G;
}
constexpr int64_t kFoldListWgsMax = int64_t(1) << 24;  // (the knob's bound: past any grid's workgroups)
// The listed loss launch (sr_ctx::loss_compact): one buffer for the call, {list int32 [nt] | cnt int32
// [kMaxChunks][kLossListCnt] | excl uint8 [nt]} — a chunk's register-stack region (its only listed launch)
// uses the slices at its first launch position and the counters of its chunk {listed, entries per workgroup,
// workgroups per row block, -}; byte offsets and the call's bytes.
constexpr int kLossListCnt = 4;
inline size_t sr_loss_list_cnt_off(int64_t nt) { return size_t(nt) * sizeof(int32_t); }
inline size_t sr_loss_list_excl_off(int64_t nt) {
  return sr_loss_list_cnt_off(nt) + size_t(kMaxChunks) * kLossListCnt * sizeof(int32_t);
}
inline size_t sr_loss_list_bytes(int64_t nt) { return sr_loss_list_excl_off(nt) + size_t(nt); }
