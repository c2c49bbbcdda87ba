// plan_check.cpp — stand-alone host check of the batch engine's launch plan (csrc/sr_plan.h; no GPU, no
// HIP, no Python).
//
// Build and run through `make -C symbolicregression.jl_amd plan-check`, which compiles this file with
// -fsanitize=address,undefined.  It checks the grids (values derived by hand from make_grid, and its
// invariants over a sweep), the chunk bounds (the two-chunk pipeline and the three-chunk schedule), a chunk's launch order (counting sort, the deal over tree
// groups, views), the code layout, the view segments, the longest group span and the in-order fold's path
// decision.  Exit status 0 and "plan_check: ok" on success.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../symbolicregression.jl_amd/csrc/sr_plan.h"

namespace {

int g_failed = 0;
#define CHECK(cond)                                                         \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::fprintf(stderr, "plan_check: %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      if (++g_failed > 20) std::exit(1);                                    \
    }                                                                       \
  } while (0)

struct Rng {
  uint64_t s;
  uint32_t next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return uint32_t(s >> 33);
  }
  int below(int n) { return int(next() % uint32_t(n)); }
};

GridSpec spec(int elem_size, int64_t rows, int W, int64_t bound, int tree_group = 0) {
  GridSpec s;
  s.elem_size = elem_size;
  s.n_rows = rows;
  s.W = W;
  s.nfk = 5;
  s.weighted = false;
  s.tree_group = tree_group;
  s.max_row_blocks = bound;
  return s;
}

void check_grids() {
  {  // 1024 tiles of 1024 rows, two per block; 128 trees per group keep 512 x 79 >= 4096 workgroups
    const Grid g = spec(4, int64_t(1) << 20, 4, 512).grid(10000, 16, 0);
    CHECK(g.tiles == 2 && g.n_row_blocks == 512 && g.G == 128 && g.n_groups == 79 && g.n_blocks == 40448);
    CHECK(g.R == 16 && g.W == 4 && g.rb_rows() == 2048);
    CHECK(g.lds == sr_tile_lds_bytes(4, 5, 16, 0, 128, 0, 4, false));
    CHECK(g.lds == size_t(5 + 1) * 1024 * 4);
  }
  {  // one tile: G halves down to 4
    const Grid g = spec(4, 100, 4, 512).grid(50, 8, 1);
    CHECK(g.tiles == 1 && g.n_row_blocks == 1 && g.G == 4 && g.n_groups == 13 && g.n_blocks == 13);
  }
  CHECK(spec(4, 100, 4, 512, 32).grid(20, 8, 1).G == 20);
  CHECK(spec(4, 100, 4, 512, 32).grid(100, 8, 1).G == 32);
  for (int R : {8, 16})
    for (int W : {4, 8})
      for (int64_t rows : {int64_t(1), int64_t(63), int64_t(64) * R, int64_t(64) * R + 1, int64_t(1) << 17,
                           (int64_t(1) << 20) + 5})
        for (int64_t trees : {1, 3, 127, 129, 5000})
          for (int64_t bound : {1, 16, 512, 4096}) {
            const Grid g = spec(4, rows, W, bound).grid(trees, R, 1);
            const int64_t tile = 64 * int64_t(R);
            CHECK(g.n_row_blocks >= 1 && g.tiles >= 1 && g.n_row_blocks <= bound);
            CHECK(int64_t(g.tiles) * g.n_row_blocks * tile >= rows);
            CHECK(int64_t(g.n_row_blocks - 1) * g.tiles * tile < rows);
            CHECK(g.G >= 1 && (W <= g.G || trees < W));
            CHECK(int64_t(g.n_groups) * g.G >= trees && trees > int64_t(g.n_groups - 1) * g.G);
            CHECK(g.n_blocks == int64_t(g.n_row_blocks) * g.n_groups);
          }
  // another row count and bound over the same call (the fold-path choice's grid)
  const GridSpec s = spec(4, 1000, 4, 512);
  const GridSpec o = s.over(int64_t(1) << 20, 1049);
  CHECK(o.n_rows == (int64_t(1) << 20) && o.max_row_blocks == 1049 && o.W == s.W && o.nfk == s.nfk);
  // the launch shapes
  CHECK(sr_rows_per_lane<float>(SR_MODE_LOSS, SR_TIER_BASIC, 0) == 8 && sr_rows_per_lane<float>(SR_MODE_LOSS, SR_TIER_BASIC, 16) == 16);
  CHECK(sr_rows_per_lane<float>(SR_MODE_PRED, SR_TIER_BASIC, 16) == 4 && sr_rows_per_lane<double>(SR_MODE_LOSS, SR_TIER_BASIC, 0) == 4);
  CHECK(sr_rows_per_lane<double>(SR_MODE_LOSS, SR_TIER_FULL, 0) == 2);
  CHECK(sr_waves_per_block(4, SR_MODE_LOSS, SR_TIER_BASIC, 8, 8) == 8 && sr_waves_per_block(8, SR_MODE_LOSS, SR_TIER_BASIC, 8, 8) == 4);
  CHECK(sr_vstk_rows(4, int64_t(1) << 17, 0) == SR_VSTK_DEFAULT_ROWS && sr_vstk_rows(4, (int64_t(1) << 17) - 1, 0) == 0);
  CHECK(sr_vstk_rows(4, 100, 32) == 32 && sr_vstk_rows(4, int64_t(1) << 20, 8) == 0 && sr_vstk_rows(8, int64_t(1) << 20, 0) == 8);
  CHECK(sr_vstk_rows(8, 100, -4) == 4 && sr_vstk_rows(8, int64_t(1) << 20, 2) == 0);
}

void check_chunks() {
  CHECK(sr_chunk_count(10000, 2, 6, 1024, false, SR_MODE_LOSS) == 2);
  CHECK(sr_chunk_bound(0, 2, 10000, 6) == 0 && sr_chunk_bound(1, 2, 10000, 6) == 1666 && sr_chunk_bound(2, 2, 10000, 6) == 10000);
  CHECK(sr_chunk_count(6000, 2, 6, 1024, false, SR_MODE_LOSS) == 1);
  CHECK(sr_chunk_bound(0, 1, 6000, 6) == 0 && sr_chunk_bound(1, 1, 6000, 6) == 6000);
  CHECK(sr_chunk_count(10000, 4, 6, 1024, false, SR_MODE_LOSS) == 4);
  for (int k = 0; k <= 4; ++k) CHECK(sr_chunk_bound(k, 4, 10000, 6) == 2500 * k);
  CHECK(sr_chunk_count(3000, 4, 6, 1024, false, SR_MODE_LOSS) == 1);
  CHECK(sr_chunk_count(100000, 8, 6, 1024, false, SR_MODE_LOSS) == kMaxChunks);
  CHECK(sr_chunk_count(10000, 2, 6, 1024, true, SR_MODE_LOSS) == 1);   // several views
  CHECK(sr_chunk_count(10000, 4, 6, 1024, true, SR_MODE_LOSS) == 1);
  CHECK(sr_chunk_count(10000, 2, 6, 1024, false, SR_MODE_PRED) == 1);  // PRED writes rows by caller tree index
  CHECK(sr_chunk_count(10000, 1, 6, 1024, false, SR_MODE_LOSS) == 1);
  // the three-chunk schedule (sr_chunk_plan): C2's 10,000 trees
  {
    const ChunkPlan p = sr_chunk_plan(10000, 2, 6, 1024, false, SR_MODE_LOSS, 4);  // {1/6, 1/2, 1/3}
    CHECK(p.n == 3 && p.bound[0] == 0 && p.bound[1] == 1666 && p.bound[2] == 10000 - 3333 && p.bound[3] == 10000);
    CHECK(sr_chunk_plan(6600, 2, 6, 1024, false, SR_MODE_LOSS, 1).n == 2);   // (a last chunk of 550 < chunk_min)
    CHECK(sr_chunk_plan(1204, 2, 6, 64, false, SR_MODE_LOSS, 4).n == 3);
    CHECK(sr_chunk_plan(1204, 2, 2, 64, false, SR_MODE_LOSS, 6).n == 2);     // (nothing left for the middle chunk)
  }
  // ... over every tree count to a few thousand and every chunk_min / first_chunk / tail_chunk the knobs allow
  // (chunk_min sampled): monotone bounds that cover [0, nt], at most kMaxChunks chunks, none but the only one
  // below chunk_min, the first chunk 1 / first_chunk; and with tail 0 — every call outside the schedule's
  // rule — sr_chunk_count / sr_chunk_bound exactly
  for (int64_t nt = 0; nt <= 3000; nt += (nt < 300 ? 1 : 7))
    for (int first_chunk : {2, 3, 6, 7, 12, 64})
      for (int64_t chunk_min : {int64_t(1), int64_t(2), int64_t(64), int64_t(100), int64_t(1024), int64_t(5000)})
        for (int chunks : {1, 2, 3, 4, 8})
          for (int mode : {int(SR_MODE_LOSS), int(SR_MODE_PRED)})
            for (int multi = 0; multi <= 1; ++multi)
              for (int tail = 0; tail <= kTailTwelfths; ++tail) {
                const ChunkPlan p = sr_chunk_plan(nt, chunks, first_chunk, chunk_min, multi != 0, mode, tail);
                const int n_old = sr_chunk_count(nt, chunks, first_chunk, chunk_min, multi != 0, mode);
                CHECK(p.n >= 1 && p.n <= kMaxChunks && p.bound[0] == 0 && p.bound[p.n] == nt);
                for (int k = 0; k < p.n; ++k) {
                  CHECK(p.bound[k] <= p.bound[k + 1]);
                  if (p.n > 1 && chunks == 2) CHECK(p.bound[k + 1] - p.bound[k] >= chunk_min);
                }
                const bool old = tail == 0 || chunks != 2 || multi || mode != SR_MODE_LOSS || p.n != 3;
                if (old) {
                  CHECK(p.n == n_old);
                  for (int k = 0; k <= p.n; ++k) CHECK(p.bound[k] == sr_chunk_bound(k, n_old, nt, first_chunk));
                } else {
                  CHECK(n_old == 2 && p.bound[1] == nt / first_chunk);  // (the first chunk hides the compile)
                  CHECK(p.bound[3] - p.bound[2] == nt * tail / 12);
                }
              }
  // the staging image: code | offsets | static_bad | order | ends | segments, each part 256-byte aligned
  // and large enough for its array
  for (int64_t nt : {0, 1, 63, 1000})
    for (size_t n_seg : {size_t(0), size_t(7)}) {
      const int64_t nodes = 11 * nt;
      const ProgImage m = sr_prog_image(nodes, nt, 16, n_seg);
      CHECK(m.code_cap >= size_t(nodes) && m.o_off >= m.code_cap * 16);
      CHECK(m.o_bad >= m.o_off + (size_t(nt) + 1) * 4 && m.o_perm >= m.o_bad + size_t(nt));
      CHECK(m.o_end >= m.o_perm + size_t(nt) * 4 && m.o_seg >= m.o_end + size_t(nt) * 4);
      CHECK(m.bytes == m.o_seg + n_seg * sizeof(SrSegment));
      for (size_t o : {m.o_off, m.o_bad, m.o_perm, m.o_end, m.o_seg}) CHECK(o % 256 == 0);
    }
}

bool is_permutation(const std::vector<uint32_t>& perm) {
  std::vector<uint8_t> seen(perm.size(), 0);
  for (uint32_t v : perm) {
    if (v >= perm.size() || seen[v]) return false;
    seen[v] = 1;
  }
  return true;
}

// a launch's tree groups as the engine takes them: from the grid of np positions
GroupShape shape(const GridSpec& gs, int64_t np, int R, int depth) {
  if (np <= 0) return GroupShape{};
  const Grid g = gs.grid(np, R, depth);
  return GroupShape{g.G, g.n_groups};
}

void check_order(Rng& rng, int64_t nc, int tree_group) {
  std::vector<uint32_t> cost(static_cast<size_t>(nc)), prog_off(size_t(nc) + 1, 0);
  std::vector<uint8_t> depth(static_cast<size_t>(nc));
  for (int64_t i = 0; i < nc; ++i) {
    cost[size_t(i)] = uint32_t(1 + rng.below(40));  // (few distinct values: many ties)
    depth[size_t(i)] = uint8_t(1 + rng.below(4));
    prog_off[size_t(i) + 1] = prog_off[size_t(i)] + uint32_t(rng.below(30));  // (empty programs too)
  }
  const GridSpec gs = spec(4, int64_t(1) << 20, 4, 512, tree_group);
  const int Rv = 16, R = 8, dmax = 4;
  for (int vstk = 0; vstk <= 1; ++vstk) {
    const int64_t n_vs_want = sr_count_vstk(depth.data(), nc, vstk != 0);
    const GroupShape vs = shape(gs, n_vs_want, Rv, 0), ls = shape(gs, nc - n_vs_want, R, dmax);
    std::vector<uint32_t> plain(size_t(nc), 0xffffffffu), sorted = plain, dealt = plain;
    // sort off: index order within a class
    int64_t n_vs = sr_launch_order(cost.data(), depth.data(), nc, nullptr, 0, false, true, vstk != 0, vs, ls, plain.data());
    CHECK(n_vs == n_vs_want && is_permutation(plain));
    int64_t want = 0;
    for (int64_t i = 0; i < nc; ++i) want += (vstk && depth[size_t(i)] <= SR_VSTK_SLOTS) ? 1 : 0;
    CHECK(n_vs == want && (vstk || n_vs == 0));
    for (int64_t p = 0; p < nc; ++p) {
      if (vstk) CHECK((depth[plain[size_t(p)]] <= SR_VSTK_SLOTS) == (p < n_vs));
      if (p > 0 && p != n_vs) CHECK(plain[size_t(p - 1)] < plain[size_t(p)]);
    }
    // sorted, no balance: costs non-increasing within each class, ties keep index order
    n_vs = sr_launch_order(cost.data(), depth.data(), nc, nullptr, 0, true, false, vstk != 0, vs, ls, sorted.data());
    CHECK(n_vs == n_vs_want && is_permutation(sorted));
    for (int64_t p = 0; p < nc; ++p) {
      if (vstk) CHECK((depth[sorted[size_t(p)]] <= SR_VSTK_SLOTS) == (p < n_vs));
      if (p > 0 && p != n_vs) {
        const uint32_t a = sorted[size_t(p - 1)], b = sorted[size_t(p)];
        CHECK(cost[a] > cost[b] || (cost[a] == cost[b] && a < b));
      }
    }
    // balance: group g of a class holds the cost ranks g, g + n_groups, ... in that order; once the short
    // last group is full the deal goes on over the other groups (stride n_groups - 1)
    n_vs = sr_launch_order(cost.data(), depth.data(), nc, nullptr, 0, true, true, vstk != 0, vs, ls, dealt.data());
    CHECK(n_vs == n_vs_want && is_permutation(dealt));
    auto check_class = [&](int64_t p0, int64_t np, GroupShape sh) {
      if (np <= 0) return;
      const int64_t G = sh.G, ng = sh.n_groups;
      CHECK(ng * G >= np && np > (ng - 1) * G);
      if (np <= 1 || ng <= 1) {
        for (int64_t p = p0; p < p0 + np; ++p) CHECK(dealt[size_t(p)] == sorted[size_t(p)]);
        return;
      }
      const int64_t last = np - (ng - 1) * G;  // the short group's size
      for (int64_t g = 0; g < ng; ++g)
        for (int64_t j = 0; j < (g + 1 < ng ? G : last); ++j) {
          const int64_t rank = j < last ? j * ng + g : last * ng + (j - last) * (ng - 1) + g;
          CHECK(dealt[size_t(p0 + g * G + j)] == sorted[size_t(p0 + rank)]);
        }
    };
    check_class(0, n_vs, vs);
    check_class(n_vs, nc - n_vs, ls);
    // nc <= 1: nothing to sort
    // code layout: starts and ends tile [code_base, code_base + Σ len) with no gap, in launch order
    const uint32_t code_base = 77;
    std::vector<uint32_t> off(size_t(nc), 0), end(size_t(nc), 0);
    const uint32_t stop = sr_code_layout(dealt.data(), prog_off.data(), nc, code_base, off.data(), end.data());
    CHECK(stop == code_base + prog_off[size_t(nc)]);
    uint32_t at = code_base;
    for (int64_t p = 0; p < nc; ++p) {
      const uint32_t i = dealt[size_t(p)];
      CHECK(off[i] == at && end[i] - off[i] == prog_off[size_t(i) + 1] - prog_off[size_t(i)]);
      at = end[i];
    }
    CHECK(at == stop);
    // the longest group span of each launch against the groups' own sums
    auto check_span = [&](int64_t p0, int64_t np, GroupShape sh) {
      if (np <= 0) return;
      int64_t want_span = 0;
      for (int64_t g = 0; g < sh.n_groups; ++g) {
        int64_t sum = 0;
        for (int64_t p = p0 + g * sh.G; p < std::min(p0 + np, p0 + (g + 1) * sh.G); ++p)
          sum += int64_t(end[dealt[size_t(p)]]) - int64_t(off[dealt[size_t(p)]]);
        want_span = std::max(want_span, sum);
      }
      CHECK(sr_max_group_span(dealt.data(), off.data(), end.data(), p0, np, int(sh.G), int(sh.n_groups)) == want_span);
    };
    check_span(0, n_vs, vs);
    check_span(n_vs, nc - n_vs, ls);
  }
  // several views (a gathered call: no register stack): each view's trees contiguous, views ascending,
  // cost order within a view, never dealt
  const int n_views = 5;
  const int64_t n_idx = 300;
  std::vector<int32_t> view(static_cast<size_t>(nc));
  for (int64_t i = 0; i < nc; ++i) view[size_t(i)] = int32_t(rng.below(n_views) == 3 ? 0 : rng.below(n_views));
  const GridSpec gv = spec(4, n_idx, 4, 512, tree_group);
  const Grid gm = gv.grid(nc, R, dmax);
  for (int sort = 0; sort <= 1; ++sort) {
    std::vector<uint32_t> perm(size_t(nc), 0xffffffffu);
    const int64_t n_vs = sr_launch_order(cost.data(), depth.data(), nc, view.data(), n_views, sort != 0, true, false,
                                         GroupShape{}, GroupShape{gm.G, gm.n_groups}, perm.data());
    CHECK(n_vs == 0 && is_permutation(perm));
    for (int64_t p = 1; p < nc; ++p) {
      const uint32_t a = perm[size_t(p - 1)], b = perm[size_t(p)];
      CHECK(view[a] <= view[b]);
      if (view[a] == view[b]) CHECK(sort ? (cost[a] > cost[b] || (cost[a] == cost[b] && a < b)) : a < b);
    }
    // segments: view-pure, pos0 / n_pos partition the chunk, block0 the running sum of groups x row blocks
    std::vector<SrSegment> segs(static_cast<size_t>(n_views));
    int n_seg = -1;
    const int64_t blocks = sr_view_segments(view.data(), perm.data(), nc, gm.G, gm.n_row_blocks, n_idx, segs.data(), &n_seg);
    CHECK(n_seg >= 1 && n_seg <= n_views);
    int64_t pos = 0, block = 0;
    int last_view = -1;
    for (int k = 0; k < n_seg; ++k) {
      const SrSegment& sg = segs[size_t(k)];
      CHECK(sg.pos0 == pos && sg.n_pos >= 1 && sg.block0 == block);
      const int v = view[perm[size_t(sg.pos0)]];
      CHECK(v > last_view);
      last_view = v;
      for (int64_t p = sg.pos0; p < sg.pos0 + sg.n_pos; ++p) CHECK(view[perm[size_t(p)]] == v);
      CHECK(sg.groups == (sg.n_pos + gm.G - 1) / gm.G);
      CHECK(sg.row_off == int64_t(v) * n_idx);
      pos += sg.n_pos;
      block += int64_t(sg.groups) * gm.n_row_blocks;
    }
    CHECK(pos == nc && block == blocks);
  }
}

FoldPlanIn fold_in(int elem_size, int64_t nt, int64_t n_eval, int64_t max_shard, int64_t fold_len, int R, int Rv) {
  FoldPlanIn in;
  in.nt = nt;
  in.n_eval = n_eval;
  in.max_shard = max_shard;
  in.fold_len = fold_len;
  in.elem_size = elem_size;
  in.tier = SR_TIER_BASIC;
  in.R = R;
  in.Rv = Rv;
  in.fold_store_mb = 512;
  in.fold_slot_mb = 24576;
  in.fold_seg_max = 16384;
  in.fold_rows_max = int64_t(1) << 24;
  return in;
}
// the grids as the engine builds them
void fold_grids(FoldPlanIn* in) {
  const GridSpec gs = spec(in->elem_size, in->n_eval, 4, 512);
  in->g_ls = gs.grid(in->nt, in->R, 1);
  if (in->Rv > 0) in->g_vs = gs.grid(in->nt, in->Rv, 0);
  in->g_big = gs.over(in->max_shard, std::max<int64_t>(512, (in->max_shard + in->fold_seg_max - 1) /
                                                                 std::max<int64_t>(1, in->fold_seg_max)))
                  .grid(in->nt, in->R, 1);
}

void check_fold() {
  const int64_t M = int64_t(1) << 20;
  {  // the compacted FOLD launch's counters: every region of a call its own {cnt [n_rb] | wg0 [n_rb + 1]}
    for (int64_t n_rb : {1, 20, 512, 4096}) {
      size_t end = 0;
      for (int c = 0; c < kMaxChunks; ++c)
        for (bool vstk : {true, false}) {
          const int r = sr_fold_region(c, vstk);
          CHECK(r >= 0 && r < 2 * kMaxChunks);
          CHECK(sr_fold_wg_off(r, n_rb) >= end);  // (regions in launch order, none overlapping the last)
          end = sr_fold_wg_off(r, n_rb) + size_t(n_rb) + size_t(n_rb + 1);
        }
      CHECK(end <= sr_fold_wg_words(n_rb));
    }
  }
  {  // the listed loss launch's buffer: the list, word-aligned counters per chunk, the marks, none overlapping
    for (int64_t nt : {1, 7, 600, 10000, 100000}) {
      CHECK(sr_loss_list_cnt_off(nt) >= size_t(nt) * sizeof(int32_t) && sr_loss_list_cnt_off(nt) % sizeof(int32_t) == 0);
      CHECK(sr_loss_list_excl_off(nt) >= sr_loss_list_cnt_off(nt) + size_t(kMaxChunks) * kLossListCnt * sizeof(int32_t));
      CHECK(sr_loss_list_bytes(nt) >= sr_loss_list_excl_off(nt) + size_t(nt));
    }
  }
  {  // 100 trees x 1,000 rows: two row blocks of 512, 400 KiB of losses: stored
    FoldPlanIn in = fold_in(4, 100, 1000, 1000, 1000, 8, 0);
    fold_grids(&in);
    const FoldPlan p = sr_fold_plan(in);
    CHECK(p.path == 1 && p.pos_rows == 1024 && p.slot_rows == 512 && p.slots == 0);
  }
  {  // 10,000 trees x 2^20 rows: 40 GiB of losses: the FOLD pass, 24 slots of 2,048 rows per tree
    FoldPlanIn in = fold_in(4, 10000, M, M, M, 8, 16);
    fold_grids(&in);
    const FoldPlan p = sr_fold_plan(in);
    CHECK(p.path == 2 && p.pos_rows == M && p.slot_rows == 2048);
    CHECK(p.slot_budget == 24576 * M / (2048 * 4));
    CHECK(p.slots == std::min<int64_t>(std::max<int64_t>(24 * in.nt, 1024), in.fold_slot_mb * M / (p.slot_rows * 4)));
    CHECK(p.slots == 240000);
    in.nt = 10;  // at least 1,024 slots
    fold_grids(&in);
    in.fold_store_mb = 1;
    CHECK(sr_fold_plan(in).path == 2 && sr_fold_plan(in).slots == 1024);
    in.nt = 10000;  // fold_slot_mb caps the slots
    in.fold_slot_mb = 1;
    fold_grids(&in);
    const FoldPlan q = sr_fold_plan(in);
    CHECK(q.path == 2 && q.slots == 128 && q.slots == std::min<int64_t>(std::max<int64_t>(24 * in.nt, 1024), M / (q.slot_rows * 4)));
    // no FOLD build at these rows per lane
    FoldPlanIn r4 = fold_in(4, 10000, M, M, M, 4, 0);
    fold_grids(&r4);
    CHECK(sr_fold_plan(r4).path == 0);
    r4.tier = SR_TIER_FULL;  // (the FULL tier's FOLD build runs 4 rows per lane)
    CHECK(sr_fold_plan(r4).path == 2);
  }
  {  // Float64 over the store budget: the f64 sum stays (no FOLD build); within it: stored
    FoldPlanIn in = fold_in(8, 10000, M, M, M, 4, 8);
    fold_grids(&in);
    CHECK(sr_fold_plan(in).path == 0);
    // ... also when only the largest shard's share passes the budget (every rank decides alike)
    FoldPlanIn sh = fold_in(8, 1000, 32768, 4 * 32768, 5 * 32768, 4, 0);
    fold_grids(&sh);
    CHECK(double(sh.nt) * 32768 * 8 <= 512.0 * double(M) && sr_fold_plan(sh).path == 0);
    sh.max_shard = 32768;
    fold_grids(&sh);
    CHECK(sr_fold_plan(sh).path == 1);
  }
  {  // row blocks past fold_seg_max rows on the largest shard: 1,049 blocks allowed, 1,024 of 1,024 rows
    FoldPlanIn in = fold_in(4, 10000, M, M, M, 8, 16);
    in.fold_seg_max = 1000;
    fold_grids(&in);
    CHECK(in.g_big.rb_rows() == 1024 && sr_fold_plan(in).path == 0);
    in.fold_seg_max = 1024;
    fold_grids(&in);
    CHECK(sr_fold_plan(in).path == 2);
  }
  {  // a fold longer than fold_rows_max (a row-sharded call's global rows)
    FoldPlanIn in = fold_in(4, 10000, M, M, 32 * M, 8, 16);
    fold_grids(&in);
    CHECK(sr_fold_plan(in).path == 0);
    in.fold_len = 16 * M;
    CHECK(sr_fold_plan(in).path == 2);
  }
  CHECK(sr_max_shard_rows({}, 7) == 7 && sr_max_shard_rows({0, 5, 30, 31}, 5) == 25 && sr_max_shard_rows({0, 5}, 9) == 9);
}

// The compacted FOLD launch's entries per workgroup (sr_fold_list_g): the rule's bounds and its minimality,
// and the bisection sr_fold_compact_scan_kernel runs instead of the scan over g (the same g: the workgroup sum
// does not grow with g).
int bisect_g(const std::vector<int32_t>& cnt, int G, int64_t target, int64_t grid) {
  int g = G;
  if (target > 0 && G >= 4) {
    const int64_t lim = std::min(target, grid);
    int lo = 1, hi = G / 4 + 1;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (sr_fold_list_wgs(cnt.data(), int(cnt.size()), 4 * mid) <= lim) hi = mid;
      else lo = mid + 1;
    }
    if (lo <= G / 4) g = 4 * lo;
  }
  return g;
}
void check_fold_list(Rng& rng) {
  {  // C2's last chunk as the issue reasons it: 512 row blocks of ~105 entries, row block 0 lists all 1,170
    std::vector<int32_t> cnt(512, 105);
    cnt[0] = 1170;
    const int64_t grid = 512 * 27;
    CHECK(sr_fold_list_g(cnt.data(), 512, 128, 0, grid) == 128);
    CHECK(sr_fold_list_wgs(cnt.data(), 512, 128) == 511 + 10);
    CHECK(sr_fold_list_g(cnt.data(), 512, 128, 1024, grid) == 108);  // (two per row block: 511 x 2 + 21 = 1,043 at 56)
    CHECK(sr_fold_list_g(cnt.data(), 512, 128, 2048, grid) == 36);   // 511 x 3 + 33
    CHECK(sr_fold_list_g(cnt.data(), 512, 128, 1 << 20, grid) == 8);  // (4 would need 14,090 workgroups)
    CHECK(sr_fold_list_g(cnt.data(), 512, 128, 1 << 20, 1 << 20) == 4);
    CHECK(sr_fold_list_g(cnt.data(), 512, 128, 100, grid) == 128);  // no g meets the target: G
  }
  for (int it = 0; it < 2000; ++it) {
    const int n_rb = 1 + rng.below(40);
    const int G = std::vector<int>{1, 3, 4, 5, 8, 9, 16, 32, 64, 128, 256}[size_t(rng.below(11))];
    const int np = 1 + rng.below(3000);
    std::vector<int32_t> cnt(size_t(n_rb), 0);
    const int kind = rng.below(4);
    for (int r = 0; r < n_rb; ++r)
      cnt[size_t(r)] = kind == 0 ? 0 : (kind == 1 ? np : (r == 0 ? np : rng.below(np + 1) / (1 + rng.below(12))));
    const int64_t grid = int64_t(n_rb) * ((np + G - 1) / G);
    const int64_t target = std::vector<int64_t>{0, 1, 7, 100, 1000, 5000, kFoldListWgsMax}[size_t(rng.below(7))];
    const int g = sr_fold_list_g(cnt.data(), n_rb, G, target, grid);
    CHECK(g == bisect_g(cnt, G, target, grid));
    CHECK(g == G || (G >= 4 && target > 0 && g % 4 == 0 && g >= 4 && g < G));
    CHECK(sr_fold_list_wgs(cnt.data(), n_rb, g) <= grid);  // the launch always fits its grid
    if (target == 0) CHECK(g == G);
    if (g != G) {
      CHECK(sr_fold_list_wgs(cnt.data(), n_rb, g) <= target);
      if (g > 4) CHECK(sr_fold_list_wgs(cnt.data(), n_rb, g - 4) > std::min(target, grid));  // the smallest
    }
    // every listed entry belongs to exactly one workgroup's [k g, k g + g) of its row block
    for (int r = 0; r < n_rb; ++r) {
      const int64_t w = (int64_t(cnt[size_t(r)]) + g - 1) / g;
      CHECK(w * g >= cnt[size_t(r)] && (w == 0 || (w - 1) * g < cnt[size_t(r)]));
    }
  }
}

}  // namespace

int main() {
  check_grids();
  check_chunks();
  Rng rng{12345};
  check_fold_list(rng);
  for (int64_t nc : {1, 2, 127, 128, 129, 1000})
    for (int tree_group : {0, 4, 32}) check_order(rng, nc, tree_group);
  check_fold();
  if (g_failed) {
    std::fprintf(stderr, "plan_check: %d checks failed\n", g_failed);
    return 1;
  }
  std::printf("plan_check: ok\n");
  return 0;
}
