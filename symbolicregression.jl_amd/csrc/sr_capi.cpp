// sr_capi.cpp — the C ABI (include/sr_amd.h) over the HIP interpreter.
//
// Call path of one batched scoring call (sr_eval_loss_batch):
//   host: compile the trees (sr_compile.cpp) -> upload programs -> interpreter kernel (partials per
//   row block) -> fixed-order reduce kernel -> copy per-tree {Σloss, flags} back -> rare exact-sum
//   check for trees whose checked values came close to overflowing -> loss = Σ / denominator.
// Mirrors reference src/LossFunctions.jl:90-117 (`_eval_loss`) for each tree of the batch.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <dlfcn.h>
#include <limits.h>
#include <stdlib.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/sr_amd.h"
#include "sr_compile.h"
#include "sr_eval.h"
#include "sr_fold.h"
#include "sr_fold_dev.h"
#include "sr_knobs.h"
#include "sr_param_pack.h"

namespace {

thread_local std::string g_last_error;
struct SrComm;  // the sharded calls' transport (multi-GPU section below)

int set_error(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}

#define SR_HIP_CHECK(expr)                                                                          \
  do {                                                                                              \
    hipError_t _e = (expr);                                                                         \
    if (_e != hipSuccess)                                                                           \
      return set_error(SR_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));              \
  } while (0)

// A device allocation that grows on demand and belongs to whatever holds it (the context: freed with it).
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  hipError_t ensure(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    if (p) {
      hipError_t e = hipFree(p);
      if (e != hipSuccess) return e;
      p = nullptr;
      cap = 0;
    }
    size_t want = bytes < 4096 ? 4096 : bytes + bytes / 4;
    hipError_t e = hipMalloc(&p, want);
    if (e == hipSuccess) cap = want;
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  template <typename U>
  U* as() const {
    return static_cast<U*>(p);
  }
};

// Pinned host staging (programs, offsets, launch order): hipMemcpyAsync from it is a true async DMA,
// so the host compiles the next chunk while the device runs the previous one.
struct HostBuf {
  void* p = nullptr;
  size_t cap = 0;
  unsigned flags = hipHostMallocDefault;
  HostBuf() = default;
  HostBuf(const HostBuf&) = delete;
  HostBuf& operator=(const HostBuf&) = delete;
  ~HostBuf() { release(); }
  hipError_t ensure(size_t bytes, hipStream_t s, hipStream_t s2) {
    if (bytes <= cap) return hipSuccess;
    if (p) {
      hipError_t e = hipStreamSynchronize(s);  // no DMA may still read the old buffer
      if (e == hipSuccess && s2) e = hipStreamSynchronize(s2);  // (a context's second stream is created lazily)
      if (e == hipSuccess) e = hipHostFree(p);
      if (e != hipSuccess) return e;
      p = nullptr;
      cap = 0;
    }
    size_t want = bytes < 65536 ? 65536 : bytes + bytes / 4;
    hipError_t e = hipHostMalloc(&p, want, flags);
    if (e == hipSuccess) cap = want;
    return e;
  }
  void release() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
  }
  template <typename U>
  U* as() const {
    return static_cast<U*>(p);
  }
};

constexpr int kLossCodeBase = 256;
// expression losses (sr_register_loss_expr): code = kLossExprBase + index
constexpr int kLossExprBase = 1 << 20;
const char* const kLossExprOnly =
    "an expression loss (sr_register_loss_expr) is taken by sr_eval_loss_batch(_views), sr_eval_grad_batch(_views), "
    "sr_optimize_constants_batch and the native search on plain trees only: not by the parametric, sharded, partials "
    "or jsum calls";

// Parameter-free losses (and HuberLoss with its default delta = 1) may be passed by kind.
inline bool loss_direct_ok(int kind) {
  switch (kind) {
    case SR_LOSS_LP: case SR_LOSS_L1_EPS_INS: case SR_LOSS_L2_EPS_INS: case SR_LOSS_PERIODIC:
    case SR_LOSS_QUANTILE: case SR_LOSS_SMOOTH_L1_HINGE: case SR_LOSS_DWD_MARGIN:
      return false;
    default:
      return kind >= 0 && kind < SR_LOSS_COUNT;
  }
}

}  // namespace

// the thread-local error message, for the other translation units of the library (sr_search.cpp)
int sr_set_error(int code, const std::string& msg) { return set_error(code, msg); }

// The context: its tuning knobs (SrKnobs, sr_knobs.h) and its streams, events, buffers and last-call records.
struct sr_ctx : SrKnobs {
  int device = 0;
  hipStream_t stream = nullptr;
  // second stream of the chunked pipeline (odd chunks), created on the first chunked call: a HIP
  // stream takes one of the process's GPU_MAX_HW_QUEUES (4) hardware queues round-robin at creation, so
  // an idle second stream per context left the search's four scoring lanes sharing two queues
  hipStream_t stream2 = nullptr;
  hipError_t need_stream2() {
    return stream2 ? hipSuccess : hipStreamCreateWithFlags(&stream2, hipStreamNonBlocking);
  }
  // (the exact_early knob's events and stream, sr_knobs.h)
  hipEvent_t ev_flags = nullptr;
  hipEvent_t ev_red[kMaxChunks] = {};  // chunk c's loss launches and reduces have ended
  hipStream_t stream3 = nullptr;       // the early exact-sum pass's, created on the first such call
  hipError_t need_stream3() {
    return stream3 ? hipSuccess : hipStreamCreateWithFlags(&stream3, hipStreamNonBlocking);
  }
  hipEvent_t ev_join = nullptr;
  hipEvent_t ev_start = nullptr, ev_k0 = nullptr, ev_k1 = nullptr, ev_end = nullptr;
  hipEvent_t ev_c0[kMaxChunks] = {}, ev_c1[kMaxChunks] = {};  // per-chunk interpreter launches
  hipEvent_t ev_d0 = nullptr, ev_d1 = nullptr;                 // the derived-column launch
  // the last gradient call's tangent-kernel launches, per tangent bucket (1, 2, 4, 8, 16): HIP events,
  // algorithmic flops (sr_last_grad_info), work items, rows per lane
  static constexpr int kGradBuckets = 5;
  hipEvent_t ev_g0[kGradBuckets] = {}, ev_g1[kGradBuckets] = {};
  // the in-order loss fold's device phases (sr_last_fold_ms): PRED pass, segment sums, composed steps,
  // chain; events around each, accumulated over the call's fold batches (the fold is rare: always timed)
  hipEvent_t ev_f[5] = {};
  double fold_ms[4] = {0, 0, 0, 0};
  bool grad_timed[kGradBuckets] = {};
  double grad_ms_done[kGradBuckets] = {};  // (a chunked call's earlier launches of the bucket, read back already)
  double grad_flops[kGradBuckets] = {};
  int64_t grad_items[kGradBuckets] = {};
  int grad_rows[kGradBuckets] = {};
  // What the last run_batch did, for the sr_last_* / sr_tuning_info / sr_ref_fold_info / sr_last_fold_cand
  // getters and settle_timing: no call decides anything from an earlier call's record.  Written by a call's own
  // run_batch (and its fold's launches); the fold's internal prediction passes (BatchWants::internal) write a
  // scratch copy instead.
  struct LastCall {
    int n_chunks = 0;
    int rows = 0;          // rows per lane of the interpreter launches (sr_last_phase_ms out[7])
    bool timed = false;    // the call recorded its events
    bool derived = false;  // it launched derived columns (timed by ev_d0 / ev_d1)
    int n_derived = 0;
    int fold_path = 0;     // 0 none, 1 stored losses, 2 FOLD mode
    bool fold_timed = false;
    // the listed launches (loss_compact): per chunk the launch's positions (0: not listed), and the counters
    // read back once on request (sr_last_phase_ms out[16..18])
    int64_t loss_listed_np[kMaxChunks] = {};
    int64_t loss_list_nt = 0;
    bool loss_list_read = true;
    int64_t n_loss_listed_launches = 0, n_loss_live = 0, n_loss_excl = 0;
    // the compacted FOLD launches (fold_compact): per region its row blocks (0: none) and the call's row
    // blocks per position, for sr_last_phase_ms out[19..] (read back once on request)
    int fold_wg_nrb[2 * kMaxChunks] = {};
    int64_t fold_wg_stride_rb = 0;
    bool fold_wg_read = true;
    double fold_wg_info[2 * kMaxChunks][4] = {};  // {live workgroups, listed entries, g, the longest list}
    bool fold_cand_read = true;  // fold_ctl's counters are in n_cand_* below
    int64_t n_cand_taken = 0, n_cand_rerun = 0;
  } last;
  int64_t n_exact_last = 0;  // trees of the last eval_loss call sent through the exact-sum pass
  int64_t n_fold_last = 0;   // trees of the last eval_loss call whose loss fold was computed in order (sr_fold.h)
  int64_t fold_slow_last = 0;  // ... their segments folded row by row (the rest: composed steps)
  int64_t fold_seg_last = 0;   // ... and the segment length used
  double exact_kernel_ms = 0.0;  // device time of that pass (its interpreter + combine launches)
  // programs + per-tree metadata of the last run_batch: ONE device allocation and ONE pinned staging
  // buffer with the same layout (code | offsets | static_bad | launch order), so a single-chunk call
  // uploads with one DMA; per-tree {Σ loss, flags} likewise share one allocation (one DMA back)
  HostBuf h_prog, h_outs, h_grad;  // (h_grad: the gradient call's staging image, then its results)
  // the host_reduce knob's (sr_knobs.h) pinned partials and the launches that wrote them
  HostBuf h_part;
  struct HostReduction {
    int64_t p0, np;
    int n_rb;
  };
  std::vector<HostReduction> host_reductions;  // this call's launches whose partials await the host
  std::vector<double> host_acc;                // (their per-(position, lane) accumulators)
  std::vector<uint32_t> host_fl;
  int64_t host_red_rb = 0;                     // their partial buffer's row-block stride (n_rb)
  const uint8_t* h_bad_last = nullptr;         // the last run_batch's staged static flags and launch order
  const uint32_t* h_perm_last = nullptr;
  void* d_code = nullptr;
  uint32_t* d_off = nullptr;
  uint8_t* d_bad = nullptr;
  uint32_t* d_perm = nullptr;
  uint32_t* d_end = nullptr;  // [nt] end of each tree's program (code is staged in launch order)
  double* d_out_sum = nullptr;
  uint32_t* d_out_flag = nullptr;
  size_t outs_flag_off = 0;
  uint32_t hint_epoch = 0;  // dead-tree hint epoch of the current call
  void* hint_reserve = nullptr;    // debug_hint_regrow's fixed-address reservation
  std::mutex mu;
  std::vector<SrOpset> opsets;
  std::vector<int> tiers;
  std::vector<std::pair<int, double>> losses;  // registered (kind, param); code = kLossCodeBase + index
  // expression losses (sr_register_loss_expr; code = kLossExprBase + index): the registration's bytes (the
  // same expression again gets the same code), the program per element type (sr_loss_expr.h) and their
  // device copies — one small buffer, uploaded once: the Float32 instructions, then the Float64 ones
  struct LossExpr {
    std::string key;
    SrLossProg<float> p32;
    SrLossProg<double> p64;
    void* dev = nullptr;
    template <typename T>
    const SrLossProg<T>& prog() const {
      if constexpr (sizeof(T) == 4) return p32;
      else return p64;
    }
    template <typename T>
    SrLossProgArgs<T> args() const {
      const char* d = static_cast<const char*>(dev);
      if constexpr (sizeof(T) == 4) return SrLossProgArgs<T>{reinterpret_cast<const SrIns<T>*>(d), p32.n};
      else return SrLossProgArgs<T>{reinterpret_cast<const SrIns<T>*>(d + sizeof(p32.ins)), p64.n};
    }
  };
  std::deque<LossExpr> loss_exprs;  // (a deque: a call keeps a pointer to its entry while others register)
  DevBuf prog, outs, part_sum, part_flag, pred, row_idx,
      range_lo, range_hi, range_sums, packed, hint, jsum_prog, jsum_scratch, probe_sum, probe_flag, g_code, g_offsets, g_consts, g_const_off, g_items, g_part, g_out,
      derived_cols, probe_derived, fold_io;
  // The exact-sum pass's small transfers (round 5): the leaf ranges and the Julia-sum level program
  // depend only on the view's row count, so they stay on the device between calls (host mirrors below;
  // a buffer that grows loses them); the pass reads its tree list from pinned memory and the verdicts come
  // back through it.  Pageable copies cost ~15 us each, and a one-tree pass made five of them.
  HostBuf h_exact;
  std::vector<int64_t> exact_lo_dev, exact_hi_dev;  // what range_lo / range_hi hold
  int64_t jsum_n_dev = -1;                          // the row count jsum_prog was built for
#ifdef SR_STAMPS
  DevBuf stamps;  // latency-analysis builds: the last main launch's per-wave stamps (sr_debug_stamps)
  int64_t n_stamps = 0;
#endif
  // data-path transport of the sharded calls: the library's own RCCL over xGMI on its own HIP runtime
  // (sr_comm_init; torch's bundled runtime cannot share the GPU with this one in a process), or the
  // caller's host collectives (sr_comm_init_host)
  std::unique_ptr<SrComm> xport;
  int comm_ranks = 0;
  int comm_rank = 0;
  uint64_t comm_gen = 0;  // process-unique id of the current communicator (shard layouts are cached per id)
  // buffers of the sharded calls' collectives only (their growth is identical on every rank: Prep):
  // shard layout / exact-pass folds / loss-fold chain / tree results, the packed partials, the agree word
  DevBuf coll_buf, coll_packed, ctl;
  HostBuf h_coll;        // pinned staging of the tree-sharded results
  double last_eval_ms = 0.0, last_total_ms = 0.0;
  double last_busy_ms = 0.0;  // union of the last call's interpreter launch intervals (sr_last_phase_ms out[8])
  // the two above are read from the last call's events lazily, when asked for (sr_last_kernel_ms /
  // sr_last_phase_ms): a small call (the search's) does not pay the event queries it never reads
  bool timing_pending = false;
  // host-side phases of the last eval_loss call (ms): compile, upload+launch, wait, exact pass,
  // finalize (sr_last_phase_ms)
  double phase_ms[5] = {0, 0, 0, 0, 0};
  std::chrono::steady_clock::time_point phase_t;
  void start_phases(std::chrono::steady_clock::time_point t) {
    phase_t = t;
    for (double& v : phase_ms) v = 0.0;
  }
  void mark_phase(int i) {
    const auto now = std::chrono::steady_clock::now();
    phase_ms[i] = std::chrono::duration<double, std::milli>(now - phase_t).count();
    phase_t = now;
  }
  int cu_count = 256;
  std::vector<uint32_t> perm_host;
  // The in-order loss fold's buffers (the ref_fold and fold_* knobs: sr_knobs.h)
  DevBuf fold_cand;          // (fold_single_pass) the candidates, [row block][position] int4 (sr_fold_dev.h)
  DevBuf fold_list;          // (fold_compact) [row block][position] int32, laid out as the partials
  DevBuf fold_wg;            // per region (2 per chunk): {cnt [n_rb], wg0 [n_rb + 1], g}
  DevBuf loss_list;          // (loss_compact) {list int32 [nt] | cnt int32 [kMaxChunks][4] | excl uint8 [nt]} (sr_plan.h)
  DevBuf fold_est;           // (fold_cand_est) per launch position: {f64 sum [nt] | u32 count [nt]}, zeroed by every call
  DevBuf fold_dbg;           // (fold_stats)
  DevBuf fold_code, fold_tab, fold_store, fold_ctl, fold_io2, fold_sq, fold_tab2;
  std::shared_ptr<void> fold_job;  // a row-sharded call's FoldJob<T>, until its ranks agree on the verdicts
  size_t outs_fval_off = 0, outs_fst_off = 0, outs_bytes_all = 0;
  hipEvent_t ev_fc0[kMaxChunks] = {}, ev_fc1[kMaxChunks] = {};  // each chunk's fold launches
  int64_t n_ref_ok_last = 0, n_ref_fail_last = 0;  // trees whose loss is the walk's fold / that fell back
  double fold_kernel_ms_last = 0.0;
  DevBuf ptab;     // the last parametric run_batch's table (EvalReq::params), [tree][parameter][class] (T)
  HostBuf h_ptab;  // its pinned staging
};

// For the search engine (sr_search.cpp, not in the public header): set the context's "timing" knob
// and return its previous value, under the context's lock (a caller's setting is restored after the
// engine's calls).
int sr_ctx_swap_timing(sr_ctx* ctx, int value) {
  std::lock_guard<std::mutex> g(ctx->mu);
  const int old = ctx->timing;
  ctx->timing = value != 0 ? 1 : 0;
  return old;
}

struct sr_dataset {
  sr_ctx* ctx = nullptr;
  int dtype = SR_DTYPE_F32;
  int64_t nf = 0, n = 0, ld = 0;
  void* X = nullptr;  // [nf][ld]
  void* y = nullptr;  // [ld] or NULL
  void* w = nullptr;  // [ld] or NULL
  std::vector<double> w_host;  // weights (for Σw of SubDataset views)
  double wsum = 0.0;
  double w_min = 0.0;      // smallest weight (the loss-fold overflow rule needs w >= 0: sr_fold.h)
  double max_abs_x = 0.0;  // max |X| over the data (NaN / Inf if any value is non-finite)
  // sr_dataset_upload_classes: the rows' classes, 0-based in T, as row nf of X (a hidden extra row: nf,
  // max_abs_x and the probe's stress rows leave it out; only parametric calls stage it); 0: no classes
  int32_t n_classes = 0;
  mutable double wsum_jl_f32 = NAN, wsum_jl_f64 = NAN;  // Base.sum(w) in Float32 / Float64 (cached on first use)
  // dead-tree probe rows (large datasets): the "stress rows" — per feature the K largest, K smallest
  // and K smallest-magnitude values, where exp overflows, logs and divisions blow up — then rows 0, 1,
  // ... up to kProbeRows; int64 row indices on the device (NULL for small datasets)
  void* probe_rows = nullptr;
  int64_t n_probe = 0;
  // row-sharded calls (sr_eval_loss_sharded): every shard's rows, Σw and max|X|, exchanged once per
  // communicator (shard_gen = its sr_ctx::comm_gen; rank r holds global rows [offs[r], offs[r + 1]))
  mutable uint64_t shard_gen = 0;
  mutable std::vector<int64_t> shard_offs;
  mutable double shard_wsum = 0.0, shard_max_abs_x = 0.0;
  mutable double shard_w_min = 0.0;  // smallest weight over every shard
  mutable int64_t shard_min_rows = 0;
};

namespace {

constexpr int64_t kRowAlign = 2048;  // a multiple of every kernel's row tile (64 lanes x R rows)
constexpr int64_t kProbeRows = 2048;
constexpr int kProbeTiles = 4;  // row tiles of a dead-tree probe launch
// dynamic LDS a register-stack workgroup may use with its program cache: with the 5 KiB of static
// libm tables, 4 workgroups still fit a CU's 160 KiB
constexpr size_t kCodeCacheLds = 34 * 1024;

template <typename T>
double t_max() {
  return double(SrM<T>::big);
}

struct Lock {
  std::lock_guard<std::mutex> g;
  explicit Lock(sr_ctx* c) : g(c->mu) {}
};

int check_ctx(sr_ctx* ctx) {
  if (!ctx) return set_error(SR_ERR_INVALID_ARG, "NULL context");
  return SR_OK;
}

int validate_common(sr_ctx* ctx, const sr_dataset* ds, int opset_id, const sr_tree_batch* trees) {
  if (check_ctx(ctx) != SR_OK) return SR_ERR_INVALID_ARG;
  if (!ds || ds->ctx != ctx)
    return set_error(SR_ERR_INVALID_ARG, "dataset is NULL or belongs to another context");
  if (opset_id < 0 || opset_id >= int(ctx->opsets.size()))
    return set_error(SR_ERR_INVALID_ARG, "unknown opset id " + std::to_string(opset_id));
  if (!trees) return set_error(SR_ERR_INVALID_ARG, "NULL tree batch");
  if (trees->n_trees < 0) return set_error(SR_ERR_INVALID_ARG, "negative tree count");
  if (trees->n_trees > (int64_t(1) << 30)) return set_error(SR_ERR_INVALID_ARG, "too many trees in one batch");
  return SR_OK;
}

// loss_kind as passed to the eval calls -> (SrLossKind, parameter).
// expr: where the call takes expression losses, receives the registered one (NULL otherwise); a call that
// passes none refuses their codes.
int decode_loss(sr_ctx* ctx, int code, int* kind, double* param, const sr_ctx::LossExpr** expr = nullptr) {
  if (expr) *expr = nullptr;
  if (code >= kLossExprBase) {
    const size_t i = size_t(code - kLossExprBase);
    if (i >= ctx->loss_exprs.size()) return set_error(SR_ERR_INVALID_ARG, "unknown expression loss code " + std::to_string(code));
    if (!expr) return set_error(SR_ERR_INVALID_ARG, kLossExprOnly);
    *kind = SR_LOSS_EXPR;
    *param = 0.0;
    *expr = &ctx->loss_exprs[i];
    return SR_OK;
  }
  if (code >= kLossCodeBase) {
    const size_t i = size_t(code - kLossCodeBase);
    if (i >= ctx->losses.size()) return set_error(SR_ERR_INVALID_ARG, "unknown registered loss code " + std::to_string(code));
    *kind = ctx->losses[i].first;
    *param = ctx->losses[i].second;
    return SR_OK;
  }
  if (!loss_direct_ok(code))
    return set_error(SR_ERR_INVALID_ARG, "loss kind " + std::to_string(code) +
                                             " is unknown or needs a parameter: register it with sr_register_loss");
  *kind = code;
  *param = code == SR_LOSS_HUBER ? 1.0 : 0.0;
  return SR_OK;
}

// Row-sharded calls decide data-dependent launch choices from the statistics of ALL shards, so every
// rank compiles identical programs (same derived columns: the exact path numbers checked arrays the
// same on every rank): max|X| over every shard and the smallest shard's row count.
struct ShardCtl {
  double max_abs_x;
  int64_t min_rows;
};

// Several row views in one LOSS call (sr_eval_loss_batch_views): tree t is scored on the rows
// view_rows[tree_view[t] * view_len ...] (the caller's row_idx array holds n_views views of view_len rows).
struct ViewSpec {
  const int32_t* tree_view;
  int n_views;
  int64_t view_len;
};

// What a scoring call asked for: filled once by the entry point and passed by reference to every function
// behind it (the fold's fallback builds a sub-request over a few of its trees: fold_prepare).
struct EvalReq {
  const sr_dataset* ds = nullptr;
  int opset_id = 0;
  const sr_tree_batch* trees = nullptr;
  const sr_param_batch* params = nullptr;  // the batch's parameter side (sr_eval_*_parametric); NULL: plain trees
  const int64_t* row_idx = nullptr;        // the view's rows (views: n_views views of n_idx rows each); NULL: every row
  int64_t n_idx = 0;
  const ViewSpec* views = nullptr;         // several row views in one call; NULL: one view
  int loss_kind = 0;                       // as passed to the eval calls (decode_loss)
  const sr_scalar_ties* ties = nullptr;    // sr_eval_grad_batch_tied: tied / frozen constants (the gradient only)
  bool gather() const { return row_idx != nullptr && n_idx > 0; }
  int64_t n_eval() const { return gather() ? n_idx : ds->n; }
  // view v alone, as a request of its own (the exact-sum pass and the fallback fold run view by view)
  EvalReq view(int v) const {
    EvalReq r = *this;
    r.row_idx = gather() ? row_idx + int64_t(v) * n_idx : nullptr;
    r.views = nullptr;
    return r;
  }
};

// What a caller wants from run_batch beside the request.
struct BatchWants {
  int mode = SR_MODE_LOSS;
  int64_t n_total = 0;          // rows of the whole view over every shard (the overflow budgets)
  bool allow_derived = false;   // derived columns may be used
  const ShardCtl* shard = nullptr;
  bool host_out = false;        // (host_io) a small call's {Σ, flags} may go straight to pinned memory
  bool fold = false;            // the caller takes every complete tree's in-order fold (ref_fold)
  bool early = false;           // the caller can take the flags early (exact_early)
  bool takes_expr = false;      // the call accepts expression losses
  bool internal = false;        // a pass inside another call (the fold's PRED passes): the last-call record, the
                                // timing events and the phase clock stay that call's
};

// What run_batch hands back beside the context-owned buffers (d_out_sum, d_out_flag, ...).
struct BatchResult {
  Grid grid;                  // the last launch's
  bool early = false;         // the flags were copied early, the results' copy is left to the caller
  bool outs_on_host = false;  // {Σ, flags} are in h_outs already
  int fold_path = 0;          // 0 none, 1 stored losses, 2 FOLD mode
};

// Rows of the reference's loss fold for the overflow rule (sr_fold.h), or 0 when the rule does not
// apply (negative weights: the fold is not monotone; an expression loss, which may be negative itself:
// such a call runs as a call on a dataset with a negative weight does — the f64 sum, no fold, no verdict
// from bounds).
inline int64_t fold_terms(const sr_dataset* ds, int64_t n_rows, int loss_code = 0) {
  return ((ds->w && ds->w_min < 0.0) || loss_code >= kLossExprBase) ? 0 : n_rows;
}
// An expression loss against the dataset: the weight is its third argument exactly when the dataset has
// weights (the reference calls loss(x, y, w) then, loss(x, y) otherwise: a MethodError for the other arity).
inline int check_loss_expr_weights(const sr_ctx::LossExpr* e, const sr_dataset* ds) {
  if (!e) return SR_OK;
  if (e->p32.uses_w && !ds->w)
    return set_error(SR_ERR_INVALID_ARG, "the loss expression references the weight, but the dataset has no weights");
  if (!e->p32.uses_w && ds->w)
    return set_error(SR_ERR_INVALID_ARG, "the dataset has weights, but the loss expression takes (prediction, target) only");
  return SR_OK;
}

// ---------------------------------------------------------------- every complete tree's in-order fold
// One loss launch of a call whose trees the in-order fold covers (sr_ctx::ref_fold): its arguments (the
// FOLD pass re-launches them), launch positions [pos0, pos0 + np) of the call (chunk t0: perm values and
// per-tree arrays are chunk-local), grid and kernel build.
template <typename T>
struct FoldRegion {
  SrEvalArgs<T> a;  // (a parametric call's: ptab set)
  int64_t t0, pos0, np, n_blocks;
  int Rc;
  bool vstk;
  Grid g;
  int idx = -1;  // its place among the call's regions (the compacted FOLD launch's counters); -1: no compaction
  int64_t rb_rows() const { return int64_t(g.tiles) * 64 * Rc; }
  // the region's offset in the partial buffers of n_rb row blocks per position, and its plan arrays there
  size_t off(int64_t n_rb) const { return size_t(n_rb) * size_t(pos0); }
  SrFoldTabs tabs(sr_ctx* ctx, int64_t n_rb) const;
};
// A call's fold: its regions and the launch facts every fold kernel needs (kept by a row-sharded call's
// batch engine until the ranks have agreed on the verdicts: FoldJob::deferred).
template <typename T>
struct FoldJob {
  std::vector<FoldRegion<T>> regions;
  int path = 0;  // 1 stored losses, 2 FOLD pass
  int tier = 0;
  bool gather = false;
  int64_t n_eval = 0, n_rb = 0, slot_rows = 0, n_terms = 0;
  int slot_cap = 0;
  double delta = 0.0;
  bool fuse_reduce = false;  // (stored losses, one GPU: the pair kernel does the call's reduce)
};

// a region's plan arrays at partial-buffer offset off
template <typename T>
SrFoldTabs fold_tabs(sr_ctx* ctx, size_t off) {
  using Pair = typename SrFoldTab<T>::Pair;
  return SrFoldTabs{ctx->fold_code.as<int32_t>() + off, ctx->fold_tab.as<char>() + off * sizeof(Pair),
                    ctx->fold_sq.as<int32_t>() + off, ctx->fold_tab2.as<char>() + off * sizeof(Pair)};
}
template <typename T>
SrFoldTabs FoldRegion<T>::tabs(sr_ctx* ctx, int64_t n_rb) const {
  return fold_tabs<T>(ctx, off(n_rb));
}
// the call's whole-batch arrays (sums / flags / elig / est / the pinned mirrors at the caller's tree
// index) from a region's chunk offset on
inline SrFoldWho fold_who_at(SrFoldWho who, int64_t t0) {
  if (who.sums) who.sums += t0;
  if (who.flags) who.flags += t0;
  if (who.elig) who.elig += t0;
  if (who.est) who.est += t0;
  if (who.msum) who.msum += t0;
  if (who.mflag) who.mflag += t0;
  return who;
}
// A stored-loss call of one row block of at most 256 rows that starts the fold (C1's 100-row calls): the
// walk's serial start folds every row and takes eligibility from the call's flags itself, so the pair
// kernel's launch is skipped (round 6: ~5 us of a ~45 us call)
template <typename T>
bool fold_tiny(const FoldJob<T>& job, const FoldRegion<T>& fr, const SrFoldWho& who) {
  return job.path == 1 && fr.g.n_row_blocks == 1 && job.n_eval <= 256 && who.first && who.elig == nullptr &&
         who.est == nullptr;
}
// A region's steps: the stored-loss tables (path 1) or the plan and the FOLD pass (path 2).  who: the
// call's whole-batch arrays (this function adds the region's chunk offset).
template <typename T>
int fold_steps(sr_ctx* ctx, const FoldJob<T>& job, const FoldRegion<T>& fr, SrFoldWho who, hipStream_t cs) {
  const int nrb = fr.g.n_row_blocks;
  const SrFoldTabs ft = fr.tabs(ctx, job.n_rb);
  const double* part = nrb > 1 ? fr.a.part_sum : nullptr;
  const int np = int(fr.np);
  who = fold_who_at(who, fr.t0);
  if (job.path == 1) {
    if (fold_tiny(job, fr, who)) return SR_OK;  // (the walk's serial start is the whole fold: no pairs)
    const bool fr_red = job.fuse_reduce && nrb > 1;
    SR_HIP_CHECK(sr_launch_fold_stab<T>(part, np, nrb, fr.rb_rows(), job.n_eval, fr.a.perm, who, job.delta,
                                        fr.a.fold_loss, ft, fr_red ? fr.a.part_flag : nullptr,
                                        fr_red ? ctx->d_bad + fr.t0 : nullptr, fr_red ? ctx->d_out_sum + fr.t0 : nullptr,
                                        fr_red ? ctx->d_out_flag + fr.t0 : nullptr, cs));
    return SR_OK;
  }
  SR_HIP_CHECK(sr_launch_fold_plan<T>(part, np, nrb, fr.a.perm, who, job.delta, ft, ctx->fold_ctl.as<int>(),
                                      job.slot_cap, fr.a.fold_cand, cs));
  SrEvalArgs<T> fa = fr.a;
  fa.hint = nullptr;
  fa.out_sum = nullptr;
  fa.out_flag = nullptr;
  fa.stamps = nullptr;
  fa.fold_code = ft.code;
  fa.fold_tab = ft.tab;
  fa.fold_sq = ft.sq;
  fa.fold_tab2 = ft.tab2;
  fa.fold_loss = ctx->fold_store.as<T>();
  fa.fold_slot_rows = job.slot_rows;
  fa.fold_pos_stride = 0;
  fa.fold_cand = nullptr;
  fa.fold_est_sum = nullptr;
  fa.fold_est_cnt = nullptr;
  fa.fold_list = nullptr;  // (a listed loss launch's list is not the FOLD pass's)
  fa.fold_cnt = nullptr;
  fa.fold_wg0 = nullptr;
  // the compacted launch (sr_ctx::fold_compact): plain single-GPU calls over the full view; the grid stays the
  // region's (an upper bound: the list's workgroups come first, the rest return at once)
  if (ctx->fold_compact && fr.idx >= 0 && !fr.a.ptab && !job.gather && fr.a.segs == nullptr && who.elig == nullptr &&
      who.est == nullptr) {
    int32_t* cnt = ctx->fold_wg.as<int32_t>() + sr_fold_wg_off(fr.idx, job.n_rb);
    int32_t* wg0 = cnt + job.n_rb;
    int32_t* list = ctx->fold_list.as<int32_t>() + fr.off(job.n_rb);
    SR_HIP_CHECK(sr_launch_fold_compact(ft, np, nrb, fr.a.trees_per_block, int(ctx->fold_list_wgs),
                                        int(std::min<int64_t>(fr.n_blocks, kFoldListWgsMax)), list, cnt, wg0, cs));
    ctx->last.fold_wg_nrb[fr.idx] = nrb;  // (sr_last_phase_ms out[19..]; no internal pass folds)
    ctx->last.fold_wg_stride_rb = job.n_rb;
    ctx->last.fold_wg_read = false;
    fa.fold_list = list;
    fa.fold_cnt = cnt;
    fa.fold_wg0 = wg0;
    fa.code_lds = 0;  // (a listed workgroup's programs are no contiguous span: no LDS program cache)
  }
  // the FOLD build of the region's loss launch (a candidate launch's: the plain register-stack FOLD build)
  const SrBuildRequest q{int(sizeof(T)), SR_MODE_FOLD, job.gather, job.tier, fr.Rc, fr.g.W, fr.vstk, fa.loss_kind,
                         fa.ptab ? SR_FAMILY_PARAM : SR_FAMILY_PLAIN};
  SR_HIP_CHECK(sr_launch_eval<T>(fa, q, int(fr.n_blocks), cs));
  return SR_OK;
}
// A region's walk: the folds' values and status at the caller's tree index (out arrays and carry are
// whole-batch, tree-indexed).
template <typename T>
int fold_walk(sr_ctx* ctx, const FoldJob<T>& job, const FoldRegion<T>& fr, SrFoldWho who, const T* carry, T* out_val,
              int32_t* out_st, hipStream_t cs) {
  const int nrb = fr.g.n_row_blocks;
  const int tiny = carry == nullptr && fold_tiny(job, fr, who) ? 16 : 0;
  // (stored losses, the pair kernel launched, the fold starting here: it did the serial start)
  const int pre = job.path == 1 && !tiny && carry == nullptr && who.first ? 32 : 0;
  who = fold_who_at(who, fr.t0);
  const int64_t rb_rows = fr.rb_rows();
  const SrFoldTabs ft = fr.tabs(ctx, job.n_rb);
  const T* losses = job.path == 1 ? fr.a.fold_loss : ctx->fold_store.as<T>();
  const int64_t slot_rows = job.path == 1 ? rb_rows : job.slot_rows;
  int4* dbg = ctx->fold_stats ? ctx->fold_dbg.as<int4>() + fr.t0 : nullptr;  // (SR_AMD_FOLD_STATS)
  // (fold_stats 2, analysis: the same walk again, its loads now warm: the statistics are the second's)
  for (int pass = 0; pass < (ctx->fold_stats == 2 ? 2 : 1); ++pass)
    SR_HIP_CHECK(sr_launch_fold_walk<T>(ft, who, int(fr.np), nrb, rb_rows, job.n_eval, losses, slot_rows, fr.a.perm,
                                        carry ? carry + fr.t0 : nullptr, out_val + fr.t0, out_st + fr.t0, dbg,
                                        int(job.path == 1) | tiny | pre, cs));
  return SR_OK;
}

// ---------------------------------------------------------------- the batch engine
// Shared engine: compile + upload + interpreter(+reduce).  Leaves per-tree {sum, flag} in
// ctx->d_out_sum / ctx->d_out_flag (device).  n_eval rows (full dataset or row_idx view).
//
// Large LOSS batches are pipelined in up to kMaxChunks tree chunks: the host compiles chunk c+1
// while the device runs chunk c (programs staged through pinned memory, async DMA).  Every chunk is
// an independent launch over its own slice of the per-tree device arrays; `prog` receives the merged
// per-tree summary (offsets into the device code buffer, static_bad, max_depth, max_checks) that
// the exact-sum pass and the callers use — its `code` stays empty.
//
// run_batch is a driver over the stages below (DESIGN.md §4.6 lists them in order); the host-only
// decisions — grids, chunks, launch order, code layout, segments, the fold's path — are sr_plan.h's.
// One tree chunk [t0, t0 + nc) of a call: its compiled programs and launch plan.
template <typename T>
struct BatchChunk {
  int c = 0;
  int64_t t0 = 0, nc = 0;
  uint32_t max_nodes = 1;  // the chunk's largest tree (bounds the untracked values: SR_TRACK_LITE)
  hipStream_t cs = nullptr;
  SrProgramBatch<T> pc;
  int depth = 1;
  size_t ncode = 0;
  int64_t n_vs = 0;  // launch positions [0, n_vs) -> register-stack kernel
  Grid g_vs, g_ls;   // the grids of its two launches: [0, n_vs) at Rv, [n_vs, nc) at R — the deal's, the
                     // segments' and the launch's alike
  int n_seg = 0;
  int64_t seg_blocks = 0;
};

#define SR_STAGE(expr)           \
  do {                           \
    const int _rc = (expr);      \
    if (_rc != SR_OK) return _rc; \
  } while (0)

// One call's state, written by the stages in order, and the stages (run() calls them).
template <typename T>
struct BatchCall {
  // the inputs: the request, what the caller wants, and where the merged program summary and the results go
  sr_ctx* ctx;
  const EvalReq& req;
  const BatchWants& want;
  SrProgramBatch<T>* prog;
  BatchResult* res;
  // the last-call record this run writes: the context's, or — an internal pass — a scratch copy
  sr_ctx::LastCall scratch;
  sr_ctx::LastCall& last;
  bool allow_derived;  // (want.allow_derived until a stage withdraws it: several views, an expression loss, parameters)
  BatchCall(sr_ctx* c, const EvalReq& q, const BatchWants& w, SrProgramBatch<T>* p, BatchResult* r)
      : ctx(c), req(q), want(w), prog(p), res(r), last(w.internal ? scratch : c->last), allow_derived(w.allow_derived) {}
  void mark_phase(int i) {
    if (!want.internal) ctx->mark_phase(i);
  }
  // validate_call: the view, the decoded loss, the batch's size
  bool gather = false, multi = false;
  int64_t n_eval = 0, n_rows_up = 0, nt = 0, total_nodes = 0;
  int mrb = 0, lkind = 0;  // (mrb: the row-block bound of the call's grids)
  double lparam = 0.0;
  const sr_ctx::LossExpr* lexpr = nullptr;  // an expression-loss call's registered loss (plain LOSS calls only)
  // stage_param_table: a parametric call's table facts (nfk: the X rows a launch stages)
  const sr_param_batch* pb = nullptr;
  bool parametric = false;
  int nfk = 0;
  int64_t p_stride = 0;
  double max_abs_p = 0.0;
  // choose_kernels: tier, rows per lane (classic R, register-stack Rv or 0), waves; the build request of the
  // call's launches (each launch sets its own R, waves, stack and view); every grid's spec; row blocks the
  // partial buffers hold per tree (the most any kernel uses); the chunks
  int tier = 0, R = 0, W = 0, Rv = 0, n_rb = 1, n_chunks = 1;
  SrBuildRequest breq;
  GridSpec gs;
  Grid g_ls, g_vs;  // the whole batch's grids at R (depth 1) and, Rv > 0, at Rv (depth 0)
  Grid glast;       // the last launch's (BatchResult::grid)
  // bind_buffers: the staging image's layout, its device and pinned copies, the partials' count
  ProgImage img;
  size_t n_part = 0;
  char *dprog = nullptr, *hprog = nullptr;
  SrIns<T>* h_code = nullptr;
  uint32_t *h_off = nullptr, *h_perm = nullptr, *h_end = nullptr;
  uint8_t* h_bad = nullptr;
  // plan_fold / bind_outputs / prepare_hints
  int64_t fold_n_terms = 0;
  FoldPlan fold;
  bool fold_cand = false, fold_compact = false, loss_compact = false;
  // plan_chunks: the chunks' bounds
  ChunkPlan cplan;
  bool early = false;  // the flags go to pinned memory behind the last chunk's reduce (sr_ctx::exact_early)
  bool host_out = false, fold_mirror = false, host_red = false, use_hint = false, use_probe = false, stress_probe = false;
  // launch_derived: the derived-column spec and map, the columns' leading dimension, the call's leaf bound
  std::vector<int16_t> dmap;
  SrDerivedSpec spec{};
  int64_t dld = 0;
  double max_abs_x = 0.0;
  // the chunks
  FoldJob<T> fjob;  // (the regions of the chunk being launched; a row-sharded call's: all of them, kept)
  size_t fold_store_at = 0;  // (stored losses: the regions one after another, [position][n_rb x rb rows])
  T* d_fval = nullptr;
  int32_t* d_fst = nullptr;
  uint32_t code_base = 0;
  std::chrono::steady_clock::time_point t_pre;
  std::string err;
  hipStream_t s = nullptr;
  bool in_flight = false;  // the call has enqueued asynchronous work: an error exit joins both streams

  // the largest leaf value of the call, as the deferred checks bound it
  double leaf_bound(double max_abs_x_data) const { return parametric ? std::max(max_abs_x_data, max_abs_p) : max_abs_x_data; }
  // Σ over n_total rows of values below tbig cannot overflow T, even with rounding slack.
  T tbig() const { return T(t_max<T>() / (2.0 * double(want.n_total > 0 ? want.n_total : 1))); }

  // The view, the row-block bound, the loss and the batch's size.
  int validate_call() {
    gather = req.gather();
    // PRED passes (the fold's few band trees) write no partials: more row blocks fill the GPU (C4's 14 trees
    // x 2^26 rows ran 1,024 workgroups at 256)
    mrb = want.mode == SR_MODE_PRED ? std::max(ctx->max_row_blocks, 4096) : ctx->max_row_blocks;
    n_eval = req.n_eval();
    if (n_eval <= 0) return set_error(SR_ERR_INVALID_ARG, "no rows to evaluate");
    // under the in-order fold, row blocks of at most fold_seg_max rows on the largest shard (every rank
    // the same count): a slow block's rows are kept whole (C4's 2^26 rows per GPU: 4,096 blocks of 16k)
    if (want.mode == SR_MODE_LOSS && want.fold && ctx->ref_fold && sizeof(T) == 4 && ctx->fold_seg_max > 0 &&
        (want.shard ? want.n_total : n_eval) <= ctx->fold_rows_max) {
      const int64_t max_rows = want.shard ? sr_max_shard_rows(req.ds->shard_offs, n_eval) : n_eval;
      const int64_t need = (max_rows + ctx->fold_seg_max - 1) / ctx->fold_seg_max;
      if (need > mrb) mrb = int(std::min<int64_t>(need, 16384));
    }
    // several views: one launch, its tree groups view-pure (SrSegment); rows uploaded for every view
    multi = req.views != nullptr && gather && want.mode == SR_MODE_LOSS;
    n_rows_up = multi ? int64_t(req.views->n_views) * req.n_idx : req.n_idx;
    if (multi) allow_derived = false;
    // (expression losses: the calls that ask for them, BatchWants::takes_expr — plain single-context LOSS calls;
    //  the sharded, partials and parametric calls pass no slot and are refused with the message that names the
    //  restriction)
    if (decode_loss(ctx, req.loss_kind, &lkind, &lparam, want.takes_expr ? &lexpr : nullptr) != SR_OK)
      return SR_ERR_INVALID_ARG;
    if (check_loss_expr_weights(lexpr, req.ds) != SR_OK) return SR_ERR_INVALID_ARG;
    if (lexpr) allow_derived = false;  // (derived columns are chosen for the catalog builds: not measured here)
    nt = req.trees->n_trees;
    if (nt < 0) return set_error(SR_ERR_INVALID_ARG, "negative tree count");
    if (nt > 0 && !req.trees->offsets) return set_error(SR_ERR_INVALID_ARG, "sr_tree_batch has NULL arrays");
    total_nodes = nt > 0 ? req.trees->offsets[nt] - req.trees->offsets[0] : 0;
    if (total_nodes < 0 || total_nodes > int64_t(0xffffffffu) / 2)
      return set_error(SR_ERR_INVALID_ARG, "tree batch node count out of range");
    return SR_OK;
  }

  // A parametric call (EvalReq::params; the entry point has checked the batch against the dataset: check_params):
  // the table the kernels gather from, [tree][parameter][class] in T (each tree's Julia column-major matrix
  // transposed, so that one parameter's classes are contiguous),
  // staged in pinned memory here and uploaded by begin_programs; the leaf bound of the deferred checks
  // becomes max(max|X|, max|P|), Inf when any entry is non-finite (then, as for such data, the
  // per-node-check tier runs: DESIGN.md §4.6).  nfk: the X rows a launch stages (the hidden class row
  // included).
  int stage_param_table() {
    pb = req.params;
    parametric = pb != nullptr;
    nfk = int(req.ds->nf) + (parametric ? 1 : 0);
    if (!parametric) return SR_OK;
    const int64_t K = pb->max_parameters, NC = pb->n_classes;
    p_stride = K * NC;
    if (p_stride > int64_t(INT_MAX)) return set_error(SR_ERR_INVALID_ARG, "parameter matrix too large");
    const size_t bytes = size_t(std::max<int64_t>(nt, 1)) * size_t(std::max<int64_t>(p_stride, 1)) * sizeof(T);
    SR_HIP_CHECK(ctx->h_ptab.ensure(bytes, ctx->stream, ctx->stream2));
    SR_HIP_CHECK(ctx->ptab.ensure(bytes));
    T* hp = ctx->h_ptab.as<T>();
    const T* src = static_cast<const T*>(pb->parameters);
    bool bad = false;
    double mp = 0.0;
    for (int64_t t = 0; t < nt; ++t)
      for (int64_t c = 0; c < NC; ++c)
        for (int64_t k = 0; k < K; ++k) {
          const T v = src[size_t(t) * size_t(p_stride) + size_t(c * K + k)];
          hp[size_t(t) * size_t(p_stride) + size_t(k * NC + c)] = v;
          const double m = std::fabs(double(v));
          bad |= !std::isfinite(m);
          mp = m > mp ? m : mp;
        }
    max_abs_p = bad ? double(INFINITY) : mp;
    allow_derived = false;  // (derived columns are chosen for plain populations: not measured here)
    return SR_OK;
  }

  // The kernels of the call: the tier, rows per lane and waves; then every grid's spec, the row blocks of
  // the partial buffers and the chunk count.
  void choose_kernels() {
    // (SR_TRACK_LITE: the deferred-check kernels bound untracked values by L x max|x| for trees of up to
    //  L nodes; data at or above tbig / L — huge or non-finite values, never seen in practice — runs the
    //  per-node-check kernels instead, whose checks hold for any data)
    tier = ctx->tiers[req.opset_id];
#ifdef SR_TRACK_LITE
    if (tier == SR_TIER_BASIC && want.mode == SR_MODE_LOSS && nt > 0) {
      int64_t lmax = 1;
      for (int64_t t = 0; t < nt; ++t) lmax = std::max<int64_t>(lmax, req.trees->offsets[t + 1] - req.trees->offsets[t]);
      const double mx = leaf_bound(want.shard ? want.shard->max_abs_x : req.ds->max_abs_x);
      if (!(mx < double(tbig()) / double(lmax))) tier = SR_TIER_FULL;
    }
#endif
    // register-stack kernel (f32 BASIC loss over the full dataset): Rv rows per lane, used for every
    // chunk whose programs need <= 2 operand-stack slots (all trees of <= 30 nodes); other chunks run
    // the LDS-stack kernel at R rows per lane
    const SrBuildFamily family = parametric ? SR_FAMILY_PARAM : (lexpr ? SR_FAMILY_LOSSX : SR_FAMILY_PLAIN);
    const SrLaunchShape shape = sr_launch_shape(int(sizeof(T)), want.mode, tier, gather, family, n_eval, ctx->rows_override,
                                                ctx->waves_override, ctx->vstk_rows);
    R = shape.R;
    W = shape.W;
    Rv = shape.Rv;
    // (an expression-loss call's launches are plain ones whose loss kind is SR_LOSS_EXPR: sr_resolve_build)
    breq = SrBuildRequest{int(sizeof(T)), want.mode, gather, tier, R, W, false, lkind, parametric ? SR_FAMILY_PARAM : SR_FAMILY_PLAIN};
    // every grid of the call comes from this one spec
    gs = GridSpec{int(sizeof(T)), n_eval, W, nfk, req.ds->w != nullptr, ctx->tree_group, mrb};
    // a wide dataset whose register-stack tile (its rows per lane are twice the classic kernel's) would
    // not fit the LDS runs the classic kernel instead (Float64 with ~40-75 features)
    if (Rv > 0) {
      g_vs = gs.grid(nt > 0 ? nt : 1, Rv, 0);
      if (g_vs.lds > kLdsMax) Rv = 0;
    }
    last.rows = Rv > 0 ? Rv : R;  // (every C2-like tree fits the register stack)
    g_ls = gs.grid(nt > 0 ? nt : 1, R, 1);
    glast = g_ls;
    n_rb = g_ls.n_row_blocks;
    if (Rv > 0) n_rb = std::max(n_rb, g_vs.n_row_blocks);
  }

  // device + pinned buffers sized for the whole batch up front (a chunk's kernel may still run while
  // the next one is staged): a program has at most one instruction per node
  int bind_buffers() {
    s = ctx->stream;
    img = sr_prog_image(total_nodes, nt, sizeof(SrIns<T>), multi ? size_t(req.views->n_views) : 0);
    SR_HIP_CHECK(ctx->prog.ensure(img.bytes));
    SR_HIP_CHECK(ctx->h_prog.ensure(img.bytes, s, ctx->stream2));
    dprog = ctx->prog.as<char>();
    ctx->d_code = dprog;
    ctx->d_off = reinterpret_cast<uint32_t*>(dprog + img.o_off);
    ctx->d_bad = reinterpret_cast<uint8_t*>(dprog + img.o_bad);
    ctx->d_perm = reinterpret_cast<uint32_t*>(dprog + img.o_perm);
    ctx->d_end = reinterpret_cast<uint32_t*>(dprog + img.o_end);
    n_part = size_t(nt) * size_t(n_rb);
    SR_HIP_CHECK(ctx->part_sum.ensure(n_part * sizeof(double) + 8));
    SR_HIP_CHECK(ctx->part_flag.ensure(n_part * sizeof(uint32_t) + 4));
    return SR_OK;
  }

  // the reference's in-order loss fold of every complete tree (sr_ctx::ref_fold): the path (sr_fold_plan)
  // and its buffers
  // (a row-sharded call: the global rows and every shard's weights; its ranks fold or not together —
  //  the choice depends on the largest shard's rows, known to every rank)
  int plan_fold() {
    fold_n_terms = want.shard ? ((req.ds->w && req.ds->shard_w_min < 0.0) ? 0 : want.n_total)
                              : fold_terms(req.ds, n_eval, req.loss_kind);
    if (want.shard) ctx->fold_job.reset();
    if (want.fold && ctx->ref_fold && want.mode == SR_MODE_LOSS && nt > 0 && fold_n_terms > 0) {
      FoldPlanIn in;
      in.nt = nt;
      in.n_eval = n_eval;
      in.max_shard = want.shard ? sr_max_shard_rows(req.ds->shard_offs, n_eval) : n_eval;
      in.fold_len = want.shard ? want.n_total : n_eval;
      in.elem_size = int(sizeof(T));
      in.tier = tier;
      in.R = R;
      in.Rv = Rv;
      in.fold_store_mb = ctx->fold_store_mb;
      in.fold_slot_mb = ctx->fold_slot_mb;
      in.fold_seg_max = ctx->fold_seg_max;
      in.fold_rows_max = ctx->fold_rows_max;
      in.g_ls = g_ls;
      in.g_vs = g_vs;
      // NOT the call's spec: the largest shard's rows, and a row-block bound that follows fold_seg_max
      // whatever max_row_blocks says
      in.g_big = gs.over(in.max_shard, std::max<int64_t>(512, (in.max_shard + ctx->fold_seg_max - 1) /
                                                                     std::max<int64_t>(1, ctx->fold_seg_max)))
                     .grid(nt, R, 1);
      fold = sr_fold_plan(in);
      if (fold.path == 1) {
        SR_HIP_CHECK(ctx->fold_store.ensure(size_t(nt) * size_t(fold.pos_rows) * sizeof(T)));
      } else if (fold.path == 2) {
        SR_HIP_CHECK(ctx->fold_store.ensure(size_t(fold.slots) * size_t(fold.slot_rows) * sizeof(T)));
        SR_HIP_CHECK(ctx->fold_ctl.ensure(64));
        // the call's slot counter, and its (tree, block) pairs taken from the candidates / left to the FOLD pass
        SR_HIP_CHECK(hipMemsetAsync(ctx->fold_ctl.p, 0, 4 * sizeof(int), s));
      }
      if (fold.path && ctx->fold_stats) {
        SR_HIP_CHECK(ctx->fold_dbg.ensure(size_t(nt) * sizeof(int4) + 16));
        SR_HIP_CHECK(hipMemsetAsync(ctx->fold_dbg.p, 0, size_t(nt) * sizeof(int4), s));
      }
      if (fold.path) {
        SR_HIP_CHECK(ctx->fold_code.ensure(n_part * sizeof(int32_t) + 4));
        SR_HIP_CHECK(ctx->fold_tab.ensure(n_part * sizeof(typename SrFoldTab<T>::Pair) + 16));
        SR_HIP_CHECK(ctx->fold_sq.ensure(n_part * sizeof(int32_t) + 4));
        SR_HIP_CHECK(ctx->fold_tab2.ensure(n_part * sizeof(typename SrFoldTab<T>::Pair) + 16));
      }
    }
    // the candidate-composing loss launch (sr_ctx::fold_single_pass): plain calls only
    fold_cand = fold.path == 2 && ctx->fold_single_pass && sizeof(T) == 4 && tier == SR_TIER_BASIC && !gather &&
                !multi && !want.shard && !parametric && n_rb > 1;
    if (fold_cand) SR_HIP_CHECK(ctx->fold_cand.ensure(n_part * sizeof(int4) + 16));
    if (fold_cand && ctx->fold_cand_est) {  // every position's running prefix {sum | count}: none finished yet
      SR_HIP_CHECK(ctx->fold_est.ensure(size_t(nt) * (sizeof(double) + sizeof(uint32_t)) + 8));
      SR_HIP_CHECK(hipMemsetAsync(ctx->fold_est.p, 0, size_t(nt) * (sizeof(double) + sizeof(uint32_t)), s));
    }
    // the compacted FOLD launch (sr_ctx::fold_compact): plain calls only
    fold_compact = fold.path == 2 && ctx->fold_compact && !gather && !multi && !want.shard && !parametric;
    if (fold_compact) {
      SR_HIP_CHECK(ctx->fold_list.ensure(n_part * sizeof(int32_t) + 4));
      SR_HIP_CHECK(ctx->fold_wg.ensure(sr_fold_wg_words(n_rb) * sizeof(int32_t)));
    }
    // the listed loss launch (sr_ctx::loss_compact): the calls that take both of the above
    loss_compact = fold_compact && fold_cand && ctx->loss_compact && want.mode == SR_MODE_LOSS;
    if (loss_compact) SR_HIP_CHECK(ctx->loss_list.ensure(sr_loss_list_bytes(nt)));
    for (int c = 0; c < kMaxChunks; ++c) last.loss_listed_np[c] = 0;
    last.loss_list_nt = nt;
    last.loss_list_read = true;
    last.n_loss_listed_launches = last.n_loss_live = last.n_loss_excl = 0;
    for (int r = 0; r < 2 * kMaxChunks; ++r) {
      last.fold_wg_nrb[r] = 0;
      for (int k = 0; k < 4; ++k) last.fold_wg_info[r][k] = 0.0;
    }
    last.fold_wg_read = true;
    last.fold_path = res->fold_path = fold.path;
    last.fold_timed = false;
    last.fold_cand_read = fold.path != 2;
    last.n_cand_taken = last.n_cand_rerun = 0;
    return SR_OK;
  }

  // The chunks of the call (sr_plan.h), after the fold's path: a plain path-2 call whose loss launch composes
  // candidates takes the three-chunk schedule (sr_ctx::tail_chunk; a view below the register-stack kernel's
  // 2^17 rows has no such launch and keeps two chunks), every other call the two-chunk pipeline; and whether
  // the flags go back early (sr_ctx::exact_early).
  int plan_chunks() {
    cplan = sr_chunk_plan(nt, ctx->chunks, ctx->first_chunk, ctx->chunk_min, multi, want.mode,
                          fold_compact && fold_cand && Rv == 16 ? ctx->tail_chunk : 0);  // (Rv 16: launch_region's cand_launch)
    n_chunks = cplan.n;
    early = ctx->exact_early && want.early && fold.path != 0 && n_chunks > 1 && !multi && !want.shard && !parametric &&
            want.mode == SR_MODE_LOSS;
    if (early) SR_HIP_CHECK(ctx->need_stream3());
    res->early = early;
    return SR_OK;
  }

  // The call's results: {Σ loss | flags | the fold's values | their status}, one allocation (one DMA back),
  // on the device or — the latency path — in pinned host memory; the PRED rows.
  int bind_outputs() {
    ctx->outs_flag_off = sr_align256(size_t(nt) * sizeof(double) + 8);
    ctx->outs_fval_off = sr_align256(ctx->outs_flag_off + size_t(nt) * sizeof(uint32_t) + 4);
    ctx->outs_fst_off = sr_align256(ctx->outs_fval_off + size_t(nt) * sizeof(T) + 8);
    const size_t outs_bytes = ctx->outs_fst_off + size_t(nt) * sizeof(int32_t) + 4;
    ctx->outs_bytes_all = outs_bytes;
    SR_HIP_CHECK(ctx->outs.ensure(outs_bytes));
    // latency path (see host_io): results written to pinned host memory, programs read from it
    const bool small_call = n_chunks == 1 && want.mode == SR_MODE_LOSS;
    // (under the in-order fold the plan reads the call's flags and partials on the device; a stored-loss
    // fold of one row block of <= 256 rows — fold_tiny, the walk alone — reads and writes pinned memory)
    const bool fold_small = fold.path == 1 && n_rb == 1 && n_eval <= 256;
    host_out = small_call && ctx->host_io >= 1 && want.host_out && (fold.path == 0 || fold_small);
    // (other stored-loss folds of a small call: Σ and flags stay on the device for the pair kernel, and the
    //  walk copies them to pinned memory beside the fold's values — no copy back, SrFoldWho::msum)
    fold_mirror = small_call && ctx->host_io >= 1 && want.host_out && fold.path == 1 && !fold_small && !want.shard;
    if (host_out || fold_mirror || early) SR_HIP_CHECK(ctx->h_outs.ensure(outs_bytes, s, ctx->stream2));
    res->outs_on_host = host_out || fold_mirror;
    host_red = host_out && ctx->host_reduce > 0 && !multi && n_rb > 1 && int64_t(n_part) <= ctx->host_reduce;
    ctx->host_reductions.clear();
    ctx->host_red_rb = n_rb;
    if (host_red) SR_HIP_CHECK(ctx->h_part.ensure(n_part * (sizeof(double) + sizeof(uint32_t)) + 16, s, ctx->stream2));
    char* const sums_base = host_out ? ctx->h_outs.as<char>() : ctx->outs.as<char>();
    ctx->d_out_sum = reinterpret_cast<double*>(sums_base);
    ctx->d_out_flag = reinterpret_cast<uint32_t*>(sums_base + ctx->outs_flag_off);
    if (want.mode == SR_MODE_PRED) SR_HIP_CHECK(ctx->pred.ensure(size_t(nt) * size_t(n_eval) * sizeof(T) + 16));
    return SR_OK;
  }

  // Dead-tree hints (one word per launch position) and the probe's scratch partials.
  int prepare_hints() {
    use_hint = ctx->dead_hints && want.mode == SR_MODE_LOSS && n_rb > 1;  // (hints are per position)
    if (use_hint) {
      // epoch-tagged hints: each call marks dead positions with its own epoch, so the array needs a
      // reset only when (re)allocated or when the epoch counter wraps
      // (a reallocation is detected by the capacity, not the address: the allocator may hand back the
      // freed address for the larger buffer, whose new part then holds stale words — possibly equal to
      // this call's epoch, which would mark live trees dead)
      const size_t cap_before = ctx->hint.cap;
      const size_t hint_bytes = size_t(nt) * sizeof(uint32_t) + 4;
      if (ctx->debug_hint_regrow && hint_bytes > ctx->hint.cap) {
        // (tests: sr_set_tuning "debug_hint_regrow") the array grows IN PLACE, at the same address, its
        // new words holding the epoch the next call would use without a reset — the conditions of the
        // round-3 stale-hint bug (a reallocation that got the freed address back); only the capacity
        // check below catches it
        constexpr size_t kReserve = size_t(64) << 20;
        if (hint_bytes + hint_bytes / 4 > kReserve) return set_error(SR_ERR_INVALID_ARG, "debug_hint_regrow: batch too large");
        if (ctx->hint_reserve == nullptr) SR_HIP_CHECK(hipMalloc(&ctx->hint_reserve, kReserve));
        if (ctx->hint.p != ctx->hint_reserve) {
          ctx->hint.release();
          ctx->hint.p = ctx->hint_reserve;
        }
        // (word-aligned: an earlier ordinary allocation may have left an odd capacity)
        const size_t from = (cap_before + 3) & ~size_t(3);
        const size_t want = (hint_bytes + hint_bytes / 4 + 255) & ~size_t(255);
        SR_HIP_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(static_cast<char*>(ctx->hint.p) + from),
                                       int(ctx->hint_epoch + 1), (want - from) / 4, s));
        ctx->hint.cap = want;
      } else {
        if (ctx->hint.p == ctx->hint_reserve && ctx->hint_reserve != nullptr) {  // (leaving the debug mode)
          ctx->hint.p = nullptr;
          ctx->hint.cap = 0;
        }
        SR_HIP_CHECK(ctx->hint.ensure(hint_bytes));
      }
      if (ctx->hint.cap != cap_before || ctx->hint_epoch == 0xffffffffu) {
        SR_HIP_CHECK(hipMemsetAsync(ctx->hint.p, 0, ctx->hint.cap, s));
        ctx->hint_epoch = 0;
      }
      ++ctx->hint_epoch;
    }
    // dead-tree probe: the first kProbeTiles row tiles of the view, hints only (scratch partials)
    use_probe = use_hint && ctx->probe && n_rb >= 16 && !multi;  // (per chunk: its grid has >= 16 row blocks)
    if (use_probe) {
      SR_HIP_CHECK(ctx->probe_sum.ensure(size_t(nt) * kProbeTiles * sizeof(double) + 8));
      SR_HIP_CHECK(ctx->probe_flag.ensure(size_t(nt) * kProbeTiles * sizeof(uint32_t) + 4));
    }
    return SR_OK;
  }

  // The view's row indices and the views' tree map checked; the merged summary and the call's record reset;
  // the staging pointers bound; the call's first uploads (row indices, a parametric call's table).
  int begin_programs() {
    if (gather) {
      for (int64_t i = 0; i < n_rows_up; ++i)
        if (req.row_idx[i] < 0 || req.row_idx[i] >= req.ds->n)
          return set_error(SR_ERR_INVALID_ARG, "row index " + std::to_string(req.row_idx[i]) + " out of range");
      SR_HIP_CHECK(ctx->row_idx.ensure(size_t(n_rows_up) * sizeof(int64_t)));
    }
    if (multi)
      for (int64_t t = 0; t < nt; ++t)
        if (req.views->tree_view[t] < 0 || req.views->tree_view[t] >= req.views->n_views)
          return set_error(SR_ERR_INVALID_ARG, "tree " + std::to_string(t) + ": view index out of range");

    prog->code.clear();
    prog->offsets.assign(size_t(nt) + 1, 0);
    prog->static_bad.assign(size_t(nt), 0);
    prog->n_checks.assign(size_t(nt), 0);
    prog->max_depth = 0;
    prog->tier = tier;
    prog->max_checks = 0;
    prog->total_nodes = 0;
    prog->total_ops = 0;
    hprog = ctx->h_prog.as<char>();
    h_code = reinterpret_cast<SrIns<T>*>(hprog);
    h_off = reinterpret_cast<uint32_t*>(hprog + img.o_off);
    h_bad = reinterpret_cast<uint8_t*>(hprog + img.o_bad);
    h_perm = reinterpret_cast<uint32_t*>(hprog + img.o_perm);
    ctx->h_bad_last = h_bad;
    ctx->h_perm_last = h_perm;
    h_end = reinterpret_cast<uint32_t*>(hprog + img.o_end);
    last.n_chunks = 0;
    last.derived = false;
    last.n_derived = 0;
    last.timed = ctx->timing != 0 && !want.internal;  // (this run records its events)
    if (last.timed) SR_HIP_CHECK(hipEventRecord(ctx->ev_start, s));
    if (gather)
      SR_HIP_CHECK(hipMemcpyAsync(ctx->row_idx.p, req.row_idx, size_t(n_rows_up) * sizeof(int64_t), hipMemcpyHostToDevice,
                                  s));
    if (parametric && nt > 0 && p_stride > 0)  // (ahead of the chunks' join: both streams see the table)
      SR_HIP_CHECK(hipMemcpyAsync(ctx->ptab.p, ctx->h_ptab.p, size_t(nt) * size_t(p_stride) * sizeof(T), hipMemcpyHostToDevice, s));
    return SR_OK;
  }

  // derived columns (LOAD_DERIVED): for the BASIC-tier deferred-check loss kernels over many rows,
  // every unary(feature) node of a transcendental shared by several trees is evaluated once for the
  // call.  Chosen from a sample of the batch; not when the data itself needs tracked feature loads.
  int launch_derived() {
    dld = (n_eval + kRowAlign - 1) / kRowAlign * kRowAlign;
    // (row-sharded calls pass `shard`: the choice then depends only on the trees and on statistics of
    // every shard, so all ranks compile the same programs and number their checked arrays alike)
    max_abs_x = leaf_bound(want.shard ? want.shard->max_abs_x : req.ds->max_abs_x);
    const int64_t derived_rows = want.shard ? want.shard->min_rows : n_eval;
    // (and only for calls with enough work: the column pass is one more launch, which a search's small
    // calls — tens of trees x 1e5 rows — would pay in latency for nothing)
    if (allow_derived && ctx->derived && want.mode == SR_MODE_LOSS && tier == SR_TIER_BASIC &&
        derived_rows >= kDerivedMinRows && nt >= 64 && double(nt) * double(derived_rows) >= kDerivedMinWork &&
        max_abs_x < double(tbig())) {  // (track_x off)
      choose_derived(*req.trees, ctx->opsets[req.opset_id], req.ds->nf, &spec, &dmap);
      if (spec.n > 0) {
        SR_HIP_CHECK(ctx->derived_cols.ensure(size_t(spec.n) * size_t(dld) * sizeof(T)));
        if (last.timed) SR_HIP_CHECK(hipEventRecord(ctx->ev_d0, s));
        SR_HIP_CHECK(sr_launch_derived<T>(static_cast<const T*>(req.ds->X), req.ds->ld,
                                          gather ? ctx->row_idx.as<int64_t>() : nullptr, n_eval, dld, spec,
                                          ctx->derived_cols.as<T>(), dld, s));
        if (last.timed) SR_HIP_CHECK(hipEventRecord(ctx->ev_d1, s));
        last.derived = true;
        last.n_derived = spec.n;
      } else {
        dmap.clear();
      }
    }
    // the probe over the dataset's stress rows (full views only: a gathered view's rows are its own);
    // its LOAD_DERIVED nodes read columns computed over those rows
    stress_probe = use_probe && !gather && req.ds->probe_rows != nullptr && ctx->stress_probe;
    if (stress_probe && !dmap.empty()) {
      SR_HIP_CHECK(ctx->probe_derived.ensure(size_t(spec.n) * size_t(kProbeRows) * sizeof(T)));
      SR_HIP_CHECK(sr_launch_derived<T>(static_cast<const T*>(req.ds->X), req.ds->ld,
                                        static_cast<const int64_t*>(req.ds->probe_rows), req.ds->n_probe, kProbeRows, spec,
                                        ctx->probe_derived.as<T>(), kProbeRows, s));
    }
    return SR_OK;
  }

  // The second stream joins the shared setup; the fold's launch facts.
  // the fold's launches per chunk: every launch of the chunk, then its plan / tables / FOLD pass / walk
  int begin_chunks() {
    if (n_chunks > 1) {  // odd chunks run on the second stream, after the shared setup above
      SR_HIP_CHECK(ctx->need_stream2());
      SR_HIP_CHECK(hipEventRecord(ctx->ev_join, s));
      SR_HIP_CHECK(hipStreamWaitEvent(ctx->stream2, ctx->ev_join, 0));
    }
    fjob.path = fold.path;
    fjob.tier = tier;
    fjob.gather = gather;
    fjob.n_eval = n_eval;
    fjob.n_rb = n_rb;
    fjob.slot_rows = fold.slot_rows;
    fjob.n_terms = fold_n_terms;
    fjob.delta = std::ldexp(1.0, -ctx->fold_delta_log2);
    // stored losses on one GPU: the pair kernel reduces the partials itself (one launch fewer a call)
    fjob.fuse_reduce = fold.path == 1 && !want.shard && want.mode == SR_MODE_LOSS;
    fjob.slot_cap = fold.path == 2
                        ? int(std::min<int64_t>({int64_t(INT_MAX / 2), fold.slot_budget,
                                                 int64_t(ctx->fold_store.cap / (size_t(fold.slot_rows) * sizeof(T)))}))
                        : 0;
    char* const outs_base = (host_out || fold_mirror) ? ctx->h_outs.as<char>() : ctx->outs.as<char>();
    d_fval = reinterpret_cast<T*>(outs_base + ctx->outs_fval_off);
    d_fst = reinterpret_cast<int32_t*>(outs_base + ctx->outs_fst_off);
    t_pre = std::chrono::steady_clock::now();
    return SR_OK;
  }

  // Chunk c's bounds, stream and compiled programs.
  int compile_chunk(BatchChunk<T>& ch) {
    static const bool phase_debug = std::getenv("SR_AMD_PHASE_DEBUG") != nullptr;  // (latency analysis)
    const int64_t t0 = ch.t0 = cplan.bound[ch.c];
    const int64_t nc = ch.nc = cplan.bound[ch.c + 1] - t0;
    for (int64_t t = t0; t < t0 + nc; ++t)
      ch.max_nodes = std::max<uint32_t>(ch.max_nodes, uint32_t(req.trees->offsets[t + 1] - req.trees->offsets[t]));
    // chunks alternate between two streams: chunk c+1's workgroups fill the GPU while chunk c drains
    ch.cs = (ch.c & 1) ? ctx->stream2 : s;
    sr_tree_batch sub = *req.trees;
    sub.n_trees = nc;
    sub.offsets = req.trees->offsets + t0;  // node arrays stay indexed by absolute offsets
    ch.pc.keep_pieces = true;  // (staged below straight from the compile workers' buffers)
    // (a parametric batch's per-node arrays are indexed by absolute node offsets, like the tree batch's)
    const SrParamNodes pnodes{parametric ? pb->is_parameter : nullptr, parametric ? pb->parameter : nullptr,
                              parametric ? pb->max_parameters : 0};
    const int rc = sr_compile_batch<T>(sub, ctx->opsets[req.opset_id], want.n_total, req.ds->nf, false, &ch.pc, &err,
                                       dmap.empty() ? nullptr : dmap.data(), parametric ? &pnodes : nullptr);
    if (rc != SR_OK) {
      if (rc == SR_ERR_BAD_TREE || rc == SR_ERR_INVALID_ARG) {
        // report the tree index of the whole batch
        const size_t at = err.find("tree ");
        if (at == 0) {
          const int64_t k = std::atoll(err.c_str() + 5);
          err = "tree " + std::to_string(k + t0) + err.substr(err.find(':'));
        }
      }
      return set_error(rc, err);
    }
    if (ch.c == 0) {
      if (phase_debug) {
        const auto now = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[sr phase] trees %lld chunks %d: setup %.3f ms, compile of chunk 0 (%lld trees) %.3f ms\n",
                     (long long)nt, n_chunks, std::chrono::duration<double, std::milli>(t_pre - ctx->phase_t).count(),
                     (long long)nc, std::chrono::duration<double, std::milli>(now - t_pre).count());
      }
      mark_phase(0);
    }
    ch.depth = ch.pc.max_depth > 0 ? ch.pc.max_depth : 1;
    ch.ncode = ch.pc.n_code;
    return SR_OK;
  }

  // The chunk's launch plan (sr_plan.h) and its staging image: code at code_base, offsets made absolute,
  // static_bad, launch order (chunk-local), view segments.
  int order_and_stage(BatchChunk<T>& ch) {
    const SrProgramBatch<T>& pc = ch.pc;
    const int64_t t0 = ch.t0, nc = ch.nc;
    ch.n_vs = sr_count_vstk(pc.depth.data(), nc, Rv > 0);
    // the chunk's two launches: the register-stack trees, then the deeper ones on the LDS-stack kernel
    if (ch.n_vs > 0) ch.g_vs = gs.grid(ch.n_vs, Rv, 0);
    if (ch.n_vs < nc) ch.g_ls = gs.grid(nc - ch.n_vs, R, ch.depth);
    if (code_base + ch.ncode > img.code_cap) return set_error(SR_ERR_INVALID_ARG, "program longer than its node count");
    std::memcpy(h_bad + t0, pc.static_bad.data(), size_t(nc));
    uint32_t* const perm = h_perm + t0;
    sr_launch_order(pc.cost.data(), pc.depth.data(), nc, multi ? req.views->tree_view + t0 : nullptr,
                    multi ? req.views->n_views : 0, ctx->cost_order, ctx->balance_groups, Rv > 0,
                    GroupShape{ch.g_vs.G, ch.g_vs.n_groups}, GroupShape{ch.g_ls.G, ch.g_ls.n_groups}, perm);
    uint32_t* const off = h_off + t0;
    uint32_t* const end = h_end + t0;
    sr_code_layout(perm, pc.offsets.data(), nc, code_base, off, end);
    // the copies into the pinned staging buffer: a large chunk's ~2 MB on the compile workers
    // (single-threaded they sat on the host path between the first chunk's launch and the second's)
    auto copy = [&](int64_t p0, int64_t p1) {
      for (int64_t p = p0; p < p1; ++p) {
        const uint32_t i = perm[p];
        const uint32_t len = end[i] - off[i];
        if (len) std::memcpy(h_code + off[i], pc.tree_code(i), size_t(len) * sizeof(SrIns<T>));
      }
    };
    constexpr int64_t kCopyPiece = 512;
    if (nc >= 4 * kCopyPiece) {
      sr_parallel_for(int((nc + kCopyPiece - 1) / kCopyPiece), [&](int w) {
        const int64_t p0 = int64_t(w) * kCopyPiece;
        copy(p0, std::min<int64_t>(nc, p0 + kCopyPiece));
      });
    } else {
      copy(0, nc);
    }
    // (several views: Rv = 0, so the one launch's grid is g_ls)
    if (multi && nc > 0)
      ch.seg_blocks = sr_view_segments(req.views->tree_view + t0, perm, nc, ch.g_ls.G, ch.g_ls.n_row_blocks, req.n_idx,
                                       reinterpret_cast<SrSegment*>(hprog + img.o_seg), &ch.n_seg);
    return SR_OK;
  }

  // The chunk's programs to the device, and its part of the merged summary.
  int upload_chunk(BatchChunk<T>& ch) {
    const SrProgramBatch<T>& pc = ch.pc;
    const int64_t t0 = ch.t0, nc = ch.nc;
    hipStream_t cs = ch.cs;
    if (n_chunks == 1) {  // the whole staging image (code, offsets, static_bad, order): one DMA
      const size_t used = multi ? img.o_seg + size_t(ch.n_seg) * sizeof(SrSegment) : img.o_end + size_t(nc) * sizeof(uint32_t);
      SR_HIP_CHECK(hipMemcpyAsync(dprog, hprog, used, hipMemcpyHostToDevice, cs));
    } else {
      if (ch.ncode)
        SR_HIP_CHECK(hipMemcpyAsync(static_cast<SrIns<T>*>(ctx->d_code) + code_base, h_code + code_base,
                                    ch.ncode * sizeof(SrIns<T>), hipMemcpyHostToDevice, cs));
      SR_HIP_CHECK(hipMemcpyAsync(ctx->d_off + t0, h_off + t0, size_t(nc) * sizeof(uint32_t), hipMemcpyHostToDevice, cs));
      SR_HIP_CHECK(hipMemcpyAsync(ctx->d_end + t0, h_end + t0, size_t(nc) * sizeof(uint32_t), hipMemcpyHostToDevice, cs));
      SR_HIP_CHECK(hipMemcpyAsync(ctx->d_bad + t0, h_bad + t0, size_t(nc), hipMemcpyHostToDevice, cs));
      SR_HIP_CHECK(hipMemcpyAsync(ctx->d_perm + t0, h_perm + t0, size_t(nc) * sizeof(uint32_t), hipMemcpyHostToDevice, cs));
    }
    // merged summary
    for (int64_t i = 0; i < nc; ++i) prog->offsets[size_t(t0 + i)] = h_off[t0 + i];  // (starts; ends: h_end)
    std::memcpy(prog->static_bad.data() + t0, pc.static_bad.data(), size_t(nc));
    std::copy(pc.n_checks.begin(), pc.n_checks.end(), prog->n_checks.begin() + t0);
    if (pc.max_depth > prog->max_depth) prog->max_depth = pc.max_depth;
    if (pc.max_checks > prog->max_checks) prog->max_checks = pc.max_checks;
    prog->total_nodes += pc.total_nodes;
    prog->total_ops += pc.total_ops;
    return SR_OK;
  }

  // The argument blocks of one launch over launch positions [p0, p0 + np) of the chunk; its partials
  // occupy [n_rb][np] words from p0 * n_rb (the chunk's region holds n_rb rows for every position).
  // out_sum (the reduce's routing), segs and fold_cand are the launch's own (launch_region).
  void fill_region_args(const BatchChunk<T>& ch, int64_t p0, int64_t np, bool vstk, const Grid& g, SrEvalArgs<T>* out) {
    const int64_t t0 = ch.t0;
    const int Rc = vstk ? Rv : R;
    SrEvalArgs<T>& a = *out = SrEvalArgs<T>{};
    a.code = static_cast<const SrIns<T>*>(ctx->d_code);
    a.offsets = ctx->d_off + t0;
    a.ends = ctx->d_end + t0;
    a.perm = ctx->d_perm + t0 + p0;
    a.hint = use_hint ? ctx->hint.as<uint32_t>() + t0 + p0 : nullptr;
    a.hint_epoch = ctx->hint_epoch;
    a.n_trees = int(np);
    a.trees_per_block = g.G;
    a.X = static_cast<const T*>(req.ds->X);
    a.y = static_cast<const T*>(req.ds->y);
    a.w = static_cast<const T*>(req.ds->w);
    a.row_idx = gather ? ctx->row_idx.as<int64_t>() : nullptr;
    a.ld = req.ds->ld;
    a.derived = dmap.empty() ? nullptr : ctx->derived_cols.as<T>();
    a.dld = dld;
    a.n_rows = n_eval;
    a.nf = nfk;
    if (parametric) {  // (the chunk's rows of the table: the kernel indexes it by the chunk-local tree index)
      a.ptab = ctx->ptab.as<T>() + size_t(t0) * size_t(p_stride);
      a.p_stride = int(p_stride);
      a.n_classes = int(pb->n_classes);
    }
    a.tiles_per_block = g.tiles;
    a.n_row_blocks = g.n_row_blocks;
    a.n_groups = g.n_groups;
    a.stack_depth = vstk ? std::min(ch.depth, SR_VSTK_SLOTS) : ch.depth;  // (the register-stack trees need <= SR_VSTK_SLOTS)
    a.tbig = tbig();
    {  // the view's padded rows over every shard: n_total + at most one 2048-row tile of padding per shard
      const double padded = double(want.n_total > 0 ? want.n_total : 1) + 2048.0 * double(want.shard ? ctx->comm_ranks : 1);
      a.big_budget = 64.0 * (t_max<T>() / (1.01 * padded));  // (f64: 64 x DBL_MAX alone is +Inf)
    }
    a.track_x = !(max_abs_x < double(a.tbig)) ? 1 : 0;
#ifdef SR_TRACK_LITE
    if (want.mode == SR_MODE_LOSS && tier == SR_TIER_BASIC) {
      // (the deferred-check kernels leave +, - of stack values / features and cos, sin, neg, abs,
      //  sqrt untracked: such a value is at most L x max(tracked max, max|x|, 1) for a tree of L
      //  nodes, so with tbig / L as the tracked threshold every value stays below tbig, and a tile
      //  within budget / L - 64 (max|x| + 1) keeps every array's sum within the original budget;
      //  max|x| < tbig / L here: larger data took the per-node-check tier in choose_kernels)
      const double L = double(std::max<uint32_t>(1u, ch.max_nodes));
      a.tbig = T(double(a.tbig) / L);
      a.big_budget = a.big_budget / L - 64.0 * (max_abs_x + 1.0);
      a.track_x = 0;
    }
#endif
    a.loss_kind = lkind;
    a.loss_param = T(lparam);
    if (lexpr) {
      const SrLossProgArgs<T> lx = lexpr->template args<T>();
      a.lx_code = lx.code;
      a.lx_n = lx.n;
    }
    a.part_sum = (host_red ? ctx->h_part.as<double>() : ctx->part_sum.as<double>()) + size_t(n_rb) * size_t(t0 + p0);
    a.part_flag = (host_red ? reinterpret_cast<uint32_t*>(ctx->h_part.as<double>() + n_part)
                              : ctx->part_flag.as<uint32_t>()) + size_t(n_rb) * size_t(t0 + p0);
    a.pred = ctx->pred.as<T>();
    a.pred_ld = n_eval;
    if (fold.path == 1) {  // (small calls under the in-order fold: every live tree's losses, [position][rows])
      a.fold_pos_stride = int64_t(g.n_row_blocks) * int64_t(g.tiles) * 64 * Rc;
      a.fold_loss = ctx->fold_store.as<T>() + fold_store_at;
      fold_store_at += size_t(np) * size_t(a.fold_pos_stride);
    }
    // LDS program cache (register-stack launches: 4 workgroups per CU leave ~36 KiB of dynamic LDS
    // each): sized for the longest group span of this launch, capped by that budget (groups longer
    // than the cap stream their windows from global memory)
    a.code_lds = 0;
    // (round 4's cache in the classic launches too — code_cache 2 — was measured without payoff and
    //  removed in round 6)
    const size_t code_budget = vstk ? kCodeCacheLds : 0;
    if (want.mode == SR_MODE_LOSS && ctx->code_cache && size_t(g.lds) < code_budget) {
      const int64_t maxspan = sr_max_group_span(h_perm + t0, h_off + t0, h_end + t0, p0, np, g.G, g.n_groups);
      const int64_t cap = int64_t((code_budget - size_t(g.lds)) / 16);
      a.code_lds = int(std::min(maxspan, cap));
      if (a.code_lds < 64) a.code_lds = 0;
    }
  }

  // The dead-tree probe of a launch, from the launch's own arguments.
  // Trees that are non-finite on the first rows are flagged before the main launch, so its
  // workgroups skip them from their first tile (without the probe, the ~16 row blocks that
  // start together evaluate every such tree in full before a hint exists).  Only hints come
  // out of it: a tree non-finite on some rows of the view is incomplete on the whole view.
  // a wide, short grid: 16 trees x 1 tile per workgroup, kProbeTiles row blocks; always the
  // classic kernel at R rows per lane (a register-stack launch's 2x longer tiles would double the
  // probe's work for the same verdicts: C2's dead trees 0.88 -> 0.6x ms)
  int launch_probe(const BatchChunk<T>& ch, const SrEvalArgs<T>& a, int64_t np, const Grid& g) {
    SrEvalArgs<T> pa = a;
    pa.fold_loss = nullptr;  // (its rows are the stress rows; the main launch stores the view's)
    pa.stack_depth = ch.depth;
    pa.out_sum = nullptr;
    pa.out_flag = nullptr;
    pa.code_lds = 0;  // (its groups differ from the main launch's)
    pa.stamps = nullptr;
    pa.trees_per_block = std::max(16, g.W);
    pa.n_groups = int((np + pa.trees_per_block - 1) / pa.trees_per_block);
    pa.tiles_per_block = 1;
    pa.n_row_blocks = kProbeTiles;
    pa.n_rows = std::min<int64_t>(n_eval, int64_t(kProbeTiles) * 64 * R);
    pa.part_sum = ctx->probe_sum.as<double>();
    pa.part_flag = ctx->probe_flag.as<uint32_t>();
    if (stress_probe) {  // the stress rows first (sr_dataset::probe_rows), through the gather build
      pa.row_idx = static_cast<const int64_t*>(req.ds->probe_rows);
      pa.n_rows = std::min<int64_t>(req.ds->n_probe, int64_t(kProbeTiles) * 64 * R);
      if (!dmap.empty()) {
        pa.derived = ctx->probe_derived.as<T>();
        pa.dld = kProbeRows;
      }
    }
    SrBuildRequest q = breq;  // (the classic kernel at the call's R and W)
    q.gather = gather || stress_probe;
    SR_HIP_CHECK(sr_launch_eval<T>(pa, q, pa.n_groups * kProbeTiles, ch.cs));
    return SR_OK;
  }

  // One launch of the chunk: its probe, the kernel for it, and its partials' reduce — in the launch, by a
  // reduce launch, by the fold's pair kernel or (host_red) by the host after the call's synchronisation.
  int launch_region(const BatchChunk<T>& ch, int64_t p0, int64_t np, bool vstk) {
    const int64_t t0 = ch.t0;
    hipStream_t cs = ch.cs;
    const int Rc = vstk ? Rv : R;
    const Grid& g = vstk ? ch.g_vs : ch.g_ls;
    if (g.lds > kLdsMax)
      return set_error(SR_ERR_TOO_DEEP, "the row tile (" + std::to_string(req.ds->nf) + " features, " +
                                            std::to_string(ch.depth) + " stack slots) needs " + std::to_string(g.lds) +
                                            " bytes of LDS; the limit is 160 KiB");
    if (g.n_blocks > 0x7fffffff || g.n_row_blocks > n_rb) return set_error(SR_ERR_INVALID_ARG, "grid too large");
    glast = g;
    SrEvalArgs<T> a;
    fill_region_args(ch, p0, np, vstk, g, &a);
    int64_t n_blocks = g.n_blocks;
    if (multi) {  // (one launch over the whole chunk: the segments order_and_stage computed)
      a.segs = reinterpret_cast<const SrSegment*>(dprog + img.o_seg);
      a.n_segs = ch.n_seg;
      n_blocks = ch.seg_blocks;
      if (n_blocks > 0x7fffffff) return set_error(SR_ERR_INVALID_ARG, "grid too large");
    }
    const bool direct = want.mode == SR_MODE_LOSS && g.n_row_blocks == 1;
    if (direct) {  // the interpreter writes the final per-tree values; no reduce launch
      a.out_sum = ctx->d_out_sum + t0;
      a.out_flag = ctx->d_out_flag + t0;
      a.static_bad = ctx->d_bad + t0;
    }
    // mode 2 (default): every chunk after the first (its probe overlaps the first chunk's kernel),
    // and a single-chunk call when it is large (>= 512 trees x 2^18 rows: the tree-sharding share,
    // 1,250 trees x 1M rows, 1.09 -> 1.01 ms; the search's small calls pay the probe's launch and
    // keep none: profiles/r05_ab_probe.txt)
    // (round 5, later: also the first of two chunks when it is that large — C4's 8M-row shard
    //  216.9 -> 214.4 ms per call, C2 unchanged; tools/c4_shard_probe.py, profiles/r05_ab_c4_shard.txt)
    const bool probe_first = ch.nc >= 512 && n_eval >= (int64_t(1) << 18);
    const bool probed = use_probe && p0 == 0 && g.n_row_blocks >= 16 && (ctx->probe != 2 || ch.c > 0 || probe_first);
    if (probed) SR_STAGE(launch_probe(ch, a, np, g));
#ifdef SR_STAMPS
    ctx->n_stamps = g.n_blocks * g.W * SR_NSTAMPS;
    SR_HIP_CHECK(ctx->stamps.ensure(size_t(ctx->n_stamps) * sizeof(uint64_t)));
    SR_HIP_CHECK(hipMemsetAsync(ctx->stamps.p, 0, size_t(ctx->n_stamps) * sizeof(uint64_t), cs));
    a.stamps = ctx->stamps.as<uint64_t>();
#endif
    // (the register-stack launch at 16 rows per lane has the candidate build; the LDS-stack launch's few
    //  deep trees take the whole FOLD pass)
    const bool cand_launch = fold_cand && vstk && Rc == 16 && g.W == 4 && g.n_row_blocks > 1;
    if (cand_launch) a.fold_cand = ctx->fold_cand.as<int4>() + size_t(n_rb) * size_t(t0 + p0);
    if (cand_launch && ctx->fold_cand_est) {  // (plan_fold zeroed them)
      a.fold_est_sum = ctx->fold_est.as<double>() + t0 + p0;
      a.fold_est_cnt = reinterpret_cast<uint32_t*>(ctx->fold_est.as<double>() + nt) + t0 + p0;
      a.fold_est_min = uint32_t(ctx->fold_cand_est_min);
    }
    // the listed launch (sr_ctx::loss_compact): the candidate launch of a region whose probe has just run on
    // this stream, reduced by a reduce launch; the list from the hints as the probe left them
    const bool listed = loss_compact && cand_launch && probed && !direct && !host_red && !fjob.fuse_reduce &&
                        !parametric && !multi;
    uint8_t* excl = nullptr;
    if (listed) {
      char* const lb = ctx->loss_list.as<char>();
      int32_t* const list = reinterpret_cast<int32_t*>(lb) + t0 + p0;
      int32_t* const cnt = reinterpret_cast<int32_t*>(lb + sr_loss_list_cnt_off(nt)) + ch.c * kLossListCnt;
      excl = reinterpret_cast<uint8_t*>(lb + sr_loss_list_excl_off(nt)) + t0 + p0;
      SR_HIP_CHECK(sr_launch_loss_compact(a.hint, a.hint_epoch, int(np), a.perm, ctx->d_bad + t0, g.G, g.n_groups,
                                          ctx->loss_list_groups, list, cnt, excl, cs));
      a.fold_list = list;
      a.fold_cnt = cnt;
      // (a listed group's span takes in the excluded programs between its trees: the whole cache budget, and
      //  the kernel's own test per workgroup)
      if (a.code_lds > 0) a.code_lds = int((kCodeCacheLds - size_t(g.lds)) / 16);
      last.loss_listed_np[ch.c] = np;
      last.loss_list_read = false;
    }
    SrBuildRequest q = breq;
    q.R = Rc;
    q.waves = g.W;
    q.vstk = vstk;
    if (cand_launch) q.family = SR_FAMILY_CAND;  // (never a parametric call's: fold_cand)
    SR_HIP_CHECK(sr_launch_eval<T>(a, q, int(n_blocks), cs));
    if (fold.path) fjob.regions.push_back({a, t0, t0 + p0, np, n_blocks, Rc, vstk, g, fold_compact ? sr_fold_region(ch.c, vstk) : -1});
    if (!direct && host_red)
      ctx->host_reductions.push_back({t0 + p0, np, g.n_row_blocks});
    else if (listed)
      SR_HIP_CHECK(sr_launch_reduce_excl(a.part_sum, a.part_flag, int(np), g.n_row_blocks, a.perm, ctx->d_bad + t0, excl,
                                         ctx->d_out_sum + t0, ctx->d_out_flag + t0, cs));
    else if (!direct && !fjob.fuse_reduce)
      SR_HIP_CHECK(sr_launch_reduce(a.part_sum, a.part_flag, int(np), g.n_row_blocks, a.perm, ctx->d_bad + t0,
                                    ctx->d_out_sum + t0, ctx->d_out_flag + t0, cs));
    return SR_OK;
  }

  // the in-order fold of this chunk's complete trees (sr_aux.hip): the launches' partials and flags
  // are final here (reduce / direct write ran on this stream)
  int fold_chunk(const BatchChunk<T>& ch) {
    hipStream_t cs = ch.cs;
    if (last.timed) SR_HIP_CHECK(hipEventRecord(ctx->ev_fc0[ch.c], cs));
    SrFoldWho who{ctx->d_out_sum, ctx->d_out_flag, fold_n_terms, nullptr, nullptr, 1};
    if (fold_mirror) {
      who.msum = ctx->h_outs.as<double>();
      who.mflag = reinterpret_cast<uint32_t*>(ctx->h_outs.as<char>() + ctx->outs_flag_off);
    }
    for (const FoldRegion<T>& fr : fjob.regions) {
      SR_STAGE(fold_steps<T>(ctx, fjob, fr, who, cs));
      SR_STAGE(fold_walk<T>(ctx, fjob, fr, who, nullptr, d_fval, d_fst, cs));
    }
    fjob.regions.clear();
    if (last.timed) {
      SR_HIP_CHECK(hipEventRecord(ctx->ev_fc1[ch.c], cs));
      last.fold_timed = true;
    }
    return SR_OK;
  }

  // Chunk c of the call: compile, order and stage, upload, launch each region, fold.
  int run_chunk(int c) {
    BatchChunk<T> ch;
    ch.c = c;
    SR_STAGE(compile_chunk(ch));
    SR_STAGE(order_and_stage(ch));
    SR_STAGE(upload_chunk(ch));
    if (last.timed) SR_HIP_CHECK(hipEventRecord(ctx->ev_c0[c], ch.cs));  // the chunk's kernel time includes its probe
    if (ch.n_vs > 0) SR_STAGE(launch_region(ch, 0, ch.n_vs, true));
    if (ch.n_vs < ch.nc) SR_STAGE(launch_region(ch, ch.n_vs, ch.nc - ch.n_vs, false));
    if (last.timed) SR_HIP_CHECK(hipEventRecord(ctx->ev_c1[c], ch.cs));
    if (early) SR_HIP_CHECK(hipEventRecord(ctx->ev_red[c], ch.cs));
    if (early && c == n_chunks - 1) {  // every chunk's flags are final: to pinned memory, ahead of this chunk's chain
      for (int k = 0; k < c; ++k) SR_HIP_CHECK(hipStreamWaitEvent(ch.cs, ctx->ev_red[k], 0));
      SR_HIP_CHECK(hipMemcpyAsync(ctx->h_outs.as<char>() + ctx->outs_flag_off, ctx->outs.as<char>() + ctx->outs_flag_off,
                                  size_t(nt) * sizeof(uint32_t), hipMemcpyDeviceToHost, ch.cs));
      SR_HIP_CHECK(hipEventRecord(ctx->ev_flags, ch.cs));
    }
    if (fold.path && !want.shard && !fjob.regions.empty()) SR_STAGE(fold_chunk(ch));
    last.n_chunks = c + 1;
    code_base += uint32_t(ch.ncode);
    return SR_OK;
  }

  // The stages of a call, in order.
  int run() {
    SR_STAGE(validate_call());
    SR_STAGE(stage_param_table());
    choose_kernels();
    SR_STAGE(bind_buffers());
    in_flight = true;  // (plan_fold's memset is the call's first asynchronous operation)
    SR_STAGE(plan_fold());
    SR_STAGE(plan_chunks());
    SR_STAGE(bind_outputs());
    SR_STAGE(prepare_hints());
    SR_STAGE(begin_programs());
    SR_STAGE(launch_derived());
    SR_STAGE(begin_chunks());
    for (int c = 0; c < n_chunks && nt > 0; ++c) SR_STAGE(run_chunk(c));
    if (n_chunks > 1) {  // the caller continues on the first stream: join the second
      SR_HIP_CHECK(hipEventRecord(ctx->ev_join, ctx->stream2));
      SR_HIP_CHECK(hipStreamWaitEvent(s, ctx->ev_join, 0));
    }
    if (nt == 0) mark_phase(0);
    res->grid = glast;
    if (fold.path && want.shard) ctx->fold_job = std::make_shared<FoldJob<T>>(std::move(fjob));  // (eval_sharded_impl)
    mark_phase(1);
    return SR_OK;
  }
};

template <typename T>
int run_batch(sr_ctx* ctx, const EvalReq& req, const BatchWants& want, SrProgramBatch<T>* prog, BatchResult* res) {
  BatchCall<T> b(ctx, req, want, prog, res);
  const int rc = b.run();
  // error exits while work is in flight: no DMA may still read the staging buffers
  if (rc != SR_OK && b.in_flight) {
    (void)hipStreamSynchronize(ctx->stream);
    if (ctx->stream2) (void)hipStreamSynchronize(ctx->stream2);
  }
  return rc;
}
// run_batch for the dataset's element type, for the callers that need only ctx->d_out_sum / d_out_flag
inline int run_batch_any(sr_ctx* ctx, const EvalReq& req, const BatchWants& want, BatchResult* res) {
  if (req.ds->dtype == SR_DTYPE_F32) {
    SrProgramBatch<float> prog;
    return run_batch<float>(ctx, req, want, &prog, res);
  }
  SrProgramBatch<double> prog;
  return run_batch<double>(ctx, req, want, &prog, res);
}

// Interpreter time of the last call's own run_batch (sr_ctx::LastCall, ms): Σ of its launches' durations (as a
// kernel trace sums them; chunks on the two streams may overlap, so this can exceed the wall time they span).
inline double chunk_kernel_ms(sr_ctx* ctx) {
  double ms = 0.0;
  if (!ctx->last.timed) return 0.0;
  for (int c = 0; c < ctx->last.n_chunks; ++c) {
    float m = 0.f;
    if (hipEventElapsedTime(&m, ctx->ev_c0[c], ctx->ev_c1[c]) == hipSuccess) ms += double(m);
  }
  if (ctx->last.derived) {  // the derived columns are part of the call's interpreter work
    float m = 0.f;
    if (hipEventElapsedTime(&m, ctx->ev_d0, ctx->ev_d1) == hipSuccess) ms += double(m);
  }
  return ms;
}

// The same launches' device-busy time: the UNION of their [start, end] intervals (chunks on the two
// streams overlap, so the sum above can exceed the wall time they span; this cannot).
inline double chunk_busy_ms(sr_ctx* ctx) {
  std::vector<std::pair<double, double>> iv;
  if (!ctx->last.timed) return 0.0;
  auto add = [&](hipEvent_t a, hipEvent_t b) {
    float t0 = 0.f, t1 = 0.f;
    if (hipEventElapsedTime(&t0, ctx->ev_start, a) == hipSuccess && hipEventElapsedTime(&t1, ctx->ev_start, b) == hipSuccess)
      iv.push_back({double(t0), double(t1)});
  };
  for (int c = 0; c < ctx->last.n_chunks; ++c) add(ctx->ev_c0[c], ctx->ev_c1[c]);
  if (ctx->last.derived) add(ctx->ev_d0, ctx->ev_d1);
  if (ctx->last.fold_timed)  // (the in-order fold's launches: device work of the call too)
    for (int c = 0; c < ctx->last.n_chunks; ++c) add(ctx->ev_fc0[c], ctx->ev_fc1[c]);
  std::sort(iv.begin(), iv.end());
  double busy = 0.0, lo = 0.0, hi = -1.0;
  for (const auto& [a, b] : iv) {
    if (a > hi) {
      if (hi > lo) busy += hi - lo;
      lo = a;
      hi = b;
    } else {
      hi = std::max(hi, b);
    }
  }
  if (hi > lo) busy += hi - lo;
  return busy;
}

// ---------------------------------------------------------------- Julia's pairwise `sum`
// DynamicExpressions decides a checked array with isfinite(sum(x)); Base's `sum` over an Array runs
// Base.mapreduce_impl: [lo, hi] splits at lo + (hi - lo) >> 1 until hi - lo < 1024
// (pairwise_blocksize), each leaf block is folded sequentially (v = a[lo]; v = v + a[i]) in T, and
// the halves are added back in the same recursion (arrays of < 16 elements: one sequential fold,
// which is the same thing).  The kernel's EXACT mode computes the leaf folds over row ranges; the
// host adds them in recursion order.  Row sharding: the global leaves are intersected with each
// shard; a leaf that starts in an earlier shard is carried by its first shard's prefix fold and
// continued, row by row, with this shard's values ("head" ranges of one row each).
struct JlRange {
  int64_t lo, hi;  // local rows of this view / shard (inclusive)
  int64_t leaf;    // global leaf index
  bool head;       // a single row continuing a leaf that starts in an earlier shard
};

std::vector<std::pair<int64_t, int64_t>> jl_leaves(int64_t n) {
  std::vector<std::pair<int64_t, int64_t>> out, st;
  if (n <= 0) return out;
  st.push_back({0, n - 1});
  while (!st.empty()) {
    const auto [lo, hi] = st.back();
    st.pop_back();
    if (hi - lo < 1024) {
      out.push_back({lo, hi});
    } else {
      const int64_t mid = lo + ((hi - lo) >> 1);
      st.push_back({mid + 1, hi});
      st.push_back({lo, mid});
    }
  }
  return out;
}

// The ranges a shard holding global rows [off, off + n) of n_total sums (in this order).
std::vector<JlRange> jl_ranges(int64_t off, int64_t n, int64_t n_total) {
  std::vector<JlRange> out;
  const auto leaves = jl_leaves(n_total);
  const int64_t last = off + n - 1;
  for (size_t k = 0; k < leaves.size(); ++k) {
    const auto [L, H] = leaves[k];
    if (H < off || L > last) continue;
    const int64_t h = H < last ? H : last;
    if (L >= off) {
      out.push_back({L - off, h - off, int64_t(k), false});
    } else {
      for (int64_t r = off; r <= h; ++r) out.push_back({r - off, r - off, int64_t(k), true});
    }
  }
  return out;
}

template <typename T>
T jl_reduce(const std::vector<T>& leafval, int64_t lo, int64_t hi, size_t* idx) {
  if (hi - lo < 1024) return leafval[(*idx)++];
  const int64_t mid = lo + ((hi - lo) >> 1);
  const T a = jl_reduce<T>(leafval, lo, mid, idx);
  const T b = jl_reduce<T>(leafval, mid + 1, hi, idx);
  return a + b;
}

// isfinite(Julia sum) of n_arrays arrays of n_total rows from every shard's range folds:
// rank_vals[r] = [n_arrays][ranges of shard r] (T), shards r = [offs[r], offs[r + 1]).
template <typename T>
void jl_finite(int64_t n_total, int n_ranks, const int64_t* offs, const T* const* rank_vals, int64_t n_arrays,
               uint8_t* out_finite) {
  const size_t n_leaves = jl_leaves(n_total).size();
  std::vector<std::vector<JlRange>> ranges(static_cast<size_t>(n_ranks));
  for (int r = 0; r < n_ranks; ++r) ranges[size_t(r)] = jl_ranges(offs[r], offs[r + 1] - offs[r], n_total);
  std::vector<T> leafval(n_leaves);
  for (int64_t a = 0; a < n_arrays; ++a) {
    for (int r = 0; r < n_ranks; ++r) {
      const std::vector<JlRange>& rg = ranges[size_t(r)];
      const T* v = rank_vals[r] + size_t(a) * rg.size();
      for (size_t i = 0; i < rg.size(); ++i) {
        T& dst = leafval[size_t(rg[i].leaf)];
        dst = rg[i].head ? T(dst + v[i]) : v[i];
      }
    }
    size_t idx = 0;
    const T sum = n_total > 0 ? jl_reduce<T>(leafval, 0, n_total - 1, &idx) : T(0);
    out_finite[a] = std::isfinite(sum) ? 1 : 0;
  }
}

// Base.mapreduce_impl's combine of one view's leaf folds as a level-ordered node list: internal
// node m = (left, right) with c >= 0 = leaf c (leaves numbered in row order) and c < 0 = internal
// node -c-1; nodes are grouped by height (level_off), so every node's children lie in earlier levels.
struct JlLevels {
  std::vector<int32_t> nodes;      // 2 per internal node
  std::vector<int32_t> level_off;  // n_levels + 1
};
JlLevels jl_levels(int64_t n) {
  struct Tmp {
    int64_t l, r;  // >= 0 leaf, < 0 temporary internal id -x-1
    int h;
  };
  std::vector<Tmp> tmp;
  int64_t n_leaf = 0;
  // returns (code, height)
  std::function<std::pair<int64_t, int>(int64_t, int64_t)> rec = [&](int64_t lo, int64_t hi) -> std::pair<int64_t, int> {
    if (hi - lo < 1024) return {n_leaf++, 0};
    const int64_t mid = lo + ((hi - lo) >> 1);
    const auto L = rec(lo, mid);
    const auto R = rec(mid + 1, hi);
    const int h = 1 + std::max(L.second, R.second);
    tmp.push_back(Tmp{L.first, R.first, h});
    return {-int64_t(tmp.size()), h};
  };
  JlLevels out;
  if (n > 0) rec(0, n - 1);
  int max_h = 0;
  for (const Tmp& t : tmp) max_h = std::max(max_h, t.h);
  std::vector<int64_t> final_id(tmp.size());
  out.level_off.assign(size_t(max_h) + 1, 0);
  for (const Tmp& t : tmp) out.level_off[size_t(t.h)]++;  // counts at heights 1..max_h
  for (int h = 1; h <= max_h; ++h) out.level_off[size_t(h)] += out.level_off[size_t(h - 1)];
  std::vector<int64_t> fill(out.level_off.begin(), out.level_off.end() - 1);  // level h-1 starts at level_off[h-1]
  for (size_t i = 0; i < tmp.size(); ++i) final_id[i] = fill[size_t(tmp[i].h - 1)]++;
  out.nodes.resize(2 * tmp.size());
  auto code = [&](int64_t c) -> int32_t { return c >= 0 ? int32_t(c) : int32_t(-final_id[size_t(-c - 1)] - 1); };
  for (size_t i = 0; i < tmp.size(); ++i) {
    out.nodes[2 * size_t(final_id[i])] = code(tmp[i].l);
    out.nodes[2 * size_t(final_id[i]) + 1] = code(tmp[i].r);
  }
  return out;
}

// One view's leaves and combine program depend only on its row count: built once per thread and
// count (every call of a search or a step sees the same n; ~2k recursive calls for 1M rows).
const std::vector<JlRange>& jl_ranges_cached(int64_t n) {
  thread_local int64_t cn = -1;
  thread_local std::vector<JlRange> c;
  if (cn != n) {
    c = jl_ranges(0, n, n);
    cn = n;
  }
  return c;
}
const JlLevels& jl_levels_cached(int64_t n) {
  thread_local int64_t cn = -1;
  thread_local JlLevels c;
  if (cn != n) {
    c = jl_levels(n);
    cn = n;
  }
  return c;
}

// EXACT pass: the Julia-order fold of every checked array of the listed trees over `ranges` of this
// view -> host_vals[n_list][max_checks][ranges] (T; a tree's unused check slots hold 0).  With
// host_finite (single view: the ranges are the view's leaves in order) the leaves are combined on
// the device in recursion order and only isfinite(sum) per array comes back: host_finite[n_list][max_checks].
// Speculative use (stream `st`, sync = false; host_finite required, one batch): the launches are
// only enqueued — after a synchronisation of `st` the verdicts are at h_exact + *fin_off
// ([n_list][max_checks]) and ev_k0 / ev_k1 bracket the pass.
template <typename T>
int run_exact(sr_ctx* ctx, const EvalReq& req, const SrProgramBatch<T>& prog, const int64_t* list, int64_t n_list,
              int max_checks, const std::vector<JlRange>& ranges, T* host_vals, uint8_t* host_finite = nullptr,
              int64_t dev_row_off = 0, hipStream_t st = nullptr, bool sync = true, size_t* fin_off = nullptr) {
  if (n_list == 0 || max_checks == 0 || ranges.empty()) return SR_OK;
  if (!sync && (!host_finite || !fin_off)) return set_error(SR_ERR_INVALID_ARG, "speculative exact pass: no verdict buffer");
  const sr_dataset* const ds = req.ds;
  const bool gather = req.gather();
  const int64_t n_eval = req.n_eval();
  hipStream_t s = st ? st : ctx->stream;
  const int depth = prog.max_depth > 0 ? prog.max_depth : 1;
  const int R = sr_rows_per_lane<T>(SR_MODE_EXACT, SR_TIER_FULL, 0);
  const int64_t rows = 64 * int64_t(R);
  // (BASIC operator sets: the BASIC-tier build of the pass, same rows and LDS plan, a smaller
  //  dispatch; SR_AMD_EXACT_TIER=full keeps the FULL-tier build for A/B runs)
  static const bool exact_full = [] {
    const char* v = std::getenv("SR_AMD_EXACT_TIER");
    return v && std::strcmp(v, "full") == 0;
  }();
  // a parametric call (EvalReq::params, the table of its run_batch still on the device): the PARAM builds
  // of the pass — the FULL-tier build, 4 waves — over the staged rows with the hidden class row
  const sr_param_batch* const pb = req.params;
  const int nfk = int(ds->nf) + (pb ? 1 : 0);
  const int etier = (prog.tier == SR_TIER_BASIC && !exact_full && !pb) ? SR_TIER_BASIC : SR_TIER_FULL;
  const int64_t n_ranges = int64_t(ranges.size());
  int64_t max_len = 1;
  std::vector<int64_t> lo(static_cast<size_t>(n_ranges)), hi(static_cast<size_t>(n_ranges));
  for (int64_t i = 0; i < n_ranges; ++i) {
    lo[size_t(i)] = ranges[size_t(i)].lo;
    hi[size_t(i)] = ranges[size_t(i)].hi;
    if (hi[size_t(i)] < lo[size_t(i)] || hi[size_t(i)] >= n_eval) return set_error(SR_ERR_INVALID_ARG, "bad row range");
    max_len = std::max(max_len, hi[size_t(i)] - lo[size_t(i)] + 1);
  }
  // listed trees in batches whose range folds fit a bounded scratch buffer
  const size_t per_tree = size_t(max_checks) * size_t(n_ranges) * sizeof(T);
  const int64_t batch = std::max<int64_t>(1, int64_t((size_t(256) << 20) / per_tree));
  // pinned staging: [leaf ranges lo | hi | Julia-sum level program | tree list | verdicts]
  static const JlLevels kNoLevels{};
  const JlLevels& lv = host_finite ? jl_levels_cached(n_eval) : kNoLevels;
  const size_t n_lvp = lv.nodes.size() + lv.level_off.size();
  const size_t o_hi = size_t(n_ranges) * sizeof(int64_t), o_lvp = 2 * o_hi;
  const size_t o_list = (o_lvp + n_lvp * sizeof(int32_t) + 15) & ~size_t(15);
  const size_t o_fin = (o_list + size_t(std::min(batch, n_list)) * sizeof(uint32_t) + 15) & ~size_t(15);
  const size_t n_fin = host_finite ? size_t(std::min(batch, n_list)) * size_t(max_checks) : 0;
  SR_HIP_CHECK(ctx->h_exact.ensure(o_fin + n_fin + 16, s, ctx->stream2));
  char* const hx = ctx->h_exact.as<char>();
  {
    const size_t cap_lo = ctx->range_lo.cap, cap_hi = ctx->range_hi.cap;
    SR_HIP_CHECK(ctx->range_lo.ensure(size_t(n_ranges) * sizeof(int64_t)));
    SR_HIP_CHECK(ctx->range_hi.ensure(size_t(n_ranges) * sizeof(int64_t)));
    if (ctx->range_lo.cap != cap_lo || ctx->range_hi.cap != cap_hi || ctx->exact_lo_dev != lo || ctx->exact_hi_dev != hi) {
      ctx->exact_lo_dev.clear();  // (re-set only once the copies are queued)
      std::memcpy(hx, lo.data(), o_hi);
      std::memcpy(hx + o_hi, hi.data(), o_hi);
      SR_HIP_CHECK(hipMemcpyAsync(ctx->range_lo.p, hx, o_hi, hipMemcpyHostToDevice, s));
      SR_HIP_CHECK(hipMemcpyAsync(ctx->range_hi.p, hx + o_hi, o_hi, hipMemcpyHostToDevice, s));
      ctx->exact_lo_dev = lo;
      ctx->exact_hi_dev = hi;
    }
  }
  int n_internal = 0, n_levels = 0;
  if (host_finite) {
    n_internal = int(lv.nodes.size() / 2);
    n_levels = int(lv.level_off.size()) - 1;
    if (n_internal != n_ranges - 1 && !(n_ranges == 1 && n_internal == 0))
      return set_error(SR_ERR_INVALID_ARG, "bad leaf structure");
    // nodes then level offsets, one upload (kept for the next call over as many rows)
    const size_t cap = ctx->jsum_prog.cap;
    SR_HIP_CHECK(ctx->jsum_prog.ensure(n_lvp * sizeof(int32_t)));
    if (ctx->jsum_prog.cap != cap || ctx->jsum_n_dev != n_eval) {
      ctx->jsum_n_dev = -1;
      int32_t* b = reinterpret_cast<int32_t*>(hx + o_lvp);
      std::copy(lv.nodes.begin(), lv.nodes.end(), b);
      std::copy(lv.level_off.begin(), lv.level_off.end(), b + lv.nodes.size());
      SR_HIP_CHECK(hipMemcpyAsync(ctx->jsum_prog.p, b, n_lvp * sizeof(int32_t), hipMemcpyHostToDevice, s));
      ctx->jsum_n_dev = n_eval;
    }
  }
  if (!sync && batch < n_list) return set_error(SR_ERR_INVALID_ARG, "speculative exact pass: list too long");
  for (int64_t b0 = 0; b0 < n_list; b0 += batch) {
    const int64_t nb = std::min(batch, n_list - b0);
    // one wave per workgroup, G listed trees per workgroup (LDS: X tile + one wave's checked
    // values [max_checks][rows] + running sums [G][max_checks]): G amortises the tile staging over
    // trees, small G spreads few trees over more waves; aim at >= 1024 waves (one per SIMD), G <= 16
    // (C2's 8 listed trees x 1024 leaf ranges: G 1 -> 8, exact pass 0.28 -> 0.21 ms;
    // profiles/r02_ab_exact_g.txt)
    const int64_t g_fill = (nb * n_ranges + 1023) / 1024;
    int G = int(std::min<int64_t>(nb, ctx->exact_g > 0 ? ctx->exact_g : std::max<int64_t>(1, std::min<int64_t>(16, g_fill))));
    // four waves per workgroup share the staged rows, each folding its own trees: one wave per
    // workgroup left ~1 wave per SIMD for C2's 8 listed trees x 1024 leaves (latency-bound)
    int W = ((ctx->exact_w == 4 && G >= 4) || pb) ? 4 : 1;
    size_t lds = 0;
    for (;;) {
      lds = sr_tile_lds_bytes(int(sizeof(T)), nfk, R, depth, G, max_checks, W, false);
      if (lds <= kLdsMax || G == 1) break;
      G /= 2;
      if (G < W && !pb) W = 1;
    }
    if (lds > kLdsMax) return set_error(SR_ERR_TOO_DEEP, "exact-sum pass needs more LDS than 160 KiB");
    uint32_t* list32 = reinterpret_cast<uint32_t*>(hx + o_list);  // (the previous batch's pass has completed)
    for (int64_t i = 0; i < nb; ++i) list32[i] = uint32_t(list[b0 + i]);
    SR_HIP_CHECK(ctx->range_sums.ensure(size_t(nb) * per_tree));
    SrEvalArgs<T> a{};
    a.code = static_cast<const SrIns<T>*>(ctx->d_code);
    a.offsets = ctx->d_off;
    a.ends = ctx->d_end;
    a.perm = list32;  // (read from the pinned staging buffer: no upload ahead of the kernel)
    a.n_trees = int(nb);
    a.trees_per_block = G;
    a.X = static_cast<const T*>(ds->X);
    a.row_idx = gather ? ctx->row_idx.as<int64_t>() + dev_row_off : nullptr;  // (this view's rows on the device)
    a.ld = ds->ld;
    a.n_rows = n_eval;
    a.nf = nfk;
    if (pb) {
      a.ptab = ctx->ptab.as<T>();
      a.p_stride = int(pb->max_parameters) * int(pb->n_classes);
      a.n_classes = int(pb->n_classes);
    }
    a.tiles_per_block = int((max_len + rows - 1) / rows);
    a.n_row_blocks = int(n_ranges);
    a.n_groups = int((nb + G - 1) / G);
    a.stack_depth = depth;
    a.tbig = T(0);
    a.max_checks = max_checks;
    a.range_lo = ctx->range_lo.as<int64_t>();
    a.range_hi = ctx->range_hi.as<int64_t>();
    a.range_sums = ctx->range_sums.p;
    const int64_t blocks = int64_t(a.n_groups) * n_ranges;
    if (blocks > 0x7fffffff) return set_error(SR_ERR_INVALID_ARG, "grid too large");
    SR_HIP_CHECK(hipEventRecord(ctx->ev_k0, s));
    const SrBuildRequest q{int(sizeof(T)), SR_MODE_EXACT, gather, etier, R, W, false, a.loss_kind,
                           pb ? SR_FAMILY_PARAM : SR_FAMILY_PLAIN};
    SR_HIP_CHECK(sr_launch_eval<T>(a, q, int(blocks), s));
    if (host_finite) {
      const int64_t n_arrays = nb * max_checks;
      SR_HIP_CHECK(ctx->jsum_scratch.ensure(size_t(std::max<int64_t>(1, n_arrays * n_internal)) * sizeof(T)));
      const int32_t* lvp = ctx->jsum_prog.as<int32_t>();
      // (the verdicts go straight into the pinned staging buffer: no copy back)
      uint8_t* fin = reinterpret_cast<uint8_t*>(hx + o_fin);
      SR_HIP_CHECK(sr_launch_jsum_levels<T>(static_cast<const T*>(ctx->range_sums.p), n_arrays, int(n_ranges),
                                            reinterpret_cast<const int2*>(lvp), n_internal, lvp + 2 * n_internal,
                                            n_levels, ctx->jsum_scratch.as<T>(), fin, s));
    } else {
      SR_HIP_CHECK(hipMemcpyAsync(host_vals + size_t(b0) * max_checks * size_t(n_ranges), ctx->range_sums.p,
                                  size_t(nb) * per_tree, hipMemcpyDeviceToHost, s));
    }
    SR_HIP_CHECK(hipEventRecord(ctx->ev_k1, s));
    if (!sync) {
      *fin_off = o_fin;
      return SR_OK;
    }
    SR_HIP_CHECK(hipStreamSynchronize(s));
    if (host_finite)
      std::memcpy(host_finite + size_t(b0) * max_checks, hx + o_fin, size_t(nb) * size_t(max_checks));
    float km = 0.f;
    if (hipEventElapsedTime(&km, ctx->ev_k0, ctx->ev_k1) == hipSuccess) ctx->exact_kernel_ms += double(km);
  }
  return SR_OK;
}

// EXACT pass over the whole view on this GPU -> list_ok[i] = every checked array of tree list[i]
// passes isfinite(Julia sum).
template <typename T>
int exact_list_ok(sr_ctx* ctx, const EvalReq& req, const SrProgramBatch<T>& prog, const std::vector<int64_t>& list,
                  std::vector<uint8_t>* list_ok, int64_t dev_row_off = 0) {
  list_ok->assign(list.size(), 1);
  if (list.empty() || prog.max_checks == 0) return SR_OK;
  const std::vector<JlRange>& ranges = jl_ranges_cached(req.n_eval());
  // check slots: the most any LISTED tree has (the LDS image and the fold buffers scale with it)
  int mc = 0;
  for (int64_t t : list) mc = std::max(mc, int(prog.n_checks[size_t(t)]));
  if (mc == 0) return SR_OK;
  // leaf folds combined in recursion order on the device: only the verdicts come back
  std::vector<uint8_t> fin(list.size() * size_t(mc));
  int rc = run_exact<T>(ctx, req, prog, list.data(), int64_t(list.size()), mc, ranges, nullptr, fin.data(), dev_row_off);
  if (rc != SR_OK) return rc;
  for (size_t i = 0; i < list.size(); ++i)
    for (int k = 0; k < mc; ++k) (*list_ok)[i] &= fin[i * size_t(mc) + size_t(k)];
  return SR_OK;
}

// Finalize one tree: complete unless flagged; BIG-only trees take their exact verdict (list_ok).  A
// complete tree's loss is Σ / denom, or +Inf where the reference's T-precision fold of the losses
// overflows (sr_fold.h; n_terms = rows of the fold, 0: only SR_FLAG_ELEMINF is applied).  Trees the
// bounds cannot decide are appended to *fold_list (when given) for the exact in-order fold.
// fold (may be NULL): every complete tree's in-order fold from the call's walk (values, SR_FST_* status,
// and the T denominators: T(count), or Base.sum(w) in T, per tree); a tree the walk folded takes
// fold / denominator in T (the reference's own arithmetic), one whose walk failed joins *fold_list.
template <typename T>
struct FoldResults {
  const T* val;
  const int32_t* st;
  std::function<T(int64_t)> den;
  int64_t n_ok = 0, n_fail = 0;
  int debug_fail = 0;  // (tests, "fold_debug_fail" k: trees t % k == 0 take the fallback as if their walk failed)
};
template <typename T>
void finalize(int64_t nt, const double* sums, const uint32_t* flags, double denom, const int64_t* list,
              int64_t n_list, const uint8_t* list_ok, T* out_loss, uint8_t* out_complete, int64_t n_terms = 0,
              std::vector<int64_t>* fold_list = nullptr, const double* denoms = nullptr, FoldResults<T>* fold = nullptr) {
  std::vector<int64_t> pos;
  if (n_list > 0) {
    pos.assign(size_t(nt), -1);
    for (int64_t i = 0; i < n_list; ++i) pos[size_t(list[i])] = i;
  }
  for (int64_t t = 0; t < nt; ++t) {
    bool ok = (flags[t] & (SR_FLAG_NONFINITE | SR_FLAG_STATIC)) == 0;
    if (ok && (flags[t] & SR_FLAG_BIG)) {
      const int64_t p = pos.empty() ? -1 : pos[size_t(t)];
      if (p >= 0 && list_ok && !list_ok[p]) ok = false;
    }
    out_complete[t] = ok ? 1 : 0;
    out_loss[t] = ok ? T(sums[t] / (denoms ? denoms[t] : denom)) : T(INFINITY);
    if (!ok) continue;
    const bool elem_inf = (flags[t] & SR_FLAG_ELEMINF) != 0;
    const int cls = n_terms > 0 ? sr_fold_class<T>(sums[t], elem_inf, n_terms) : (elem_inf ? SR_FOLD_INF : SR_FOLD_FINITE);
    if (cls == SR_FOLD_INF) {
      out_loss[t] = T(INFINITY);
    } else if (cls == SR_FOLD_EXACT && fold_list) {
      fold_list->push_back(t);
    } else if (cls == SR_FOLD_FINITE && fold) {
      if (fold->st[t] == SR_FST_OK && !(fold->debug_fail > 0 && t % fold->debug_fail == 0)) {
        out_loss[t] = T(fold->val[t] / fold->den(t));
        ++fold->n_ok;
      } else if (fold->st[t] != SR_FST_NONE && fold_list) {
        fold_list->push_back(t);
        ++fold->n_fail;
      }
    }
  }
}

// The trees `idx` of a batch as a batch of their own (node arrays copied: a tree is a contiguous range).
template <typename T>
struct SubBatch {
  std::vector<int64_t> offs;
  std::vector<uint8_t> deg, op, con;
  std::vector<uint16_t> feat;
  std::vector<T> val;
  sr_tree_batch b{};
  SubBatch(const sr_tree_batch& trees, const int64_t* idx, size_t n) {
    offs.assign(n + 1, 0);
    for (size_t i = 0; i < n; ++i) offs[i + 1] = offs[i] + (trees.offsets[idx[i] + 1] - trees.offsets[idx[i]]);
    const size_t nn = size_t(offs.back());
    deg.resize(nn);
    op.resize(nn);
    con.resize(nn);
    feat.resize(nn);
    val.resize(nn);
    const T* vals = static_cast<const T*>(trees.val);
    for (size_t i = 0; i < n; ++i) {
      const int64_t b0 = trees.offsets[idx[i]], len = offs[i + 1] - offs[i], o = offs[i];
      std::memcpy(deg.data() + o, trees.degree + b0, size_t(len));
      std::memcpy(op.data() + o, trees.op + b0, size_t(len));
      std::memcpy(con.data() + o, trees.constant + b0, size_t(len));
      std::memcpy(feat.data() + o, trees.feature + b0, size_t(len) * sizeof(uint16_t));
      std::memcpy(val.data() + o, vals + b0, size_t(len) * sizeof(T));
    }
    b = sr_tree_batch{int64_t(n), offs.data(), deg.data(), op.data(), feat.data(), con.data(), val.data()};
  }
};

// The parameter side of the same trees (a parametric call's fold passes): node arrays and matrices copied
// alike (src NULL, a plain call: empty); the sub-request's `params` points at `b` (fold_prepare).
template <typename T>
struct SubParam {
  std::vector<uint8_t> isp;
  std::vector<uint16_t> par;
  std::vector<T> mats;
  sr_param_batch b{};
  SubParam(const sr_param_batch* saved, const sr_tree_batch& trees, const int64_t* idx, size_t n) {
    if (!saved) return;
    const size_t stride = size_t(saved->max_parameters) * size_t(saved->n_classes);
    const T* src = static_cast<const T*>(saved->parameters);
    mats.resize(n * stride + 1);
    for (size_t i = 0; i < n; ++i) {
      const int64_t b0 = trees.offsets[idx[i]], len = trees.offsets[idx[i] + 1] - b0;
      isp.insert(isp.end(), saved->is_parameter + b0, saved->is_parameter + b0 + len);
      par.insert(par.end(), saved->parameter + b0, saved->parameter + b0 + len);
      if (stride) std::memcpy(mats.data() + i * stride, src + size_t(idx[i]) * stride, stride * sizeof(T));
    }
    if (isp.empty()) {  // (non-NULL arrays for an empty list)
      isp.push_back(0);
      par.push_back(0);
    }
    b = sr_param_batch{isp.data(), par.data(), saved->max_parameters, saved->n_classes, mats.data()};
  }
  SubParam(const SubParam&) = delete;
  SubParam& operator=(const SubParam&) = delete;
};

// Rows per segment of the fold's segmented chain (sr_aux.hip): ctx->fold_seg < 0 chooses (<= 1024
// segments of 8k-64k rows), 0 folds the whole view with one workgroup scan per tree (rounds 3-4).
inline int64_t fold_seg_len(const sr_ctx* ctx, int64_t n) {
  if (ctx->fold_seg >= 0) return ctx->fold_seg;
  const int64_t L = ((n / 512 + 8191) / 8192) * 8192;
  return std::min<int64_t>(std::max<int64_t>(L, 8192), 65536);
}

// The prediction buffer of the fold's PRED passes is kept up to 1/32 of the device memory (9 GB on a
// 288 GB MI355X: C4's 14 band trees x 2^26 rows are 3.6 GB, and a re-allocation cost the step ~35 ms);
// anything larger is released after the call.
inline void release_large_pred(sr_ctx* ctx) {
  size_t free_b = 0, total_b = 0;
  const size_t keep = hipMemGetInfo(&free_b, &total_b) == hipSuccess ? std::max(total_b / 32, size_t(2) << 30)
                                                                       : (size_t(2) << 30);
  if (ctx->pred.cap > keep) ctx->pred.release();
}

// Device scratch of one fold batch of nb trees and n_seg segments (ctx->fold_io): segment sums,
// binades and composed steps, carries, estimates, results and slow-segment counts.
template <typename T>
struct FoldDev {
  double* segsum = nullptr;
  int2* tq = nullptr;
  int64_t* tab = nullptr;
  double* carry_est = nullptr;
  T* carry = nullptr;
  T* out = nullptr;
  int* slow = nullptr;
  static size_t al(size_t b) { return (b + 255) & ~size_t(255); }
  static size_t bytes(size_t nb, int64_t n_seg) {
    const size_t ns = nb * size_t(n_seg > 0 ? n_seg : 1);
    return al(ns * 8) + al(ns * 8) + al(ns * 32) + al(nb * 8) + 2 * al(nb * sizeof(T)) + al(nb * 4);
  }
  void bind(void* base, size_t nb, int64_t n_seg) {
    const size_t ns = nb * size_t(n_seg > 0 ? n_seg : 1);
    char* c = static_cast<char*>(base);
    segsum = reinterpret_cast<double*>(c);
    c += al(ns * 8);
    tq = reinterpret_cast<int2*>(c);
    c += al(ns * 8);
    tab = reinterpret_cast<int64_t*>(c);
    c += al(ns * 32);
    carry_est = reinterpret_cast<double*>(c);
    c += al(nb * 8);
    carry = reinterpret_cast<T*>(c);
    c += al(nb * sizeof(T));
    out = reinterpret_cast<T*>(c);
    c += al(nb * sizeof(T));
    slow = reinterpret_cast<int*>(c);
  }
};

// Trees per PRED pass of the fold: predictions of at most `budget` bytes (and half the free device
// memory when `use_free`; the row-sharded call uses a fixed budget so that every rank cuts the list
// alike).
inline int64_t fold_batch_trees(int64_t n_eval, size_t elem, bool use_free) {
  size_t budget = size_t(8) << 30, free_b = 0, total_b = 0;
  if (use_free && hipMemGetInfo(&free_b, &total_b) == hipSuccess) budget = std::min(budget, free_b / 2);
  return std::max<int64_t>(1, int64_t(budget / (size_t(std::max<int64_t>(n_eval, 1)) * elem)));
}

// One batch of listed trees, first half: the PRED interpreter over this view (or shard) into ctx->pred —
// an internal pass (BatchWants::internal) over a sub-request: these trees, and in a parametric call their
// own parameter side — the device scratch bound, and (segmented) the segment sums.
template <typename T>
int fold_prepare(sr_ctx* ctx, const EvalReq& req, int64_t n_total, const int64_t* list, size_t nb, int64_t seg_len,
                 FoldDev<T>* fd) {
  int lkind = 0;
  double lparam = 0.0;
  if (decode_loss(ctx, req.loss_kind, &lkind, &lparam) != SR_OK) return SR_ERR_INVALID_ARG;
  const sr_dataset* const ds = req.ds;
  const int64_t n_eval = req.n_eval();
  SubBatch<T> sub(*req.trees, list, nb);
  SubParam<T> subp(req.params, *req.trees, list, nb);
  EvalReq sreq = req;
  sreq.trees = &sub.b;
  sreq.params = req.params ? &subp.b : nullptr;
  sreq.views = nullptr;
  BatchWants want;
  want.mode = SR_MODE_PRED;
  want.n_total = n_total;
  want.internal = true;
  SrProgramBatch<T> prog;
  BatchResult res;
  SR_HIP_CHECK(hipEventRecord(ctx->ev_f[0], ctx->stream));
  int rc = run_batch<T>(ctx, sreq, want, &prog, &res);
  if (rc != SR_OK) return rc;
  SR_HIP_CHECK(hipEventRecord(ctx->ev_f[1], ctx->stream));
  const int64_t n_seg = seg_len > 0 ? (n_eval + seg_len - 1) / seg_len : 0;
  SR_HIP_CHECK(ctx->fold_io.ensure(FoldDev<T>::bytes(nb, n_seg)));
  fd->bind(ctx->fold_io.p, nb, n_seg);
  if (seg_len > 0)
    SR_HIP_CHECK(sr_launch_fold_segsum<T>(ctx->pred.as<T>(), n_eval, int(nb), static_cast<const T*>(ds->y),
                                          static_cast<const T*>(ds->w), req.gather() ? ctx->row_idx.as<int64_t>() : nullptr,
                                          n_eval, lkind, T(lparam), seg_len, fd->segsum, ctx->stream));
  SR_HIP_CHECK(hipEventRecord(ctx->ev_f[2], ctx->stream));
  return SR_OK;
}

// Second half: the segments' composed steps (carry_est: device, per tree, or NULL) and the chain
// (carry: device, per tree, or NULL); the folds into out (host) after one synchronisation.
template <typename T>
int fold_finish(sr_ctx* ctx, const EvalReq& req, size_t nb, int64_t seg_len, const FoldDev<T>& fd, bool with_carry_est,
                bool with_carry, T* out) {
  int lkind = 0;
  double lparam = 0.0;
  if (decode_loss(ctx, req.loss_kind, &lkind, &lparam) != SR_OK) return SR_ERR_INVALID_ARG;
  const int64_t n_eval = req.n_eval();
  hipStream_t s = ctx->stream;
  const T* y = static_cast<const T*>(req.ds->y);
  const T* w = static_cast<const T*>(req.ds->w);
  const int64_t* ri = req.gather() ? ctx->row_idx.as<int64_t>() : nullptr;
  if (seg_len > 0)
    SR_HIP_CHECK(sr_launch_fold_segtab<T>(ctx->pred.as<T>(), n_eval, int(nb), y, w, ri, n_eval, lkind, T(lparam),
                                          seg_len, fd.segsum, with_carry_est ? fd.carry_est : nullptr, fd.tq, fd.tab, s));
  SR_HIP_CHECK(hipEventRecord(ctx->ev_f[3], s));
  SR_HIP_CHECK(sr_launch_fold<T>(ctx->pred.as<T>(), n_eval, int(nb), y, w, ri, n_eval, lkind, T(lparam), seg_len, fd.tq,
                                 fd.tab, with_carry ? fd.carry : nullptr, fd.out, fd.slow, s));
  SR_HIP_CHECK(hipEventRecord(ctx->ev_f[4], s));
  std::vector<int> slow(nb, 0);
  SR_HIP_CHECK(hipMemcpyAsync(out, fd.out, nb * sizeof(T), hipMemcpyDeviceToHost, s));
  SR_HIP_CHECK(hipMemcpyAsync(slow.data(), fd.slow, nb * sizeof(int), hipMemcpyDeviceToHost, s));
  SR_HIP_CHECK(hipStreamSynchronize(s));
  for (int v : slow) ctx->fold_slow_last += v;
  for (int i = 0; i < 4; ++i) {  // (events 0-2 were recorded by fold_prepare on the same stream)
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, ctx->ev_f[i], ctx->ev_f[i + 1]) == hipSuccess) ctx->fold_ms[i] += double(ms);
  }
  ctx->fold_seg_last = seg_len;
  return SR_OK;
}

// The reference's fold of the listed trees' losses over this view, exactly and in row order
// (sr_fold.h; sr_aux.hip): their predictions from the PRED interpreter (the values the LOSS kernels
// saw), then the segmented fold.  out: the folds (T; +Inf where the fold overflows).  Runs after the
// call's other passes (it reuses the context's program buffers).
template <typename T>
int fold_exact(sr_ctx* ctx, const EvalReq& req, int64_t n_total, const std::vector<int64_t>& list, std::vector<T>* out) {
  out->assign(list.size(), T(0));
  if (list.empty()) return SR_OK;
  const int64_t n_eval = req.n_eval();
  const int64_t seg_len = fold_seg_len(ctx, n_eval);
  const int64_t per = fold_batch_trees(n_eval, sizeof(T), true);
  for (size_t b0 = 0; b0 < list.size(); b0 += size_t(per)) {
    const size_t nb = std::min(list.size() - b0, size_t(per));
    FoldDev<T> fd;
    int rc = fold_prepare<T>(ctx, req, n_total, list.data() + b0, nb, seg_len, &fd);
    if (rc != SR_OK) return rc;
    rc = fold_finish<T>(ctx, req, nb, seg_len, fd, false, false, out->data() + b0);
    if (rc != SR_OK) return rc;
  }
  release_large_pred(ctx);
  return SR_OK;
}

// Base.sum in T of v[idx[i]] (or v[i]), i < n: Base.mapreduce_impl's pairwise recursion (blocks of
// < 1024 folded sequentially) — the reference's sum(w) (LossFunctions' normalize = true).
template <typename T>
T jl_sum_T(const double* v, const int64_t* idx, int64_t lo, int64_t hi) {  // inclusive [lo, hi]
  auto at = [&](int64_t i) { return T(v[idx ? idx[i] : i]); };
  if (lo == hi) return at(lo);
  if (hi - lo < 1024) {
    T a = at(lo) + at(lo + 1);
    for (int64_t i = lo + 2; i <= hi; ++i) a = a + at(i);
    return a;
  }
  const int64_t mid = lo + ((hi - lo) >> 1);
  const T x = jl_sum_T<T>(v, idx, lo, mid);
  const T y = jl_sum_T<T>(v, idx, mid + 1, hi);
  return x + y;
}

// The partials of the call's launches (ctx->host_reductions) reduced on the host into {Σ, flags}, in
// sr_reduce_positions' order: lane l sums row blocks l, l + 64, ... from 0.0, then for off = 32 .. 1 every
// lane adds its partner l ^ off (IEEE addition commutes, so both partners hold the same bits), lane 0's
// value is the result; flags ORed; the static flags from the staging image.
void host_reduce_partials(sr_ctx* ctx, int64_t nt) {
  const size_t n_part = size_t(nt) * size_t(ctx->host_red_rb);
  const double* ps = ctx->h_part.as<double>();
  const uint32_t* pf = reinterpret_cast<const uint32_t*>(ps + n_part);
  double* out_sum = ctx->h_outs.as<double>();
  uint32_t* out_flag = reinterpret_cast<uint32_t*>(ctx->h_outs.as<char>() + ctx->outs_flag_off);
  const uint32_t* perm = ctx->h_perm_last;
  const uint8_t* bad = ctx->h_bad_last;
  // (the partials are read once, in memory order — row block by row block, each a contiguous run of
  //  positions — into per-(position, lane) accumulators; lane l still adds its row blocks l, l + 64,
  //  ... in increasing order, so the sums are the reduce kernel's bit for bit.  Round 5: the column
  //  walk it replaces touched a new cache line per partial, ~6k device-written lines per C3 call)
  std::vector<double>& acc = ctx->host_acc;
  std::vector<uint32_t>& fls = ctx->host_fl;
  for (const sr_ctx::HostReduction& hr : ctx->host_reductions) {
    const double* s0 = ps + size_t(ctx->host_red_rb) * size_t(hr.p0);
    const uint32_t* f0 = pf + size_t(ctx->host_red_rb) * size_t(hr.p0);
    const size_t np = size_t(hr.np);
    acc.assign(np * 64, 0.0);
    fls.assign(np, 0u);
    for (int i = 0; i < hr.n_rb; ++i) {
      double* a = acc.data() + size_t(i & 63);
      const double* srow = s0 + size_t(i) * np;
      const uint32_t* frow = f0 + size_t(i) * np;
      for (size_t pos = 0; pos < np; ++pos) {
        a[pos * 64] += srow[pos];
        fls[pos] |= frow[pos];
      }
    }
    for (size_t pos = 0; pos < np; ++pos) {
      double v[64];
      std::memcpy(v, acc.data() + pos * 64, sizeof(v));
      for (int off = 32; off >= 1; off >>= 1) {
        double nv[64];
        for (int l = 0; l < 64; ++l) nv[l] = v[l] + v[l ^ off];
        std::memcpy(v, nv, sizeof(v));
      }
      uint32_t fl = fls[pos];
      const uint32_t tree = perm[hr.p0 + pos];
      if (bad[tree]) fl |= SR_FLAG_STATIC | SR_FLAG_NONFINITE;
      out_sum[tree] = v[0];
      out_flag[tree] = fl;
    }
  }
  ctx->host_reductions.clear();
}

// Base.sum(w) in T over a view (the reference's normalize = true denominator); the full view's is cached
// per dataset and type.
template <typename T>
T jl_wsum_view(const sr_dataset* ds, const int64_t* row_idx, int64_t n) {
  if (n <= 0) return T(0);
  if (row_idx) return jl_sum_T<T>(ds->w_host.data(), row_idx, 0, n - 1);
  double& c = sizeof(T) == 4 ? ds->wsum_jl_f32 : ds->wsum_jl_f64;
  if (!(c == c)) c = double(jl_sum_T<T>(ds->w_host.data(), nullptr, 0, n - 1));
  return T(c);
}

template <typename T>
double view_denominator(const sr_dataset* ds, const int64_t* row_idx, int64_t n_idx) {
  const bool gather = row_idx != nullptr && n_idx > 0;
  if (!ds->w) return double(gather ? n_idx : ds->n);
  if (!gather) return ds->wsum;
  double s = 0.0;
  for (int64_t i = 0; i < n_idx; ++i) s += ds->w_host[size_t(row_idx[i])];
  return s;
}

// The second half of an eval_loss call: what finishing it needs once its device work is enqueued — the
// request (with copies of the tree batch's and the views' structs, which it then points at) and what
// run_batch handed back.
template <typename T>
struct LossCall {
  EvalReq req;
  sr_tree_batch trees{};
  ViewSpec views{};
  void* out_loss = nullptr;
  uint8_t* out_complete = nullptr;
  SrProgramBatch<T> prog;
  std::chrono::steady_clock::time_point t0;
  BatchResult res;  // (early: finish copies the results back; fold_path: the walk's folds are among them)
};
template <typename T>
int eval_loss_finish(sr_ctx* ctx, LossCall<T>& c);

// First half: compile, stage, launch, and the copy of {Σ, flags} (or the kernel's own writes into
// pinned memory); *c holds what eval_loss_finish needs.
template <typename T>
int eval_loss_submit(sr_ctx* ctx, const EvalReq& req, void* out_loss, uint8_t* out_complete, LossCall<T>* c) {
  const int64_t nt = req.trees->n_trees;
  if (nt > 0 && (!out_loss || !out_complete)) return set_error(SR_ERR_INVALID_ARG, "NULL output buffers");
  c->t0 = std::chrono::steady_clock::now();
  ctx->start_phases(c->t0);
  c->req = req;
  c->trees = *req.trees;
  c->req.trees = &c->trees;
  if (req.views) {
    c->views = *req.views;
    c->req.views = &c->views;
  }
  c->out_loss = out_loss;
  c->out_complete = out_complete;
  BatchWants want;
  want.n_total = req.n_eval();
  want.allow_derived = true;
  want.host_out = want.fold = want.early = true;
  want.takes_expr = req.params == nullptr;  // (plain trees only: kLossExprOnly)
  const int rc = run_batch<T>(ctx, req, want, &c->prog, &c->res);
  if (rc != SR_OK) return rc;
  if (nt == 0) return SR_OK;
  hipStream_t s = ctx->stream;
  if (c->res.early) return SR_OK;  // (eval_loss_finish: the exact-sum pass first, then the one copy back)
  // {Σ loss, flags} of every tree: already in pinned memory (host_io), or one DMA there
  if (!c->res.outs_on_host) {
    const size_t out_bytes = c->res.fold_path ? ctx->outs_bytes_all : ctx->outs_flag_off + size_t(nt) * sizeof(uint32_t);
    SR_HIP_CHECK(ctx->h_outs.ensure(out_bytes, s, ctx->stream2));
    SR_HIP_CHECK(hipMemcpyAsync(ctx->h_outs.p, ctx->outs.p, out_bytes, hipMemcpyDeviceToHost, s));
  }
  return SR_OK;
}

template <typename T>
int eval_loss_finish(sr_ctx* ctx, LossCall<T>& c) {
  const EvalReq& q = c.req;
  const sr_dataset* const ds = q.ds;
  const ViewSpec* const views = q.views;
  SrProgramBatch<T>& prog = c.prog;
  const int64_t nt = q.trees->n_trees;
  if (nt == 0) return SR_OK;
  const int64_t n_eval = q.n_eval();
  const int n_views = views ? views->n_views : 1;
  auto view_of = [&](int64_t t) -> int { return views ? int(views->tree_view[t]) : 0; };
  auto rows_of = [&](int v) -> const int64_t* { return q.view(v).row_idx; };
  hipStream_t s = ctx->stream;
  int rc = SR_OK;

  const double* hs = ctx->h_outs.as<double>();
  const uint32_t* hf = reinterpret_cast<const uint32_t*>(ctx->h_outs.as<char>() + ctx->outs_flag_off);
  auto big_list = [&](const uint32_t* fl, std::vector<int64_t>* out) {
    for (int64_t t = 0; t < nt; ++t)
      if ((fl[t] & (SR_FLAG_NONFINITE | SR_FLAG_STATIC)) == 0 && (fl[t] & SR_FLAG_BIG)) out->push_back(t);
  };
  std::vector<int64_t> list;
  std::vector<uint8_t> list_ok;
  bool exact_done = false;
  if (c.res.early) {
    // (sr_ctx::exact_early) the flags are in pinned memory once ev_flags has fired — the last chunk's chain
    // still runs; the BIG trees' exact-sum pass is enqueued beside it, then the results' copy behind every
    // stream, and one synchronisation covers both
    rc = [&]() -> int {
      SR_HIP_CHECK(hipEventSynchronize(ctx->ev_flags));
      ctx->mark_phase(2);
      big_list(hf, &list);
      list_ok.assign(list.size(), 1);
      ctx->n_exact_last = int64_t(list.size());
      ctx->exact_kernel_ms = 0.0;
      int mc = 0;
      for (int64_t t : list) mc = std::max(mc, int(prog.n_checks[size_t(t)]));
      const std::vector<JlRange>& ranges = jl_ranges_cached(n_eval);
      // (one batch of the pass; a longer list — never seen — takes the pass after the synchronisation)
      const bool one_batch = mc > 0 && !ranges.empty() &&
                             list.size() <= std::max<size_t>(1, (size_t(256) << 20) / (size_t(mc) * ranges.size() * sizeof(T)));
      std::vector<uint8_t> fin(list.size() * size_t(std::max(mc, 1)));
      size_t fin_off = 0;
      hipStream_t xs = ctx->stream3;  // (no chain occupies it)
      if (one_batch) {
        SR_STAGE(run_exact<T>(ctx, q, prog, list.data(), int64_t(list.size()), mc, ranges, nullptr, fin.data(), 0, xs,
                              false, &fin_off));
        SR_HIP_CHECK(hipEventRecord(ctx->ev_join, xs));
        SR_HIP_CHECK(hipStreamWaitEvent(s, ctx->ev_join, 0));
      }
      SR_HIP_CHECK(hipMemcpyAsync(ctx->h_outs.p, ctx->outs.p, ctx->outs_bytes_all, hipMemcpyDeviceToHost, s));
      SR_HIP_CHECK(hipStreamSynchronize(s));
      if (one_batch) {
        const uint8_t* f = reinterpret_cast<const uint8_t*>(ctx->h_exact.as<char>() + fin_off);
        for (size_t i = 0; i < list.size(); ++i)
          for (int k = 0; k < mc; ++k) list_ok[i] &= f[i * size_t(mc) + size_t(k)];
        float km = 0.f;
        if (hipEventElapsedTime(&km, ctx->ev_k0, ctx->ev_k1) == hipSuccess) ctx->exact_kernel_ms += double(km);
      }
      exact_done = one_batch || mc == 0;
      return SR_OK;
    }();
    if (rc != SR_OK) {  // no launch or DMA of the call may outlive it
      (void)hipStreamSynchronize(s);
      if (ctx->stream2) (void)hipStreamSynchronize(ctx->stream2);
      if (ctx->stream3) (void)hipStreamSynchronize(ctx->stream3);
      return rc;
    }
  } else {
    SR_HIP_CHECK(hipStreamSynchronize(s));
  }
  if (!ctx->host_reductions.empty()) host_reduce_partials(ctx, nt);
  std::vector<double> sums(hs, hs + nt);
  std::vector<uint32_t> flags(hf, hf + nt);
  ctx->timing_pending = true;
  if (!c.res.early) {
    ctx->mark_phase(2);
    big_list(flags.data(), &list);
    list_ok.assign(list.size(), 1);
    ctx->n_exact_last = int64_t(list.size());
    ctx->exact_kernel_ms = 0.0;
  }
  for (int v = 0; v < n_views && !list.empty() && !exact_done; ++v) {  // (each view's listed trees over its own rows)
    std::vector<int64_t> lv;
    std::vector<size_t> at;
    for (size_t i = 0; i < list.size(); ++i)
      if (view_of(list[i]) == v) {
        lv.push_back(list[i]);
        at.push_back(i);
      }
    if (lv.empty()) continue;
    std::vector<uint8_t> ok;
    rc = exact_list_ok<T>(ctx, q.view(v), prog, lv, &ok, int64_t(v) * q.n_idx);
    if (rc != SR_OK) return rc;
    for (size_t i = 0; i < lv.size(); ++i) list_ok[at[i]] = ok[i];
  }
  ctx->mark_phase(3);
  std::vector<double> vden(static_cast<size_t>(n_views)), denoms;
  for (int v = 0; v < n_views; ++v) vden[size_t(v)] = view_denominator<T>(ds, rows_of(v), q.n_idx);
  if (views) {
    denoms.resize(size_t(nt));
    for (int64_t t = 0; t < nt; ++t) denoms[size_t(t)] = vden[size_t(view_of(t))];
  }
  std::vector<int64_t> fold_list;
  // the in-order fold's results (sr_ctx::ref_fold) and the reference's T denominators per view
  std::vector<T> tden(static_cast<size_t>(n_views));
  FoldResults<T> fres;
  const bool have_fold = c.res.fold_path != 0;
  if (have_fold) {
    for (int v = 0; v < n_views; ++v)
      tden[size_t(v)] = (ds->w && n_eval > 0) ? jl_wsum_view<T>(ds, rows_of(v), n_eval) : T(double(n_eval));
    fres.val = reinterpret_cast<const T*>(ctx->h_outs.as<char>() + ctx->outs_fval_off);
    fres.st = reinterpret_cast<const int32_t*>(ctx->h_outs.as<char>() + ctx->outs_fst_off);
    fres.den = [&](int64_t t) { return tden[size_t(view_of(t))]; };
    fres.debug_fail = ctx->fold_debug_fail;
  }
  finalize<T>(nt, sums.data(), flags.data(), vden[0], list.data(), int64_t(list.size()), list_ok.data(),
              static_cast<T*>(c.out_loss), c.out_complete, fold_terms(ds, n_eval, q.loss_kind), &fold_list,
              views ? denoms.data() : nullptr, have_fold ? &fres : nullptr);
  ctx->n_ref_ok_last = fres.n_ok;
  ctx->n_ref_fail_last = fres.n_fail;
  if (have_fold && ctx->fold_stats) {  // (analysis: slow segments, rounds, runs and walk time per folded tree)
    std::vector<int4> st(static_cast<size_t>(nt));
    if (hipMemcpy(st.data(), ctx->fold_dbg.p, st.size() * sizeof(int4), hipMemcpyDeviceToHost) == hipSuccess) {
      int64_t m = 0;
      double a[4] = {0, 0, 0, 0};
      int mx[4] = {0, 0, 0, 0};
      int64_t n_skip = 0;
      for (size_t i = 0; i < st.size(); ++i) {
        int4 v = st[i];
        if (v.x == 0 && v.y == 0 && v.z == 0) continue;
        n_skip += v.x % 1000;  // (x: slow segments x 1000 + those advanced by their steps)
        v.x /= 1000;
        ++m;
        if (v.z < 0)
          std::fprintf(stderr, "[sr fold] tree %zu failed: site %d after %d slow segments, %d rounds, %d us\n", i, -v.z,
                       v.x, v.y, v.w);
        const int w[4] = {v.x, v.y, v.z < 0 ? 0 : v.z, v.w};
        for (int i = 0; i < 4; ++i) {
          a[i] += w[i];
          mx[i] = std::max(mx[i], w[i]);
        }
      }
      std::fprintf(stderr, "[sr fold] path %d: %lld walks, mean/max slow segments %.1f/%d, rounds %.1f/%d, slow-segment us %.1f/%d, walk us %.1f/%d; folded %lld fallback %lld\n",
                   c.res.fold_path, (long long)m, m ? a[0] / m : 0.0, mx[0], m ? a[1] / m : 0.0, mx[1],
                   m ? a[2] / m : 0.0, mx[2], m ? a[3] / m : 0.0, mx[3], (long long)fres.n_ok, (long long)fres.n_fail);
      std::fprintf(stderr, "[sr fold] slow segments advanced by their steps (no rows read): %lld\n", (long long)n_skip);
    }
  }
  ctx->n_fold_last = int64_t(fold_list.size());
  ctx->fold_slow_last = ctx->fold_seg_last = 0;
  for (double& v : ctx->fold_ms) v = 0.0;
  for (int v = 0; v < n_views && !fold_list.empty(); ++v) {  // rare: the reference's own fold, in row order (sr_fold.h)
    std::vector<int64_t> fv;
    for (int64_t t : fold_list)
      if (view_of(t) == v) fv.push_back(t);
    if (fv.empty()) continue;
    std::vector<T> fold;
    rc = fold_exact<T>(ctx, q.view(v), n_eval, fv, &fold);
    if (rc != SR_OK) return rc;
    // mean: total / count, in T; weighted: total / sum(w), the reference's pairwise Base.sum in T
    const T den = (ds->w && n_eval > 0) ? jl_wsum_view<T>(ds, rows_of(v), n_eval) : T(vden[size_t(v)]);
    for (size_t i = 0; i < fv.size(); ++i) static_cast<T*>(c.out_loss)[fv[i]] = T(fold[i] / den);
  }
  ctx->mark_phase(4);
  auto t1 = std::chrono::steady_clock::now();
  ctx->last_total_ms = std::chrono::duration<double, std::milli>(t1 - c.t0).count();
  return SR_OK;
}

// The whole call (sr_eval_loss_batch / _views): submit, then finish.
template <typename T>
int eval_loss_impl(sr_ctx* ctx, const EvalReq& req, void* out_loss, uint8_t* out_complete) {
  LossCall<T> c;
  const int rc = eval_loss_submit<T>(ctx, req, out_loss, out_complete, &c);
  if (rc != SR_OK) return rc;
  return eval_loss_finish<T>(ctx, c);
}

template <typename T>
int eval_pred_impl(sr_ctx* ctx, const EvalReq& req, void* out_pred, uint8_t* out_complete) {
  const int64_t nt = req.trees->n_trees;
  if (nt > 0 && (!out_pred || !out_complete)) return set_error(SR_ERR_INVALID_ARG, "NULL output buffers");
  const int64_t n_eval = req.n_eval();
  SrProgramBatch<T> prog;
  BatchWants want;
  want.mode = SR_MODE_PRED;
  want.n_total = n_eval;
  BatchResult res;
  int rc = run_batch<T>(ctx, req, want, &prog, &res);
  if (rc != SR_OK) return rc;
  if (nt == 0) return SR_OK;
  hipStream_t s = ctx->stream;
  std::vector<double> sums(static_cast<size_t>(nt));
  std::vector<uint32_t> flags(static_cast<size_t>(nt));
  SR_HIP_CHECK(hipMemcpyAsync(out_pred, ctx->pred.p, size_t(nt) * size_t(n_eval) * sizeof(T), hipMemcpyDeviceToHost, s));
  SR_HIP_CHECK(hipMemcpyAsync(flags.data(), ctx->d_out_flag, size_t(nt) * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  SR_HIP_CHECK(hipStreamSynchronize(s));
  std::vector<int64_t> list;
  for (int64_t t = 0; t < nt; ++t)
    if ((flags[t] & (SR_FLAG_NONFINITE | SR_FLAG_STATIC)) == 0 && (flags[t] & SR_FLAG_BIG)) list.push_back(t);
  std::vector<uint8_t> list_ok;
  rc = exact_list_ok<T>(ctx, req, prog, list, &list_ok);
  if (rc != SR_OK) return rc;
  std::vector<T> dummy(static_cast<size_t>(nt));
  finalize<T>(nt, sums.data(), flags.data(), 1.0, list.data(), int64_t(list.size()), list_ok.data(), dummy.data(),
              out_complete);
  // statically incomplete trees have no program: fill their rows with NaN
  T* p = static_cast<T*>(out_pred);
  for (int64_t t = 0; t < nt; ++t)
    if (prog.static_bad[size_t(t)])
      for (int64_t i = 0; i < n_eval; ++i) p[size_t(t) * size_t(n_eval) + size_t(i)] = T(NAN);
  return SR_OK;
}

// The dead-tree probe's rows (sr_dataset::probe_rows): a tree that is non-finite on some row of the
// data is incomplete, and random trees go non-finite first on extreme inputs (exp of the largest
// values, division by and log of the values nearest zero), so those rows lead the probe.  X is
// Julia's column-major [nf, n] on the host.
template <typename T>
std::vector<int64_t> stress_rows(const T* X, int64_t nf, int64_t n) {
  const int64_t K = std::max<int64_t>(1, std::min<int64_t>(100, (kProbeRows * 3 / 4) / (3 * std::max<int64_t>(nf, 1))));
  std::vector<int64_t> pick;
  std::vector<int64_t> idx(static_cast<size_t>(n));
  for (int64_t f = 0; f < nf; ++f) {
    auto val = [&](int64_t i) { return double(X[size_t(i) * size_t(nf) + size_t(f)]); };
    auto mag = [&](int64_t i) { return std::fabs(val(i)); };
    auto take = [&](auto less) {
      for (int64_t i = 0; i < n; ++i) idx[size_t(i)] = i;
      std::nth_element(idx.begin(), idx.begin() + K, idx.end(), less);
      pick.insert(pick.end(), idx.begin(), idx.begin() + K);
    };
    // (NaN values order arbitrarily here; any row is a valid probe row)
    take([&](int64_t a, int64_t b) { return val(a) > val(b); });
    take([&](int64_t a, int64_t b) { return val(a) < val(b); });
    take([&](int64_t a, int64_t b) { return mag(a) < mag(b); });
  }
  std::sort(pick.begin(), pick.end());
  pick.erase(std::unique(pick.begin(), pick.end()), pick.end());
  if (int64_t(pick.size()) > kProbeRows) pick.resize(size_t(kProbeRows));
  for (int64_t i = 0; int64_t(pick.size()) < kProbeRows && i < n; ++i) pick.push_back(i);
  return pick;
}

template <typename T>
int upload_impl(sr_ctx* ctx, const void* X, int64_t nf, int64_t n, const void* y, const void* w, sr_dataset** out,
                const int32_t* cls = nullptr, int32_t n_classes = 0) {
  auto* ds = new sr_dataset();
  ds->n_classes = cls ? n_classes : 0;
  const int64_t nf_dev = nf + (cls ? 1 : 0);  // (the hidden class row after the user's features)
  ds->ctx = ctx;
  ds->dtype = sizeof(T) == 4 ? SR_DTYPE_F32 : SR_DTYPE_F64;
  ds->nf = nf;
  ds->n = n;
  ds->ld = ((n + kRowAlign - 1) / kRowAlign) * kRowAlign;
  hipStream_t s = ctx->stream;
  auto fail = [&](hipError_t e, const char* what) {
    if (ds->X) (void)hipFree(ds->X);
    if (ds->y) (void)hipFree(ds->y);
    if (ds->w) (void)hipFree(ds->w);
    if (ds->probe_rows) (void)hipFree(ds->probe_rows);
    delete ds;
    return set_error(SR_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
  };
  {
    const T* xh = static_cast<const T*>(X);
    double m = 0.0;
    bool bad = false;
    for (int64_t i = 0; i < nf * n; ++i) {
      const double v = std::fabs(double(xh[i]));
      bad |= !std::isfinite(v);
      m = v > m ? v : m;
    }
    ds->max_abs_x = bad ? double(INFINITY) : m;
  }
  hipError_t e;
  if ((e = hipMalloc(&ds->X, size_t(nf_dev) * size_t(ds->ld) * sizeof(T))) != hipSuccess) return fail(e, "hipMalloc X");
  void* tmp = nullptr;
  if ((e = hipMalloc(&tmp, size_t(nf) * size_t(n) * sizeof(T))) != hipSuccess) return fail(e, "hipMalloc staging");
  if ((e = hipMemcpyAsync(tmp, X, size_t(nf) * size_t(n) * sizeof(T), hipMemcpyHostToDevice, s)) != hipSuccess) {
    (void)hipFree(tmp);
    return fail(e, "copy X");
  }
  if ((e = sr_launch_transpose<T>(static_cast<const T*>(tmp), nf, n, ds->ld, static_cast<T*>(ds->X), s)) != hipSuccess) {
    (void)hipFree(tmp);
    return fail(e, "transpose X");
  }
  if ((e = hipStreamSynchronize(s)) != hipSuccess) {
    (void)hipFree(tmp);
    return fail(e, "sync");
  }
  (void)hipFree(tmp);
  if (cls) {
    // the class row: 0-based ids in T (exact: n_classes < 2^24), padded like every X row with row 0's value
    std::vector<T> row(static_cast<size_t>(ds->ld));
    for (int64_t i = 0; i < ds->ld; ++i) row[size_t(i)] = T(cls[i < n ? i : 0] - 1);
    if ((e = hipMemcpy(static_cast<T*>(ds->X) + size_t(nf) * size_t(ds->ld), row.data(), row.size() * sizeof(T),
                       hipMemcpyHostToDevice)) != hipSuccess)
      return fail(e, "copy classes");
  }
  if (y) {
    if ((e = hipMalloc(&ds->y, size_t(ds->ld) * sizeof(T))) != hipSuccess) return fail(e, "hipMalloc y");
    if ((e = hipMemcpyAsync(ds->y, y, size_t(n) * sizeof(T), hipMemcpyHostToDevice, s)) != hipSuccess) return fail(e, "copy y");
    if ((e = sr_launch_pad<T>(static_cast<T*>(ds->y), n, ds->ld, T(0), 1, s)) != hipSuccess) return fail(e, "pad y");
  }
  if (w) {
    const T* wh = static_cast<const T*>(w);
    ds->w_host.resize(size_t(n));
    double sum = 0.0, wmin = INFINITY;
    for (int64_t i = 0; i < n; ++i) {
      ds->w_host[size_t(i)] = double(wh[i]);
      sum += double(wh[i]);
      wmin = std::min(wmin, double(wh[i]));
    }
    ds->wsum = sum;
    ds->w_min = wmin;
    if ((e = hipMalloc(&ds->w, size_t(ds->ld) * sizeof(T))) != hipSuccess) return fail(e, "hipMalloc w");
    if ((e = hipMemcpyAsync(ds->w, w, size_t(n) * sizeof(T), hipMemcpyHostToDevice, s)) != hipSuccess) return fail(e, "copy w");
    if ((e = sr_launch_pad<T>(static_cast<T*>(ds->w), n, ds->ld, T(0), 0, s)) != hipSuccess) return fail(e, "pad w");
  }
  if (n >= 4 * kProbeRows) {
    const std::vector<int64_t> rows = stress_rows<T>(static_cast<const T*>(X), nf, n);
    if ((e = hipMalloc(&ds->probe_rows, rows.size() * sizeof(int64_t))) != hipSuccess) return fail(e, "hipMalloc probe rows");
    if ((e = hipMemcpy(ds->probe_rows, rows.data(), rows.size() * sizeof(int64_t), hipMemcpyHostToDevice)) != hipSuccess)
      return fail(e, "copy probe rows");
    ds->n_probe = int64_t(rows.size());
  }
  if ((e = hipStreamSynchronize(s)) != hipSuccess) return fail(e, "sync");
  *out = ds;
  return SR_OK;
}

// Batched forward-mode gradient (sr_eval_grad_batch): exact loss + complete flags from the loss
// kernel, then d loss / d constants of every complete tree from the tangent kernel.
template <typename T>
int eval_grad_impl(sr_ctx* ctx, const EvalReq& req, void* out_loss, void* out_grad, uint8_t* out_complete) {
  const sr_dataset* const ds = req.ds;
  const sr_tree_batch* const trees = req.trees;
  const SrOpset& ops = ctx->opsets[req.opset_id];
  for (uint32_t u : ops.unary)
    if (!sr_unary_grad_supported(u)) return set_error(SR_ERR_UNSUPPORTED_OP, "operator without a gradient rule");
  for (uint32_t b : ops.binary)
    if (!sr_binary_grad_supported(b)) return set_error(SR_ERR_UNSUPPORTED_OP, "operator without a gradient rule");
  // a parametric call (EvalReq::params; the entry point has checked the batch against the dataset): the
  // tree's tangents are its constants, then the parameters it uses (a compact rank: an unused parameter
  // makes no tangent, no window and no work item), and the gradient of tree t is [its nc constants | K x C
  // parameter entries, column-major] (sr_param_pack.h)
  const sr_param_batch* const pb = req.params;
  const bool parametric = pb != nullptr;
  int lkind = 0;
  double lparam = 0.0;
  const sr_ctx::LossExpr* lexpr = nullptr;  // (plain trees only: the loss pass below refuses a parametric call's)
  if (decode_loss(ctx, req.loss_kind, &lkind, &lparam, parametric ? nullptr : &lexpr) != SR_OK) return SR_ERR_INVALID_ARG;
  if (lexpr && !lexpr->p32.grad_ok)
    return set_error(SR_ERR_UNSUPPORTED_OP, "the loss expression uses an operator without a gradient rule");
  int rc = eval_loss_impl<T>(ctx, req, out_loss, out_complete);
  if (rc != SR_OK) return rc;
  const int64_t nt = trees->n_trees;
  if (nt == 0) return SR_OK;
  const bool gather = req.gather();
  const int64_t n_eval = req.n_eval();
  const int n_views = (req.views && gather) ? req.views->n_views : 1;
  auto view_of = [&](int64_t t) -> int { return n_views > 1 ? int(req.views->tree_view[t]) : 0; };
  const int64_t pK = parametric ? pb->max_parameters : 0, pC = parametric ? pb->n_classes : 0;
  const SrParamNodes pnodes{parametric ? pb->is_parameter : nullptr, parametric ? pb->parameter : nullptr,
                            int32_t(pK)};
  SrProgramBatch<T> prog;
  std::string err;
  const sr_scalar_ties* const ties = req.ties;
  rc = sr_compile_batch<T>(*trees, ops, n_eval, ds->nf, true, &prog, &err, nullptr, parametric ? &pnodes : nullptr, ties);
  if (rc != SR_OK) return set_error(rc, err);
  // tree t's differentiated scalars: its constants, or with ties its n_scalars (prog.n_consts then counts the
  // constant table's entries: the scalars, then the frozen constants)
  std::vector<uint32_t> ns(size_t(nt), 0u), ns_off(size_t(nt) + 1, 0u);
  for (int64_t t = 0; t < nt; ++t) {
    ns[size_t(t)] = ties ? uint32_t(ties->n_scalars[t]) : prog.n_consts[size_t(t)];
    ns_off[size_t(t) + 1] = ns_off[size_t(t)] + ns[size_t(t)];
  }
  std::vector<uint32_t> tan_off(size_t(nt) + 1, 0u), tan_par;
  if (parametric) {
    std::vector<uint32_t> used;
    for (int64_t t = 0; t < nt; ++t) {
      srpp::used_parameters(pb->is_parameter, pb->parameter, trees->degree, trees->offsets[t], trees->offsets[t + 1], &used);
      tan_par.insert(tan_par.end(), used.begin(), used.end());
      tan_off[size_t(t) + 1] = uint32_t(tan_par.size());
    }
  }
  // where tree t's gradient starts in out_grad
  auto goff = [&](int64_t t) -> size_t { return size_t(ns_off[size_t(t)]) + size_t(t) * size_t(pK * pC); };
  // pre-order constants of every tree (get_scalar_constants order)
  const T* vals = static_cast<const T*>(trees->val);
  std::vector<T> consts;
  consts.reserve(size_t(prog.const_off[size_t(nt)]));
  if (!ties) {
    for (int64_t t = 0; t < nt; ++t)
      for (int64_t i = trees->offsets[t]; i < trees->offsets[t + 1]; ++i)
        if (trees->degree[i] == 0 && trees->constant[i]) consts.push_back(vals[i]);
  } else {
    // the constant table per tree: scalar s at entry s (all its copies must hold one value), the frozen
    // constants behind them in pre-order — the indices the tied compile gave the operands.  A scalar without a
    // constant node in the tree (an unread entry of a parameter vector; a sub-expression called only inside
    // a dropped argument) keeps the entry 0: no operand names it, so its tangent and its derivative are 0
    consts.assign(size_t(prog.const_off[size_t(nt)]), T(0));
    std::vector<uint8_t> seen;
    size_t j = 0;  // constant node of the batch
    for (int64_t t = 0; t < nt; ++t) {
      T* tab = consts.data() + prog.const_off[size_t(t)];
      const uint32_t n_s = ns[size_t(t)];
      uint32_t frozen = 0;
      seen.assign(n_s, 0);
      for (int64_t i = trees->offsets[t]; i < trees->offsets[t + 1]; ++i) {
        if (!(trees->degree[i] == 0 && trees->constant[i])) continue;
        const int32_t sl = ties->slot[j++];
        if (sl < 0) {
          tab[n_s + frozen++] = vals[i];
        } else if (seen[size_t(sl)] && std::memcmp(&tab[sl], &vals[i], sizeof(T)) != 0) {
          return set_error(SR_ERR_INVALID_ARG, "tree " + std::to_string(t) + ": copies of scalar " + std::to_string(sl) +
                                                   " hold different values");
        } else {
          tab[sl] = vals[i];
          seen[size_t(sl)] = 1;
        }
      }
    }
  }
  T* g = static_cast<T*>(out_grad);
  std::fill(g, g + size_t(ns_off[size_t(nt)]) + size_t(nt) * size_t(pK * pC), T(0));
  // work items per tangent width: (tree, first constant)
  // tangent buckets: a tree runs with the narrowest width that holds its constants (1, 2, 4, 8; more
  // than 8: passes of 16), so a one-constant tree carries one tangent, not four
  constexpr int kNB = 5;
  std::vector<uint32_t> items[kNB], k0s[kNB];
  const int kts[kNB] = {1, 2, 4, 8, 16};
  for (int64_t t = 0; t < nt; ++t) {
    // (tangents: the constants and, in a parametric call, the used parameters behind them; the limit is
    //  one on constants, which live in the kernel's cval lanes)
    //  (ties: a plain call's windows cover the scalars alone; a parametric one's tangent positions are table
    //   entries, then the used parameters, and a window holding frozen constants only is left out)
    const uint32_t ntab = prog.n_consts[size_t(t)];
    const uint32_t nc = (parametric ? ntab : ns[size_t(t)]) + (tan_off[size_t(t) + 1] - tan_off[size_t(t)]);
    if (nc == 0 || !out_complete[t]) continue;
    if (ntab > 128) return set_error(SR_ERR_TOO_DEEP, "more than 128 constants in one tree");
    const int b = nc <= 1 ? 0 : (nc <= 2 ? 1 : (nc <= 4 ? 2 : (nc <= 8 ? 3 : 4)));
    for (uint32_t k0 = 0; k0 < nc; k0 += uint32_t(kts[b])) {
      if (k0 >= ns[size_t(t)] && k0 + uint32_t(kts[b]) <= ntab) continue;
      items[b].push_back(uint32_t(t));
      k0s[b].push_back(k0);
    }
  }
  // each bucket's items by estimated program cost, longest first (stable): the kWaves waves of a
  // workgroup share every row tile and wait for each other at its barrier, so items of similar cost go
  // together (an item's gradient does not depend on its position: bit-identical either way)
  if (ctx->grad_sort) {
    std::vector<double> tcost(size_t(nt), 0.0);
    for (int64_t t = 0; t < nt; ++t) {
      double c = 0.0;
      for (uint32_t i = prog.offsets[size_t(t)]; i < prog.offsets[size_t(t) + 1]; ++i) {
        const uint32_t opc = prog.code[i].op & SR_OP_MASK;
        const uint32_t u = opc >= SR_OP_UNARY_INF0 ? opc - SR_OP_UNARY_INF0 : opc - SR_OP_UNARY0;
        const bool transc = opc >= SR_OP_UNARY0 && opc < SR_OP_LOAD_DERIVED &&
                            (u == SR_U_EXP || u == SR_U_LOG || u == SR_U_COS || u == SR_U_SIN);
        c += transc ? 5.0 : 1.0;
      }
      tcost[size_t(t)] = c;
    }
    for (int b = 0; b < kNB; ++b) {
      std::vector<size_t> ord(items[b].size());
      for (size_t i = 0; i < ord.size(); ++i) ord[i] = i;
      std::stable_sort(ord.begin(), ord.end(), [&](size_t x, size_t y) { return tcost[items[b][x]] > tcost[items[b][y]]; });
      std::vector<uint32_t> it2(ord.size()), k2(ord.size());
      for (size_t i = 0; i < ord.size(); ++i) {
        it2[i] = items[b][ord[i]];
        k2[i] = k0s[b][ord[i]];
      }
      items[b].swap(it2);
      k0s[b].swap(k2);
    }
  }
  hipStream_t s = ctx->stream;
  // the loss pass's in-order folds re-upload their own view's rows: put every view's rows back
  if (gather && ctx->n_fold_last > 0) {
    SR_HIP_CHECK(ctx->row_idx.ensure(size_t(n_views) * size_t(req.n_idx) * sizeof(int64_t)));
    SR_HIP_CHECK(hipMemcpyAsync(ctx->row_idx.p, req.row_idx, size_t(n_views) * size_t(req.n_idx) * sizeof(int64_t),
                                hipMemcpyHostToDevice, s));
  }
  // several views: each bucket's work items ordered by view (stable), one segment per view; the
  // segments' tree groups (kWaves items each) and blocks are laid out below
  constexpr int kWaves = 4;
  std::vector<SrSegment> segs[kNB];
  if (n_views > 1)
    for (int b = 0; b < kNB; ++b) {
      std::vector<size_t> ord(items[b].size());
      for (size_t i = 0; i < ord.size(); ++i) ord[i] = i;
      std::stable_sort(ord.begin(), ord.end(), [&](size_t x, size_t y) { return view_of(items[b][x]) < view_of(items[b][y]); });
      std::vector<uint32_t> it2(ord.size()), k2(ord.size());
      for (size_t i = 0; i < ord.size(); ++i) {
        it2[i] = items[b][ord[i]];
        k2[i] = k0s[b][ord[i]];
      }
      items[b].swap(it2);
      k0s[b].swap(k2);
      for (size_t p = 0; p < items[b].size();) {
        const int v = view_of(items[b][p]);
        size_t q = p;
        while (q < items[b].size() && view_of(items[b][q]) == v) ++q;
        SrSegment sg{};
        sg.pos0 = int(p);
        sg.n_pos = int(q - p);
        sg.groups = int((q - p + kWaves - 1) / kWaves);
        sg.row_off = int64_t(v) * req.n_idx;
        segs[b].push_back(sg);
        p = q;
      }
    }
  // one pinned staging image (programs, offsets, constants, constant offsets, every bucket's work
  // items and segments) -> ONE upload; every bucket's kernel and reduce go out back to back, their
  // results come back in ONE copy, and the host waits once (round 3: four uploads, then per bucket an
  // upload, a copy back and a wait)
  auto al = [](size_t x) { return (x + 255) & ~size_t(255); };
  const size_t o_code = 0;
  const size_t o_offs = al(o_code + prog.code.size() * sizeof(SrIns<T>));
  const size_t o_cons = al(o_offs + prog.offsets.size() * sizeof(uint32_t));
  const size_t o_coff = al(o_cons + consts.size() * sizeof(T));
  size_t o_items[kNB], o_vals[kNB], o_segs[kNB];
  size_t at = al(o_coff + prog.const_off.size() * sizeof(uint32_t)), n_vals_all = 0;
  // parametric: the table [tree][parameter][class] (the loss pass's layout), the tangent lists, and per
  // bucket every item's first class bin (items in their final order) behind its work items
  size_t o_ptab = 0, o_toff = 0, o_tpar = 0, o_bins[kNB] = {};
  std::vector<uint32_t> item_bin[kNB];
  size_t n_bins[kNB] = {};
  if (parametric) {
    o_ptab = at;
    o_toff = al(o_ptab + size_t(nt) * size_t(pK * pC) * sizeof(T));
    o_tpar = al(o_toff + tan_off.size() * sizeof(uint32_t));
    at = al(o_tpar + tan_par.size() * sizeof(uint32_t));
    for (int b = 0; b < kNB; ++b) {
      item_bin[b].resize(items[b].size());
      for (size_t i = 0; i < items[b].size(); ++i) {
        const uint32_t t = items[b][i], k0 = k0s[b][i], ncs = prog.n_consts[t], nu = tan_off[t + 1] - tan_off[t];
        const uint32_t q0 = k0 < ncs ? ncs - k0 : 0u, q1 = std::min<uint32_t>(uint32_t(kts[b]), ncs + nu - k0);
        item_bin[b][i] = uint32_t(n_bins[b]);
        if (q1 > q0) n_bins[b] += size_t(q1 - q0) * size_t(pC);
      }
      if (n_bins[b] > size_t(0x7fffffff)) return set_error(SR_ERR_INVALID_ARG, "too many parameter bins");
    }
  }
  for (int b = 0; b < kNB; ++b) {
    o_items[b] = at;
    at = al(at + (parametric ? 3 : 2) * items[b].size() * sizeof(uint32_t));
    o_segs[b] = at;
    at = al(at + segs[b].size() * sizeof(SrSegment));
    o_vals[b] = n_vals_all;
    n_vals_all += items[b].size() * size_t(kts[b]);
    o_bins[b] = n_vals_all;
    n_vals_all += n_bins[b];
  }
  const size_t stage_bytes = at;
  SR_HIP_CHECK(ctx->g_code.ensure(stage_bytes + 16));
  SR_HIP_CHECK(ctx->h_grad.ensure(std::max(stage_bytes, n_vals_all * sizeof(double)) + 16, s, ctx->stream2));
  char* hs = ctx->h_grad.as<char>();
  if (!prog.code.empty()) std::memcpy(hs + o_code, prog.code.data(), prog.code.size() * sizeof(SrIns<T>));
  std::memcpy(hs + o_offs, prog.offsets.data(), prog.offsets.size() * sizeof(uint32_t));
  if (!consts.empty()) std::memcpy(hs + o_cons, consts.data(), consts.size() * sizeof(T));
  std::memcpy(hs + o_coff, prog.const_off.data(), prog.const_off.size() * sizeof(uint32_t));
  for (int b = 0; b < kNB; ++b) {
    uint32_t* d = reinterpret_cast<uint32_t*>(hs + o_items[b]);
    std::copy(items[b].begin(), items[b].end(), d);
    std::copy(k0s[b].begin(), k0s[b].end(), d + items[b].size());
    if (parametric) std::copy(item_bin[b].begin(), item_bin[b].end(), d + 2 * items[b].size());
  }
  if (parametric) {
    // (each tree's matrix [class][parameter] transposed, as run_batch's stage_param_table)
    T* hp = reinterpret_cast<T*>(hs + o_ptab);
    const T* src = static_cast<const T*>(pb->parameters);
    const size_t st = size_t(pK * pC);
    for (int64_t t = 0; t < nt; ++t)
      for (int64_t c = 0; c < pC; ++c)
        for (int64_t k = 0; k < pK; ++k) hp[size_t(t) * st + size_t(k * pC + c)] = src[size_t(t) * st + size_t(c * pK + k)];
    std::memcpy(hs + o_toff, tan_off.data(), tan_off.size() * sizeof(uint32_t));
    if (!tan_par.empty()) std::memcpy(hs + o_tpar, tan_par.data(), tan_par.size() * sizeof(uint32_t));
  }
  char* ds_ = ctx->g_code.as<char>();
  SR_HIP_CHECK(ctx->g_out.ensure(n_vals_all * sizeof(double) + 16));
  std::vector<double> vden(static_cast<size_t>(n_views));
  for (int v = 0; v < n_views; ++v) vden[size_t(v)] = view_denominator<T>(ds, req.view(v).row_idx, req.n_idx);
  size_t part_need = 0;
  struct Launch { int64_t n_rb, tiles_per_block, n_groups; int rows, depth; };
  Launch lc[kNB] = {};
  for (int b = 0; b < kNB; ++b) {
    const int64_t ni = int64_t(items[b].size());
    if (ni == 0) continue;
    const int kt = kts[b];
    // the bucket's own deepest program sizes its LDS operand stacks; rows per lane drop to 1 when the
    // default's tile + stacks would not fit (many features, Float64, deep trees: ADVICE r3)
    int bdepth = 1;
    for (uint32_t t : items[b]) bdepth = std::max(bdepth, int(prog.depth[t]));
    // (an expression-loss call: the one build per width, at the plain kernel's preferred rows per lane —
    //  "grad_rows" maps onto it; a tile that does not fit there is an error, not another kernel)
    const int lx_rows = sr_grad_param_rows(int(sizeof(T)), kt);
    const bool lx_fits = sr_grad_lds_bytes(int(sizeof(T)), kt, lx_rows, int(ds->nf), ds->w != nullptr, bdepth, kWaves) <= kLdsMax;
    const int rows = lexpr ? (lx_fits ? lx_rows : 0) : parametric ? sr_grad_param_launch_rows(int(sizeof(T)), kt, int(ds->nf), ds->w != nullptr, bdepth, kWaves,
                                                            kLdsMax, int(pC),
                                                            sr_grad_param_lane_slots(int(sizeof(T)), kt, int(pK), int(pC), ctx->grad_lane_bins != 0),
                                                            ctx->grad_rows_force)
                                : sr_grad_launch_rows(int(sizeof(T)), kt, int(ds->nf), ds->w != nullptr, bdepth, kWaves, kLdsMax,
                                                      ctx->grad_rows_force);
    if (rows == 0)
      return set_error(SR_ERR_TOO_DEEP, parametric ? "gradient tile and class bins need more than 160 KiB of LDS"
                                                   : "gradient tile needs more than 160 KiB of LDS");
    int64_t n_groups = (ni + kWaves - 1) / kWaves;
    if (!segs[b].empty()) {  // (view-pure groups: a few more than ni / kWaves)
      n_groups = 0;
      for (const SrSegment& sg : segs[b]) n_groups += sg.groups;
    }
    // row blocks in units of 512 rows (64 lanes x the largest rows per lane): they cover the same rows
    // whatever the rows per lane, and a lane accumulates its rows (lane mod 64) in row order inside a
    // block either way, so the gradients are bit-identical for every rows-per-lane choice
    constexpr int64_t kUnit = 512;
    const int64_t n_units = (n_eval + kUnit - 1) / kUnit;
    int64_t n_rb = (4096 + n_groups - 1) / n_groups;
    if (n_rb > n_units) n_rb = n_units;
    if (n_rb < 1) n_rb = 1;
    const int64_t units_per_block = (n_units + n_rb - 1) / n_rb;
    n_rb = (n_units + units_per_block - 1) / units_per_block;
    const int64_t tiles_per_block = units_per_block * (kUnit / int64_t(sr_grad_tile_rows(rows)));
    if (n_rb * n_groups > 0x7fffffff) return set_error(SR_ERR_INVALID_ARG, "grid too large");
    int64_t blk = 0;  // segments' first blocks
    for (SrSegment& sg : segs[b]) {
      sg.block0 = int(blk);
      blk += int64_t(sg.groups) * n_rb;
    }
    if (!segs[b].empty()) std::memcpy(hs + o_segs[b], segs[b].data(), segs[b].size() * sizeof(SrSegment));
    lc[b] = Launch{n_rb, tiles_per_block, n_groups, rows, bdepth};
    part_need = std::max(part_need, size_t(n_rb) * (size_t(ni) * size_t(kt) + n_bins[b]));
  }
  SR_HIP_CHECK(hipMemcpyAsync(ds_, hs, stage_bytes, hipMemcpyHostToDevice, s));
  // (buckets run one after another on the stream, so they share the partials buffer)
  SR_HIP_CHECK(ctx->g_part.ensure(part_need * sizeof(double) + 16));
  // algorithmic flops of each bucket's tangent kernel (bench.py's gradient roofline), per row of an
  // item (tree, first tangent) of KT tangents: each unary node 1 (value, transcendentals count 1) +
  // 1 (its derivative) + KT (tangents scaled), each binary node 1 + 2 (partials) + 2 KT (the
  // tangents' product and fused add), and the loss epilogue 3 (d loss / d pred, weight) + KT
  // accumulations; loads move data only
  static_assert(kNB == sr_ctx::kGradBuckets, "gradient buckets");
  for (int b = 0; b < kNB; ++b) {
    ctx->grad_timed[b] = false;
    ctx->grad_ms_done[b] = 0.0;
    ctx->grad_items[b] = int64_t(items[b].size());
    ctx->grad_rows[b] = lc[b].rows;
    double per_row = 0.0;
    const double kt = kts[b];
    for (uint32_t t : items[b]) {
      per_row += 3.0 + kt;
      for (uint32_t i = prog.offsets[t]; i < prog.offsets[t + 1]; ++i) {
        const uint32_t opc = prog.code[i].op & SR_OP_MASK;
        if (opc == SR_OP_LOAD_PARAM || opc == SR_OP_LOAD_PARAM_PUSH) continue;
        if (opc >= SR_OP_BINARY0) per_row += 3.0 + 2.0 * kt;
        else if (opc >= SR_OP_UNARY0 && opc < SR_OP_LOAD_DERIVED) per_row += 2.0 + kt;
      }
    }
    ctx->grad_flops[b] = per_row * double(n_eval);
  }
  for (int b = 0; b < kNB; ++b) {
    const int64_t ni = int64_t(items[b].size());
    if (ni == 0) continue;
    const int kt = kts[b];
    SrGradArgs<T> a{};
    a.code = reinterpret_cast<const SrIns<T>*>(ds_ + o_code);
    a.offsets = reinterpret_cast<const uint32_t*>(ds_ + o_offs);
    a.consts = reinterpret_cast<const T*>(ds_ + o_cons);
    a.const_off = reinterpret_cast<const uint32_t*>(ds_ + o_coff);
    a.item_tree = reinterpret_cast<const uint32_t*>(ds_ + o_items[b]);
    a.item_k0 = a.item_tree + ni;
    a.n_items = int(ni);
    a.X = static_cast<const T*>(ds->X);
    a.y = static_cast<const T*>(ds->y);
    a.w = static_cast<const T*>(ds->w);
    a.row_idx = gather ? ctx->row_idx.as<int64_t>() : nullptr;
    a.ld = ds->ld;
    a.n_rows = n_eval;
    a.nf = int(ds->nf);
    a.tiles_per_block = int(lc[b].tiles_per_block);
    a.n_row_blocks = int(lc[b].n_rb);
    a.n_groups = int(lc[b].n_groups);
    a.stack_depth = lc[b].depth;
    a.loss_kind = lkind;
    a.loss_param = T(lparam);
    a.part = ctx->g_part.as<double>();
    if (!segs[b].empty()) {
      a.segs = reinterpret_cast<const SrSegment*>(ds_ + o_segs[b]);
      a.n_segs = int(segs[b].size());
    }
    if (ctx->timing) SR_HIP_CHECK(hipEventRecord(ctx->ev_g0[b], s));
    SrGradParamArgs<T> pa{};
    if (parametric) {
      a.nf = int(ds->nf) + 1;  // (the hidden class row is staged too)
      pa.ptab = reinterpret_cast<const T*>(ds_ + o_ptab);
      pa.p_stride = int(pK * pC);
      pa.n_classes = int(pC);
      pa.tan_off = reinterpret_cast<const uint32_t*>(ds_ + o_toff);
      pa.tan_par = reinterpret_cast<const uint32_t*>(ds_ + o_tpar);
      pa.item_bin = a.item_tree + 2 * ni;
      pa.ppart = a.part + size_t(lc[b].n_rb) * size_t(ni) * size_t(kt);
      pa.n_bins = int(n_bins[b]);
      pa.lane_slots = sr_grad_param_lane_slots(int(sizeof(T)), kt, int(pK), int(pC), ctx->grad_lane_bins != 0);
      const int nblk = int(lc[b].n_rb * lc[b].n_groups);
      SR_HIP_CHECK(gather ? (sr_launch_grad_param_any<T, true>(a, pa, kt, lc[b].rows, nblk, s))
                          : (sr_launch_grad_param_any<T, false>(a, pa, kt, lc[b].rows, nblk, s)));
    } else if (lexpr) {
      const SrLossProgArgs<T> lx = lexpr->template args<T>();
      const int nblk = int(lc[b].n_rb * lc[b].n_groups);
      SR_HIP_CHECK(gather ? (sr_launch_grad_lossx_any<T, true>(a, lx, kt, lc[b].rows, nblk, s))
                          : (sr_launch_grad_lossx_any<T, false>(a, lx, kt, lc[b].rows, nblk, s)));
    } else {
      SR_HIP_CHECK(sr_launch_grad_any<T>(a, kt, gather, lc[b].rows, int(lc[b].n_rb * lc[b].n_groups), s));
    }
    if (ctx->timing) {
      SR_HIP_CHECK(hipEventRecord(ctx->ev_g1[b], s));
      ctx->grad_timed[b] = true;
    }
    SR_HIP_CHECK(sr_launch_grad_reduce(a.part, int(lc[b].n_rb), int(size_t(ni) * kt), ctx->g_out.as<double>() + o_vals[b], s));
    if (parametric)  // (the class bins: row blocks in order, as the constants' partials)
      SR_HIP_CHECK(sr_launch_grad_reduce(pa.ppart, int(lc[b].n_rb), pa.n_bins, ctx->g_out.as<double>() + o_bins[b], s));
  }
  double* out = ctx->h_grad.as<double>();  // (the staging image is no longer needed: the upload is done)
  SR_HIP_CHECK(hipMemcpyAsync(out, ctx->g_out.p, n_vals_all * sizeof(double), hipMemcpyDeviceToHost, s));
  SR_HIP_CHECK(hipStreamSynchronize(s));
  for (int b = 0; b < kNB; ++b) {
    const int kt = kts[b];
    for (size_t i = 0; i < items[b].size(); ++i) {
      const uint32_t t = items[b][i], k0 = k0s[b][i];
      const uint32_t nc = prog.n_consts[t];  // (where the parameter tangents start: the table's entries)
      for (int q = 0; q < kt && k0 + uint32_t(q) < ns[t]; ++q)
        g[goff(t) + k0 + uint32_t(q)] = T(out[o_vals[b] + i * size_t(kt) + size_t(q)] / vden[size_t(view_of(t))]);
      if (!parametric) continue;
      // the window's parameter tangents: bin (rank, class) -> entry nc + k + K class
      const uint32_t nu = tan_off[t + 1] - tan_off[t];
      const uint32_t q0 = k0 < nc ? nc - k0 : 0u, q1 = std::min<uint32_t>(uint32_t(kt), nc + nu - k0);
      for (uint32_t q = q0; q < q1; ++q) {
        const uint32_t k = tan_par[tan_off[t] + (k0 + q - nc)];
        for (int64_t c = 0; c < pC; ++c)
          g[goff(t) + ns[t] + size_t(k) + size_t(pK) * size_t(c)] =
              T(out[o_bins[b] + item_bin[b][i] + size_t(q - q0) * size_t(pC) + size_t(c)] / vden[size_t(view_of(t))]);
      }
    }
  }
  return SR_OK;
}

// Per-row derivatives (sr_eval_grad_tree_array / sr_eval_diff_tree_array): the predictions and
// their flags from the PRED path (eval_pred_impl: sr_eval_tree_array's, bit for bit), then every complete
// tree's tangents from the per-row build of the gradient kernel.  mode: the constants' tangents, the
// features', or one feature's per tree (direction, 1-based).
enum RowGradMode { kRowGradConsts = 0, kRowGradFeatures = 1, kRowGradDiff = 2 };
// (device staging of the tangents: work items (tree, window) are launched in chunks whose outputs stay within
// the "grad_stage_bytes" knob, 256 MiB — one item's own output when that is larger; results do not depend on it)

template <typename T>
int eval_row_grad_impl(sr_ctx* ctx, const EvalReq& req, int mode, const int32_t* direction, void* out_pred, void* out_grad,
                       uint8_t* out_complete) {
  const sr_dataset* const ds = req.ds;
  const sr_tree_batch* const trees = req.trees;
  const SrOpset& ops = ctx->opsets[req.opset_id];
  for (uint32_t u : ops.unary)
    if (!sr_unary_grad_supported(u)) return set_error(SR_ERR_UNSUPPORTED_OP, "operator without a gradient rule");
  for (uint32_t b : ops.binary)
    if (!sr_binary_grad_supported(b)) return set_error(SR_ERR_UNSUPPORTED_OP, "operator without a gradient rule");
  const int64_t nt = trees->n_trees;
  const int64_t n_eval = req.n_eval();
  const bool gather = req.gather();
  const bool feat = mode != kRowGradConsts;
  constexpr int kNB = sr_ctx::kGradBuckets;
  constexpr int kWaves = 4;
  const int kts[kNB] = {1, 2, 4, 8, 16};
  for (int b = 0; b < kNB; ++b) {
    ctx->grad_timed[b] = false;
    ctx->grad_ms_done[b] = 0.0;
    ctx->grad_flops[b] = 0.0;
    ctx->grad_items[b] = 0;
    ctx->grad_rows[b] = 0;
  }
  int rc = eval_pred_impl<T>(ctx, req, out_pred, out_complete);
  if (rc != SR_OK) return rc;
  if (nt == 0) return SR_OK;
  SrProgramBatch<T> prog;
  std::string err;
  rc = sr_compile_batch<T>(*trees, ops, n_eval, ds->nf, true, &prog, &err, nullptr, nullptr);
  if (rc != SR_OK) return set_error(rc, err);
  // tree t's tangents and where its [n_grad_t][n_eval] block starts in out_grad
  auto n_grad = [&](int64_t t) -> uint32_t {
    return mode == kRowGradConsts ? prog.n_consts[size_t(t)] : (mode == kRowGradFeatures ? uint32_t(ds->nf) : 1u);
  };
  std::vector<size_t> goff(size_t(nt) + 1, 0);
  for (int64_t t = 0; t < nt; ++t) goff[size_t(t) + 1] = goff[size_t(t)] + size_t(n_grad(t)) * size_t(n_eval);
  T* g = static_cast<T*>(out_grad);
  auto zero_tree = [&](int64_t t) { std::fill(g + goff[size_t(t)], g + goff[size_t(t) + 1], T(0)); };
  const T* vals = static_cast<const T*>(trees->val);
  std::vector<T> consts;
  consts.reserve(size_t(prog.const_off[size_t(nt)]));
  for (int64_t t = 0; t < nt; ++t)
    for (int64_t i = trees->offsets[t]; i < trees->offsets[t + 1]; ++i)
      if (trees->degree[i] == 0 && trees->constant[i]) consts.push_back(vals[i]);
  // work items in tree order: (tree, first tangent, tangents of the window that are the tree's, bucket)
  struct Item { uint32_t t, k0, nq; int b; };
  std::vector<Item> all;
  for (int64_t t = 0; t < nt; ++t) {
    const uint32_t ng = n_grad(t);
    if (ng == 0) continue;
    if (!out_complete[t]) {
      zero_tree(t);
      continue;
    }
    if (prog.n_consts[size_t(t)] > 128) return set_error(SR_ERR_TOO_DEEP, "more than 128 constants in one tree");
    if (mode == kRowGradDiff) {
      all.push_back(Item{uint32_t(t), uint32_t(direction[t] - 1), 1u, 0});
      continue;
    }
    const int b = ng <= 1 ? 0 : (ng <= 2 ? 1 : (ng <= 4 ? 2 : (ng <= 8 ? 3 : 4)));
    for (uint32_t k0 = 0; k0 < ng; k0 += uint32_t(kts[b]))
      all.push_back(Item{uint32_t(t), k0, std::min<uint32_t>(uint32_t(kts[b]), ng - k0), b});
  }
  if (all.empty()) return SR_OK;
  // rows per lane per bucket, over the call's deepest program of that bucket (so they do not depend on the
  // chunking either); the tile stages X alone (y's place is kept, no weights)
  int bdepth[kNB] = {1, 1, 1, 1, 1}, rows[kNB] = {};
  bool used[kNB] = {};
  for (const Item& it : all) {
    used[it.b] = true;
    bdepth[it.b] = std::max(bdepth[it.b], int(prog.depth[it.t]));
  }
  for (int b = 0; b < kNB; ++b) {
    if (!used[b]) continue;
    rows[b] = sr_grad_launch_rows(int(sizeof(T)), kts[b], int(ds->nf), false, bdepth[b], kWaves, kLdsMax, ctx->grad_rows_force);
    if (rows[b] == 0)
      return set_error(SR_ERR_INVALID_ARG, "per-row derivatives: " + std::to_string(ds->nf) + " features and operand stacks of depth " +
                                               std::to_string(bdepth[b]) + " need more than 160 KiB of LDS at one row per lane");
    ctx->grad_rows[b] = rows[b];
  }
  hipStream_t s = ctx->stream;
  if (gather) {
    SR_HIP_CHECK(ctx->row_idx.ensure(size_t(req.n_idx) * sizeof(int64_t)));
    SR_HIP_CHECK(hipMemcpyAsync(ctx->row_idx.p, req.row_idx, size_t(req.n_idx) * sizeof(int64_t), hipMemcpyHostToDevice, s));
  }
  // the programs and constants: one image, uploaded once
  auto al = [](size_t x) { return (x + 255) & ~size_t(255); };
  const size_t o_code = 0;
  const size_t o_offs = al(o_code + prog.code.size() * sizeof(SrIns<T>));
  const size_t o_cons = al(o_offs + prog.offsets.size() * sizeof(uint32_t));
  const size_t o_coff = al(o_cons + consts.size() * sizeof(T));
  const size_t prog_bytes = al(o_coff + prog.const_off.size() * sizeof(uint32_t));
  SR_HIP_CHECK(ctx->g_code.ensure(prog_bytes + 16));
  SR_HIP_CHECK(ctx->h_grad.ensure(prog_bytes + 16, s, ctx->stream2));
  {
    char* hs = ctx->h_grad.as<char>();
    if (!prog.code.empty()) std::memcpy(hs + o_code, prog.code.data(), prog.code.size() * sizeof(SrIns<T>));
    std::memcpy(hs + o_offs, prog.offsets.data(), prog.offsets.size() * sizeof(uint32_t));
    if (!consts.empty()) std::memcpy(hs + o_cons, consts.data(), consts.size() * sizeof(T));
    std::memcpy(hs + o_coff, prog.const_off.data(), prog.const_off.size() * sizeof(uint32_t));
    SR_HIP_CHECK(hipMemcpyAsync(ctx->g_code.p, hs, prog_bytes, hipMemcpyHostToDevice, s));
    SR_HIP_CHECK(hipStreamSynchronize(s));  // (the chunks below reuse no part of h_grad, but it may grow elsewhere)
  }
  const char* dprog = ctx->g_code.as<char>();
  // row blocks as the gradient call's: units of 512 rows
  constexpr int64_t kUnit = 512;
  const int64_t n_units = (n_eval + kUnit - 1) / kUnit;
  const size_t chunk_elems = std::max<size_t>(size_t(ctx->grad_stage_bytes) / sizeof(T), 1);
  std::vector<uint8_t> tree_bad(size_t(nt), 0);
  std::vector<uint32_t> himg, hbad;
  for (size_t c0 = 0; c0 < all.size();) {
    // the chunk: items c0 .. c1 - 1, their outputs packed in item order
    size_t c1 = c0, elems = 0;
    while (c1 < all.size() && (c1 == c0 || elems + size_t(all[c1].nq) * size_t(n_eval) <= chunk_elems)) {
      elems += size_t(all[c1].nq) * size_t(n_eval);
      ++c1;
    }
    std::vector<uint32_t> items[kNB], k0s[kNB], nqs[kNB];
    std::vector<uint64_t> outs[kNB];
    std::vector<size_t> src[kNB];  // (the item's index in `all`)
    {
      size_t at_out = 0;
      for (size_t i = c0; i < c1; ++i) {
        const Item& it = all[i];
        items[it.b].push_back(it.t);
        k0s[it.b].push_back(it.k0);
        nqs[it.b].push_back(it.nq);
        outs[it.b].push_back(uint64_t(at_out));
        src[it.b].push_back(i);
        at_out += size_t(it.nq) * size_t(n_eval);
      }
    }
    // the chunk's image: per bucket {item_out u64 | item_tree | item_k0 | item_nq}
    size_t o_items[kNB], at = 0, o_bad[kNB], n_bad = 0;
    struct Launch { int64_t n_rb, tiles_per_block, n_groups; };
    Launch lc[kNB] = {};
    for (int b = 0; b < kNB; ++b) {
      o_items[b] = at;
      const size_t ni = items[b].size();
      at = al(at + ni * (sizeof(uint64_t) + 3 * sizeof(uint32_t)));
      o_bad[b] = n_bad;
      if (ni == 0) continue;
      const int64_t n_groups = (int64_t(ni) + kWaves - 1) / kWaves;
      int64_t n_rb = (4096 + n_groups - 1) / n_groups;
      if (n_rb > n_units) n_rb = n_units;
      if (n_rb < 1) n_rb = 1;
      const int64_t units_per_block = (n_units + n_rb - 1) / n_rb;
      n_rb = (n_units + units_per_block - 1) / units_per_block;
      if (n_rb * n_groups > 0x7fffffff) return set_error(SR_ERR_INVALID_ARG, "grid too large");
      lc[b] = Launch{n_rb, units_per_block * (kUnit / int64_t(sr_grad_tile_rows(rows[b]))), n_groups};
      n_bad += size_t(n_rb) * ni;
    }
    himg.assign(at / sizeof(uint32_t) + 4, 0u);
    for (int b = 0; b < kNB; ++b) {
      const size_t ni = items[b].size();
      if (ni == 0) continue;
      char* d = reinterpret_cast<char*>(himg.data()) + o_items[b];
      std::memcpy(d, outs[b].data(), ni * sizeof(uint64_t));
      uint32_t* u = reinterpret_cast<uint32_t*>(d + ni * sizeof(uint64_t));
      std::copy(items[b].begin(), items[b].end(), u);
      std::copy(k0s[b].begin(), k0s[b].end(), u + ni);
      std::copy(nqs[b].begin(), nqs[b].end(), u + 2 * ni);
    }
    SR_HIP_CHECK(ctx->g_items.ensure(at + 16));
    SR_HIP_CHECK(ctx->g_out.ensure(elems * sizeof(T) + 16));
    SR_HIP_CHECK(ctx->g_part.ensure(n_bad * sizeof(uint32_t) + 16));
    SR_HIP_CHECK(hipMemcpyAsync(ctx->g_items.p, himg.data(), at, hipMemcpyHostToDevice, s));
    SR_HIP_CHECK(hipMemsetAsync(ctx->g_part.p, 0, n_bad * sizeof(uint32_t), s));
    bool timed[kNB] = {};
    for (int b = 0; b < kNB; ++b) {
      const int64_t ni = int64_t(items[b].size());
      if (ni == 0) continue;
      SrGradArgs<T> a{};
      a.code = reinterpret_cast<const SrIns<T>*>(dprog + o_code);
      a.offsets = reinterpret_cast<const uint32_t*>(dprog + o_offs);
      a.consts = reinterpret_cast<const T*>(dprog + o_cons);
      a.const_off = reinterpret_cast<const uint32_t*>(dprog + o_coff);
      const char* di = ctx->g_items.as<char>() + o_items[b];
      SrGradRowArgs<T> d{};
      d.item_out = reinterpret_cast<const uint64_t*>(di);
      a.item_tree = reinterpret_cast<const uint32_t*>(di + size_t(ni) * sizeof(uint64_t));
      a.item_k0 = a.item_tree + ni;
      d.item_nq = a.item_tree + 2 * ni;
      a.n_items = int(ni);
      a.X = static_cast<const T*>(ds->X);
      a.row_idx = gather ? ctx->row_idx.as<int64_t>() : nullptr;
      a.ld = ds->ld;
      a.n_rows = n_eval;
      a.nf = int(ds->nf);
      a.tiles_per_block = int(lc[b].tiles_per_block);
      a.n_row_blocks = int(lc[b].n_rb);
      a.n_groups = int(lc[b].n_groups);
      a.stack_depth = bdepth[b];
      d.out = ctx->g_out.as<T>();
      d.bad = ctx->g_part.as<uint32_t>() + o_bad[b];
      d.feat = feat ? 1 : 0;
      if (ctx->timing) SR_HIP_CHECK(hipEventRecord(ctx->ev_g0[b], s));
      const int nblk = int(lc[b].n_rb * lc[b].n_groups);
      SR_HIP_CHECK(gather ? (sr_launch_grad_rows_any<T, true>(a, d, kts[b], rows[b], nblk, s))
                          : (sr_launch_grad_rows_any<T, false>(a, d, kts[b], rows[b], nblk, s)));
      if (ctx->timing) {
        SR_HIP_CHECK(hipEventRecord(ctx->ev_g1[b], s));
        timed[b] = true;
      }
      ctx->grad_items[b] += ni;
      // (algorithmic flops as the gradient call counts them, without the loss epilogue)
      double per_row = 0.0;
      const double kt = kts[b];
      for (uint32_t t : items[b])
        for (uint32_t i = prog.offsets[t]; i < prog.offsets[t + 1]; ++i) {
          const uint32_t opc = prog.code[i].op & SR_OP_MASK;
          if (opc >= SR_OP_BINARY0) per_row += 3.0 + 2.0 * kt;
          else if (opc >= SR_OP_UNARY0 && opc < SR_OP_LOAD_DERIVED) per_row += 2.0 + kt;
        }
      ctx->grad_flops[b] += per_row * double(n_eval);
    }
    // the chunk's tangents to the caller's array: runs of items whose blocks follow each other there too
    hbad.assign(n_bad + 1, 0u);
    SR_HIP_CHECK(hipMemcpyAsync(hbad.data(), ctx->g_part.p, n_bad * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    auto host_off = [&](const Item& it) {
      return goff[it.t] + (mode == kRowGradDiff ? size_t(0) : size_t(it.k0) * size_t(n_eval));
    };
    {
      size_t dev0 = 0, dev_at = 0, h0 = host_off(all[c0]), h_at = h0;
      for (size_t i = c0; i <= c1; ++i) {
        if (i == c1 || host_off(all[i]) != h_at) {
          if (dev_at > dev0)
            SR_HIP_CHECK(hipMemcpyAsync(g + h0, ctx->g_out.as<T>() + dev0, (dev_at - dev0) * sizeof(T), hipMemcpyDeviceToHost, s));
          if (i == c1) break;
          dev0 = dev_at;
          h0 = h_at = host_off(all[i]);
        }
        const size_t ne = size_t(all[i].nq) * size_t(n_eval);
        dev_at += ne;
        h_at += ne;
      }
    }
    SR_HIP_CHECK(hipStreamSynchronize(s));
    for (int b = 0; b < kNB; ++b) {
      float m = 0.f;
      if (timed[b] && hipEventElapsedTime(&m, ctx->ev_g0[b], ctx->ev_g1[b]) == hipSuccess) ctx->grad_ms_done[b] += double(m);
      const size_t ni = items[b].size();
      for (int64_t r = 0; r < lc[b].n_rb; ++r)
        for (size_t i = 0; i < ni; ++i)
          if (hbad[o_bad[b] + size_t(r) * ni + i]) tree_bad[items[b][i]] = 1;
    }
    c0 = c1;
  }
  // a tree with a non-finite derivative element is incomplete: its derivatives are zero, as an
  // incomplete tree's gradient is
  for (int64_t t = 0; t < nt; ++t)
    if (tree_bad[size_t(t)]) {
      out_complete[t] = 0;
      zero_tree(t);
    }
  return SR_OK;
}

int tier_of(const SrOpset& o) {
  auto basic_u = [](uint32_t u) {
    return u == SR_U_NEG || u == SR_U_SQUARE || u == SR_U_CUBE || u == SR_U_EXP || u == SR_U_COS ||
           u == SR_U_SIN || u == SR_U_LOG || u == SR_U_SQRT || u == SR_U_ABS;
  };
  auto basic_b = [](uint32_t b) { return b == SR_B_ADD || b == SR_B_SUB || b == SR_B_MUL || b == SR_B_DIV; };
  for (uint32_t u : o.unary)
    if (!basic_u(u)) return SR_TIER_FULL;
  for (uint32_t b : o.binary)
    if (!basic_b(b)) return SR_TIER_FULL;
  return SR_TIER_BASIC;
}

// ---------------------------------------------------------------- multi-GPU
std::atomic<uint64_t> g_comm_gen{0};

#define SR_NCCL_CHECK(expr)                                                                         \
  do {                                                                                              \
    const ncclResult_t _r = (expr);                                                                 \
    if (_r != ncclSuccess) return set_error(SR_ERR_HIP, std::string(#expr) + ": " + ncclGetErrorString(_r)); \
  } while (0)

// The file a symbol was loaded from (dladdr), with symlinks resolved.
std::string so_path(const void* sym) {
  Dl_info info{};
  if (!dladdr(sym, &info) || !info.dli_fname) return "?";
  char buf[PATH_MAX];
  return realpath(info.dli_fname, buf) ? std::string(buf) : std::string(info.dli_fname);
}
std::string dir_of(const std::string& p) {
  const size_t k = p.rfind('/');
  return k == std::string::npos ? std::string() : p.substr(0, k);
}
// The HIP runtime and the RCCL this library's calls bind to.  The dynamic loader reuses an already
// loaded soname, so when a process loaded torch's bundled ROCm first, the library runs on torch's
// HIP and RCCL, otherwise on /opt/rocm's: either way the two must come from ONE tree, because RCCL
// is handed this library's streams and device buffers.
std::string runtime_paths() {
  return "hip=" + so_path(reinterpret_cast<const void*>(&hipStreamSynchronize)) +
         ";rccl=" + so_path(reinterpret_cast<const void*>(&ncclAllReduce));
}
int check_runtime_pair() {
  const std::string hip = so_path(reinterpret_cast<const void*>(&hipStreamSynchronize));
  const std::string rccl = so_path(reinterpret_cast<const void*>(&ncclAllReduce));
  if (dir_of(hip) != dir_of(rccl))
    return set_error(SR_ERR_HIP, "the HIP runtime (" + hip + ") and RCCL (" + rccl +
                                     ") come from different ROCm trees: RCCL would run this library's streams "
                                     "on another runtime; load libsr_amd before anything else that loads HIP");
  return SR_OK;
}

// The sharded calls' data-path transport: the library's own RCCL communicator over xGMI
// (sr_comm_init), or collectives the caller registers (sr_comm_init_host: host callbacks such as a gloo
// group — several ranks can then share one GPU, and they run this same code).  Buffers are device
// memory on the library's stream; a call returns once its result is usable on that stream.
struct SrComm {
  int nranks = 1, rank = 0;
  virtual ~SrComm() = default;
  virtual const char* kind() const = 0;
  virtual int allreduce_sum(double* d, size_t n, hipStream_t s) = 0;                     // in place
  virtual int allgather(const void* send, void* recv, size_t bytes, hipStream_t s) = 0;  // recv[nranks][bytes]
};

struct SrRcclComm final : SrComm {
  ncclComm_t comm = nullptr;
  ~SrRcclComm() override {
    if (comm) (void)ncclCommDestroy(comm);
  }
  const char* kind() const override { return "rccl"; }
  int allreduce_sum(double* d, size_t n, hipStream_t s) override {
    SR_NCCL_CHECK(ncclAllReduce(d, d, n, ncclDouble, ncclSum, comm, s));
    return SR_OK;
  }
  int allgather(const void* send, void* recv, size_t bytes, hipStream_t s) override {
    SR_NCCL_CHECK(ncclAllGather(send, recv, bytes, ncclChar, comm, s));
    return SR_OK;
  }
};

// Host callbacks: the buffers are staged through host memory.  A failed staging copy still calls the
// callback, with this rank's contribution poisoned (NaN bytes): every caller appends an error word to
// its payload, which then reads non-zero on every rank.  A rank never skips a collective its peers
// enter.
struct SrHostComm final : SrComm {
  sr_host_allreduce_fn ar = nullptr;
  sr_host_allgather_fn ag = nullptr;
  void* user = nullptr;
  std::vector<char> h_send, h_recv;
  const char* kind() const override { return "host"; }
  int allreduce_sum(double* d, size_t n, hipStream_t s) override {
    h_send.resize(n * sizeof(double));
    const bool staged = hipMemcpyAsync(h_send.data(), d, h_send.size(), hipMemcpyDeviceToHost, s) == hipSuccess &&
                        hipStreamSynchronize(s) == hipSuccess;
    if (!staged) std::memset(h_send.data(), 0xff, h_send.size());
    if (ar(user, reinterpret_cast<double*>(h_send.data()), int64_t(n)) != 0)
      return set_error(SR_ERR_HIP, "the host all-reduce callback failed");
    SR_HIP_CHECK(hipMemcpyAsync(d, h_send.data(), h_send.size(), hipMemcpyHostToDevice, s));
    SR_HIP_CHECK(hipStreamSynchronize(s));
    return staged ? SR_OK : set_error(SR_ERR_HIP, "staging the all-reduce buffer failed");
  }
  int allgather(const void* send, void* recv, size_t bytes, hipStream_t s) override {
    h_send.resize(bytes);
    h_recv.resize(bytes * size_t(nranks));
    const bool staged = hipMemcpyAsync(h_send.data(), send, bytes, hipMemcpyDeviceToHost, s) == hipSuccess &&
                        hipStreamSynchronize(s) == hipSuccess;
    if (!staged) std::memset(h_send.data(), 0xff, bytes);
    if (ag(user, h_send.data(), h_recv.data(), int64_t(bytes)) != 0)
      return set_error(SR_ERR_HIP, "the host all-gather callback failed");
    SR_HIP_CHECK(hipMemcpyAsync(recv, h_recv.data(), h_recv.size(), hipMemcpyHostToDevice, s));
    SR_HIP_CHECK(hipStreamSynchronize(s));
    return staged ? SR_OK : set_error(SR_ERR_HIP, "staging the all-gather buffer failed");
  }
};

// A buffer of a sharded call's collectives, grown before the collective.  Growth happens on every rank
// at the same call (the sizes depend only on the batch and the number of ranks, and the collective
// buffers serve the collective calls alone), so whether a call grows a buffer is the same on every
// rank; a call that grows one first agrees on the outcome (agree below).  ctx->inject_fail (tests,
// sr_set_tuning "inject_failure") makes the next growths fail on this rank.
struct Prep {
  sr_ctx* ctx;
  bool grew = false;
  int rc = SR_OK;
  std::vector<DevBuf*> touched;
  std::vector<HostBuf*> touched_host;
  bool inject() {
    if (ctx->inject_fail <= 0) return false;
    --ctx->inject_fail;
    return true;
  }
  void fail(hipError_t e) {
    if (e != hipSuccess && rc == SR_OK) rc = set_error(SR_ERR_HIP, std::string("collective buffer: ") + hipGetErrorString(e));
  }
  void need(DevBuf& b, size_t bytes) {
    if (bytes <= b.cap) return;
    grew = true;
    touched.push_back(&b);
    if (rc != SR_OK) return;
    if (inject()) {
      b.release();
      fail(hipErrorOutOfMemory);
    } else {
      fail(b.ensure(bytes));
    }
  }
  void need(HostBuf& b, size_t bytes) {  // (pinned staging of a collective's results)
    if (bytes <= b.cap) return;
    grew = true;
    touched_host.push_back(&b);
    if (rc != SR_OK) return;
    if (inject()) {
      b.release();
      fail(hipErrorOutOfMemory);
    } else {
      fail(b.ensure(bytes, ctx->stream, ctx->stream2));
    }
  }
};

// Every rank's readiness before a collective: one Σ of error words (a rank whose preparation failed
// still enters it), so either every rank proceeds or every rank returns an error.
int agree(sr_ctx* ctx, int local, const char* what = "failed to prepare its collective buffers") {
  hipStream_t s = ctx->stream;
  double* d = ctx->ctl.as<double>();
  double e = local != SR_OK ? 1.0 : 0.0;
  double sum = 0.0;
  bool set = hipMemcpyAsync(d, &e, sizeof(double), hipMemcpyHostToDevice, s) == hipSuccess;
  if (!set) {  // the word must not be stale: poison it synchronously, so every peer sees a non-zero sum
    e = 1.0;
    (void)hipMemcpy(d, &e, sizeof(double), hipMemcpyHostToDevice);
  }
  int rc = ctx->xport->allreduce_sum(d, 1, s);
  bool got = false;
  if (rc == SR_OK) got = hipMemcpyAsync(&sum, d, sizeof(double), hipMemcpyDeviceToHost, s) == hipSuccess &&
                         hipStreamSynchronize(s) == hipSuccess;
  if (local != SR_OK) return local;
  if (!set) return set_error(SR_ERR_HIP, "error word upload failed");
  if (rc != SR_OK) return rc;
  if (!got) return set_error(SR_ERR_HIP, "agreement: copy of the error sum failed");
  if (sum != 0.0) return set_error(SR_ERR_HIP, std::string("a peer rank ") + what);
  return SR_OK;
}
// Grown buffers are agreed on; after a failure every rank releases them, so the next call grows them
// on every rank again (the ranks' buffer states stay identical).
int agree_prep(sr_ctx* ctx, Prep& p) {
  if (!p.grew) return SR_OK;
  const int rc = agree(ctx, p.rc);
  if (rc != SR_OK) {
    for (DevBuf* b : p.touched) b->release();
    for (HostBuf* b : p.touched_host) b->release();
  }
  return rc;
}

constexpr int kLayoutWords = 6;
// Every shard's rows, Σw, max|X| and smallest weight (one all-gather per dataset and communicator; its buffer is
// prepared and agreed on by the caller).  Collective: a local failure still enters the all-gather,
// with its error word set.
int shard_layout(sr_ctx* ctx, const sr_dataset* ds) {
  constexpr int K = kLayoutWords;
  const int nr = ctx->comm_ranks;
  hipStream_t s = ctx->stream;
  // n, Σw, max|X|, weighted, min w, error word
  double mine[K] = {double(ds->n), ds->w ? ds->wsum : 0.0, ds->max_abs_x, ds->w ? 1.0 : 0.0, ds->w ? ds->w_min : 0.0, 0.0};
  double* d = ctx->coll_buf.as<double>();
  if (hipMemcpyAsync(d, mine, sizeof(mine), hipMemcpyHostToDevice, s) != hipSuccess) {
    mine[K - 1] = 1.0;
    (void)hipMemcpy(d, mine, sizeof(mine), hipMemcpyHostToDevice);
  }
  int rc = ctx->xport->allgather(d, d + K, K * sizeof(double), s);
  if (rc != SR_OK) return rc;
  std::vector<double> all(size_t(K) * size_t(nr));
  SR_HIP_CHECK(hipMemcpyAsync(all.data(), d + K, all.size() * sizeof(double), hipMemcpyDeviceToHost, s));
  SR_HIP_CHECK(hipStreamSynchronize(s));
  std::vector<int64_t> offs(size_t(nr) + 1, 0);
  double wsum = 0.0, mx = 0.0, wmin = INFINITY;
  int64_t mn = INT64_MAX;
  int weighted = 0;
  for (int r = 0; r < nr; ++r) {
    const double* a = all.data() + size_t(K) * size_t(r);
    if (a[K - 1] != 0.0) return set_error(SR_ERR_HIP, "the shard layout exchange failed on rank " + std::to_string(r));
    const int64_t n = int64_t(a[0]);
    offs[size_t(r) + 1] = offs[size_t(r)] + n;
    wsum += a[1];
    mx = (a[2] > mx || a[2] != a[2]) ? a[2] : mx;  // NaN / Inf (non-finite data) propagate
    mn = std::min(mn, n);
    weighted += a[3] != 0.0 ? 1 : 0;
    wmin = std::min(wmin, a[4]);
  }
  if (weighted != 0 && weighted != nr) return set_error(SR_ERR_INVALID_ARG, "some shards have weights and some do not");
  if (int64_t(all[size_t(K) * size_t(ctx->comm_rank)]) != ds->n) return set_error(SR_ERR_INVALID_ARG, "shard layout exchange failed");
  ds->shard_offs = offs;
  ds->shard_wsum = wsum;
  ds->shard_w_min = weighted ? wmin : 0.0;
  ds->shard_max_abs_x = (mx != mx) ? double(INFINITY) : mx;
  ds->shard_min_rows = mn;
  ds->shard_gen = ctx->comm_gen;
  return SR_OK;
}

// EXACT verdicts of the listed (BIG-only) trees over the GLOBAL rows of a row-sharded call: each rank
// folds the Julia leaf blocks it holds (sr_jsum_partials' ranges), the folds are all-gathered, and
// every rank adds them in Base.mapreduce_impl's recursion order.  Collective (the list is the same on
// every rank: it comes from the all-reduced flags); a local failure travels in the error word.
template <typename T>
int exact_sharded(sr_ctx* ctx, const EvalReq& req, const SrProgramBatch<T>& prog, const std::vector<int64_t>& list,
                  std::vector<uint8_t>* list_ok) {
  const sr_dataset* const ds = req.ds;
  list_ok->assign(list.size(), 1);
  int mc = 0;
  for (int64_t t : list) mc = std::max(mc, int(prog.n_checks[size_t(t)]));
  if (list.empty() || mc == 0) return SR_OK;
  const int nr = ctx->comm_ranks, me = ctx->comm_rank;
  const std::vector<int64_t>& offs = ds->shard_offs;
  const int64_t n_total = offs[size_t(nr)];
  if (nr == 1) return exact_list_ok<T>(ctx, req, prog, list, list_ok);  // one shard = the whole view
  std::vector<std::vector<JlRange>> ranges(static_cast<size_t>(nr));
  size_t max_r = 0;
  for (int r = 0; r < nr; ++r) {
    ranges[size_t(r)] = jl_ranges(offs[size_t(r)], offs[size_t(r) + 1] - offs[size_t(r)], n_total);
    max_r = std::max(max_r, ranges[size_t(r)].size());
  }
  const size_t n_arrays = list.size() * size_t(mc);
  // per rank: [n_arrays][its own range count] folds, then an error word (bytes of one double)
  const size_t payload = n_arrays * max_r * sizeof(T);
  const size_t slot = (payload + sizeof(double) + 255) & ~size_t(255);
  std::vector<char> mine(slot, 0);
  int local = run_exact<T>(ctx, req, prog, list.data(), int64_t(list.size()), mc, ranges[size_t(me)],
                           reinterpret_cast<T*>(mine.data()));
  if (local != SR_OK) std::fill(mine.begin(), mine.end(), 0);
  const double err = local != SR_OK ? 1.0 : 0.0;
  std::memcpy(mine.data() + payload, &err, sizeof(double));
  hipStream_t s = ctx->stream;
  Prep prep{ctx};
  prep.need(ctx->coll_buf, slot * size_t(nr + 1));
  int rc = agree_prep(ctx, prep);
  if (rc != SR_OK) return local != SR_OK ? local : rc;
  char* d = ctx->coll_buf.as<char>();
  if (hipMemcpyAsync(d, mine.data(), slot, hipMemcpyHostToDevice, s) != hipSuccess) {
    std::memset(mine.data() + payload, 0xff, sizeof(double));  // (poisoned error word)
    (void)hipMemcpy(d, mine.data(), slot, hipMemcpyHostToDevice);
  }
  rc = ctx->xport->allgather(d, d + slot, slot, s);
  if (rc != SR_OK) return rc;
  std::vector<char> every(slot * size_t(nr));
  // a copy failure here must not leave this rank out of the fold collectives its peers may enter next
  // (the fold list depends on these verdicts): the ranks agree on it first
  int post = SR_OK;
  if (hipMemcpyAsync(every.data(), d + slot, every.size(), hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    post = set_error(SR_ERR_HIP, "the exact-sum pass: copy of the gathered folds failed");
  if (ctx->inject_post_exact > 0) {  // tests
    --ctx->inject_post_exact;
    if (post == SR_OK) post = set_error(SR_ERR_HIP, "injected failure after the exact-sum all-gather");
  }
  rc = agree(ctx, post, "failed after the exact-sum all-gather");
  if (rc != SR_OK) return local != SR_OK ? local : rc;
  for (int r = 0; r < nr; ++r) {
    double e = 0.0;
    std::memcpy(&e, every.data() + slot * size_t(r) + payload, sizeof(double));
    if (e != 0.0) return local != SR_OK ? local : set_error(SR_ERR_HIP, "the exact-sum pass failed on rank " + std::to_string(r));
  }
  std::vector<const T*> rank_vals(static_cast<size_t>(nr));
  for (int r = 0; r < nr; ++r) rank_vals[size_t(r)] = reinterpret_cast<const T*>(every.data() + slot * size_t(r));
  std::vector<uint8_t> fin(n_arrays);
  jl_finite<T>(n_total, nr, offs.data(), rank_vals.data(), int64_t(n_arrays), fin.data());
  for (size_t i = 0; i < list.size(); ++i)
    for (int k = 0; k < mc; ++k) (*list_ok)[i] &= fin[i * size_t(mc) + size_t(k)];
  return SR_OK;
}

// One all-gather of `payload` bytes per rank plus an error word (every rank enters it, also after a
// local failure: its payload zeroed, its error word set); every[r] = rank r's payload.  Returns the
// local error, or an error when any rank's word is set.
int gather_checked(sr_ctx* ctx, const void* payload, size_t bytes, int local, std::vector<char>* every, size_t* slot_out,
                   const char* what, int* pending) {
  // a failure of this rank's copy of the gathered payloads is not returned here (its peers have theirs
  // and go on to the next collective): it goes to *pending, which the caller sends in the next
  // collective's error word (or agrees on after the last one)
  if (*pending != SR_OK && local == SR_OK) local = *pending;
  const int nr = ctx->comm_ranks;
  const size_t slot = (bytes + sizeof(double) + 255) & ~size_t(255);
  *slot_out = slot;
  std::vector<char> mine(slot, 0);
  if (local == SR_OK && bytes) std::memcpy(mine.data(), payload, bytes);
  const double err = local != SR_OK ? 1.0 : 0.0;
  std::memcpy(mine.data() + bytes, &err, sizeof(double));
  hipStream_t s = ctx->stream;
  char* d = ctx->coll_buf.as<char>();
  if (hipMemcpyAsync(d, mine.data(), slot, hipMemcpyHostToDevice, s) != hipSuccess) {
    std::memset(mine.data() + bytes, 0xff, sizeof(double));  // (poisoned error word)
    (void)hipMemcpy(d, mine.data(), slot, hipMemcpyHostToDevice);
  }
  int rc = ctx->xport->allgather(d, d + slot, slot, s);
  if (rc != SR_OK) return local != SR_OK ? local : rc;
  every->assign(slot * size_t(nr), 0);
  bool copied = hipMemcpyAsync(every->data(), d + slot, every->size(), hipMemcpyDeviceToHost, s) == hipSuccess;
  copied = hipStreamSynchronize(s) == hipSuccess && copied;
  if (local != SR_OK) return local;
  if (ctx->inject_post_gather > 0 && --ctx->inject_post_gather == 0) copied = false;  // tests: the k-th gather's copy
  if (!copied) {
    *pending = set_error(SR_ERR_HIP, std::string(what) + ": copy of the gathered payloads failed");
    return SR_OK;
  }
  for (int r = 0; r < nr; ++r) {
    double e = 0.0;
    std::memcpy(&e, every->data() + slot * size_t(r) + bytes, sizeof(double));
    if (e != 0.0) return set_error(SR_ERR_HIP, std::string(what) + " failed on rank " + std::to_string(r));
  }
  return SR_OK;
}

// The reference's loss fold of the listed trees over the GLOBAL rows, in row order.  Per batch of trees:
// every rank runs its shard's PRED pass and segment sums in parallel; one all-gather of the shards'
// f64 totals gives each rank the estimate of the fold's value at its first row, and every rank
// tabulates its segments' composed steps in parallel; then the chain runs rank after rank, each
// continuing from the previous shard's fold (one all-gather per rank; a rank's chain is O(1) per
// segment but for the segments where the fold crosses a binade).  Collective; out = the folds (T).
template <typename T>
int fold_sharded(sr_ctx* ctx, const EvalReq& req, const std::vector<int64_t>& list, std::vector<T>* out) {
  const sr_dataset* const ds = req.ds;
  out->assign(list.size(), T(0));
  if (list.empty()) return SR_OK;
  const int nr = ctx->comm_ranks, me = ctx->comm_rank;
  const std::vector<int64_t>& offs = ds->shard_offs;
  const int64_t n_total = offs[size_t(nr)];
  if (nr == 1) return fold_exact<T>(ctx, req, n_total, list, out);
  int64_t max_rows = 0;
  for (int r = 0; r < nr; ++r) max_rows = std::max(max_rows, offs[size_t(r) + 1] - offs[size_t(r)]);
  const int64_t per = fold_batch_trees(max_rows, sizeof(T), false);  // the same cut on every rank
  const size_t max_nb = std::min(list.size(), size_t(per));
  Prep prep{ctx};
  prep.need(ctx->coll_buf, ((max_nb * sizeof(double) + sizeof(double) + 255) & ~size_t(255)) * size_t(nr + 1));
  int rc = agree_prep(ctx, prep);
  if (rc != SR_OK) return rc;
  const int64_t seg_len = fold_seg_len(ctx, ds->n);
  const int64_t n_seg = seg_len > 0 ? (ds->n + seg_len - 1) / seg_len : 0;
  hipStream_t s = ctx->stream;
  std::vector<char> every;
  size_t slot = 0;
  int pending = SR_OK;  // a local failure after a gather: sent in the next one's error word
  for (size_t b0 = 0; b0 < list.size(); b0 += size_t(per)) {
    const size_t nb = std::min(list.size() - b0, size_t(per));
    // 1. this shard's predictions and segment sums; its per-tree total
    FoldDev<T> fd;
    int local = fold_prepare<T>(ctx, req, n_total, list.data() + b0, nb, seg_len, &fd);
    std::vector<double> tot(nb, 0.0);
    if (local == SR_OK && seg_len > 0) {
      std::vector<double> ss(nb * size_t(n_seg));
      if (hipMemcpyAsync(ss.data(), fd.segsum, ss.size() * sizeof(double), hipMemcpyDeviceToHost, s) != hipSuccess ||
          hipStreamSynchronize(s) != hipSuccess) {
        local = set_error(SR_ERR_HIP, "fold: segment sums copy failed");
      } else {
        for (size_t b = 0; b < nb; ++b)
          for (int64_t j = 0; j < n_seg; ++j) tot[b] += ss[b * size_t(n_seg) + size_t(j)];
      }
    }
    // 2. every shard's totals -> the f64 sum of the rows before this shard; the composed steps
    rc = gather_checked(ctx, tot.data(), nb * sizeof(double), local, &every, &slot, "the loss fold's shard totals",
                        &pending);
    if (rc != SR_OK) return rc;
    std::vector<double> est(nb, 0.0);
    for (int r = 0; r < me; ++r) {
      const double* v = reinterpret_cast<const double*>(every.data() + slot * size_t(r));
      for (size_t b = 0; b < nb; ++b) est[b] += v[b];
    }
    if (seg_len > 0 && hipMemcpyAsync(fd.carry_est, est.data(), nb * sizeof(double), hipMemcpyHostToDevice, s) != hipSuccess)
      local = set_error(SR_ERR_HIP, "fold: estimate upload failed");
    // 3. the chain, shard after shard
    std::vector<T> carry(nb, T(0)), vals(nb, T(0));
    for (int r = 0; r < nr; ++r) {
      if (me == r && local == SR_OK && pending == SR_OK) {
        if (r > 0 && hipMemcpyAsync(fd.carry, carry.data(), nb * sizeof(T), hipMemcpyHostToDevice, s) != hipSuccess)
          local = set_error(SR_ERR_HIP, "fold: carry upload failed");
        if (local == SR_OK) local = fold_finish<T>(ctx, req, nb, seg_len, fd, true, r > 0, vals.data());
      }
      rc = gather_checked(ctx, vals.data(), nb * sizeof(T), me == r ? local : SR_OK, &every, &slot, "the loss fold",
                          &pending);
      if (rc != SR_OK) return local != SR_OK ? local : rc;
      std::memcpy(carry.data(), every.data() + slot * size_t(r), nb * sizeof(T));
    }
    std::copy(carry.begin(), carry.end(), out->begin() + ptrdiff_t(b0));
  }
  release_large_pred(ctx);
  // a failure after the last gather: the ranks agree on it (the weights' sum gather may follow)
  return agree(ctx, pending, "failed in the loss fold");
}

// Every complete tree's in-order loss fold across the shards (sr_ctx::ref_fold; round 6).  The verdicts
// the ranks agreed on after the all-reduce and the exact pass choose the trees (the same bytes on every
// rank); one all-gather of the shards' per-tree f64 totals gives each rank the fold's estimated value at
// its first row; every rank's steps (stored-loss tables, or the plan and the FOLD pass) run in parallel;
// the walks run rank after rank, each from the previous shard's fold values (one all-gather per rank).
// folds / ok: the trees every walk took; *fallback: those some walk failed (the caller folds them
// through the prediction pass).  Collective (every rank enters every gather, also after a failure).
template <typename T>
int fold_all_sharded(sr_ctx* ctx, int64_t nt, const uint8_t* out_complete, const T* out_loss, std::vector<T>* folds,
                     std::vector<uint8_t>* ok, std::vector<int64_t>* fallback) {
  folds->assign(size_t(nt), T(0));
  ok->assign(size_t(nt), 0);
  std::shared_ptr<FoldJob<T>> job = std::static_pointer_cast<FoldJob<T>>(ctx->fold_job);
  ctx->fold_job.reset();
  if (!job || nt == 0) return SR_OK;  // (the ranks decide to fold or not alike: run_batch)
  const int nr = ctx->comm_ranks, me = ctx->comm_rank;
  hipStream_t s = ctx->stream;
  std::vector<uint8_t> elig(static_cast<size_t>(nt));
  bool any = false;
  for (int64_t t = 0; t < nt; ++t) {
    elig[size_t(t)] = ((out_complete[t] & 1) && !(out_complete[t] & SR_COMP_FOLD) && std::isfinite(double(out_loss[t]))) ? 1 : 0;
    any = any || elig[size_t(t)];
  }
  if (!any) return SR_OK;
  const size_t pay = size_t(nt) * (sizeof(T) + sizeof(int32_t));
  Prep prep{ctx};
  prep.need(ctx->coll_buf, ((std::max(size_t(nt) * sizeof(double), pay) + sizeof(double) + 255) & ~size_t(255)) * size_t(nr + 1));
  const size_t o_est = (size_t(nt) + 255) & ~size_t(255), o_car = o_est + ((size_t(nt) * 8 + 255) & ~size_t(255));
  prep.need(ctx->fold_io2, o_car + size_t(nt) * sizeof(T) + 64);
  int rc = agree_prep(ctx, prep);
  if (rc != SR_OK) return rc;
  int local = SR_OK, pending = SR_OK;
  auto hip_local = [&](hipError_t e, const char* what) {
    if (e != hipSuccess && local == SR_OK) local = set_error(SR_ERR_HIP, std::string("fold: ") + what + ": " + hipGetErrorString(e));
  };
  std::vector<double> tot(static_cast<size_t>(nt), 0.0);
  hip_local(hipMemcpyAsync(tot.data(), ctx->d_out_sum, size_t(nt) * sizeof(double), hipMemcpyDeviceToHost, s), "totals copy");
  hip_local(hipStreamSynchronize(s), "totals copy");
  std::vector<char> every;
  size_t slot = 0;
  rc = gather_checked(ctx, tot.data(), size_t(nt) * sizeof(double), local, &every, &slot, "the loss fold's shard totals",
                      &pending);
  if (rc != SR_OK) return rc;
  std::vector<double> est(static_cast<size_t>(nt), 0.0);
  for (int r = 0; r < me; ++r) {
    const double* v = reinterpret_cast<const double*>(every.data() + slot * size_t(r));
    for (int64_t t = 0; t < nt; ++t) est[size_t(t)] += v[t];
  }
  char* io = ctx->fold_io2.as<char>();
  uint8_t* d_elig = reinterpret_cast<uint8_t*>(io);
  double* d_est = reinterpret_cast<double*>(io + o_est);
  T* d_carry = reinterpret_cast<T*>(io + o_car);
  T* d_fval = reinterpret_cast<T*>(ctx->outs.as<char>() + ctx->outs_fval_off);
  int32_t* d_fst = reinterpret_cast<int32_t*>(ctx->outs.as<char>() + ctx->outs_fst_off);
  int step = SR_OK;  // (a failure from here on rides in the next gather's error word)
  auto hip_step = [&](hipError_t e, const char* what) {
    if (e != hipSuccess && step == SR_OK) step = set_error(SR_ERR_HIP, std::string("fold: ") + what + ": " + hipGetErrorString(e));
  };
  hip_step(hipMemcpyAsync(d_elig, elig.data(), size_t(nt), hipMemcpyHostToDevice, s), "verdicts upload");
  hip_step(hipMemcpyAsync(d_est, est.data(), size_t(nt) * sizeof(double), hipMemcpyHostToDevice, s), "estimates upload");
  const SrFoldWho who{ctx->d_out_sum, ctx->d_out_flag, job->n_terms, d_elig, d_est, me == 0 ? 1 : 0};
  if (step == SR_OK && pending == SR_OK)
    for (const FoldRegion<T>& fr : job->regions)
      if (step == SR_OK) step = fold_steps<T>(ctx, *job, fr, who, s);
  std::vector<T> carry(static_cast<size_t>(nt), T(0));
  std::vector<uint8_t> failed(static_cast<size_t>(nt), 0);
  std::vector<char> payload(pay, 0);
  for (int r = 0; r < nr; ++r) {
    if (me == r && step == SR_OK && pending == SR_OK) {
      if (r > 0) hip_step(hipMemcpyAsync(d_carry, carry.data(), size_t(nt) * sizeof(T), hipMemcpyHostToDevice, s), "carry upload");
      for (const FoldRegion<T>& fr : job->regions)
        if (step == SR_OK) step = fold_walk<T>(ctx, *job, fr, who, r > 0 ? d_carry : nullptr, d_fval, d_fst, s);
      hip_step(hipMemcpyAsync(payload.data(), d_fval, size_t(nt) * sizeof(T), hipMemcpyDeviceToHost, s), "walk copy");
      hip_step(hipMemcpyAsync(payload.data() + size_t(nt) * sizeof(T), d_fst, size_t(nt) * sizeof(int32_t),
                              hipMemcpyDeviceToHost, s), "walk copy");
      hip_step(hipStreamSynchronize(s), "walk");
    }
    rc = gather_checked(ctx, payload.data(), pay, me == r ? step : SR_OK, &every, &slot, "the loss fold's walk", &pending);
    if (rc != SR_OK) return rc;
    const char* got = every.data() + slot * size_t(r);
    std::memcpy(carry.data(), got, size_t(nt) * sizeof(T));
    const int32_t* st = reinterpret_cast<const int32_t*>(got + size_t(nt) * sizeof(T));
    for (int64_t t = 0; t < nt; ++t)
      if (elig[size_t(t)] && st[t] != SR_FST_OK) failed[size_t(t)] = 1;
  }
  for (int64_t t = 0; t < nt; ++t) {
    if (!elig[size_t(t)]) continue;
    if (failed[size_t(t)]) {
      fallback->push_back(t);
    } else {
      (*folds)[size_t(t)] = carry[size_t(t)];
      (*ok)[size_t(t)] = 1;
    }
  }
  return agree(ctx, pending, "failed in the loss fold");
}

// Base.sum(w) in T over the GLOBAL rows of a row-sharded dataset: each shard folds its Julia leaf
// blocks (one-row heads continue a block begun on an earlier shard), one all-gather, and every rank
// combines them in Base.mapreduce_impl's recursion order.  Collective.
template <typename T>
int jl_wsum_sharded(sr_ctx* ctx, const sr_dataset* ds, T* out) {
  const int nr = ctx->comm_ranks, me = ctx->comm_rank;
  const std::vector<int64_t>& offs = ds->shard_offs;
  const int64_t n_total = offs[size_t(nr)];
  std::vector<std::vector<JlRange>> ranges(static_cast<size_t>(nr));
  size_t max_r = 0;
  for (int r = 0; r < nr; ++r) {
    ranges[size_t(r)] = jl_ranges(offs[size_t(r)], offs[size_t(r) + 1] - offs[size_t(r)], n_total);
    max_r = std::max(max_r, ranges[size_t(r)].size());
  }
  std::vector<T> mine(max_r, T(0));
  for (size_t i = 0; i < ranges[size_t(me)].size(); ++i) {
    const JlRange& g = ranges[size_t(me)][i];
    T a = T(ds->w_host[size_t(g.lo)]);
    for (int64_t k = g.lo + 1; k <= g.hi; ++k) a = a + T(ds->w_host[size_t(k)]);
    mine[i] = a;
  }
  Prep prep{ctx};
  prep.need(ctx->coll_buf, ((max_r * sizeof(T) + sizeof(double) + 255) & ~size_t(255)) * size_t(nr + 1));
  int rc = agree_prep(ctx, prep);
  if (rc != SR_OK) return rc;
  std::vector<char> every;
  size_t slot = 0;
  int pending = SR_OK;
  rc = gather_checked(ctx, mine.data(), max_r * sizeof(T), SR_OK, &every, &slot, "the weights' sum", &pending);
  if (rc != SR_OK) return rc;
  if (ctx->inject_post_wsum > 0 && --ctx->inject_post_wsum == 0 && pending == SR_OK)  // (tests)
    pending = set_error(SR_ERR_HIP, "injected failure after the weights' sum gather");
  // a local failure after the gather (this rank's copy of it): every rank learns of it and fails
  // together, as after the fold's gathers (a lone failing rank left its peers to enter the
  // next step's all-reduce without it)
  rc = agree(ctx, pending, "failed in the weights' sum");
  if (rc != SR_OK) return rc;
  std::vector<const T*> rank_vals(static_cast<size_t>(nr));
  for (int r = 0; r < nr; ++r) rank_vals[size_t(r)] = reinterpret_cast<const T*>(every.data() + slot * size_t(r));
  std::vector<T> leafval(jl_leaves(n_total).size());
  for (int r = 0; r < nr; ++r) {
    const std::vector<JlRange>& rg = ranges[size_t(r)];
    for (size_t i = 0; i < rg.size(); ++i) {
      T& dst = leafval[size_t(rg[i].leaf)];
      dst = rg[i].head ? T(dst + rank_vals[size_t(r)][i]) : rank_vals[size_t(r)][i];
    }
  }
  size_t idx = 0;
  *out = n_total > 0 ? jl_reduce<T>(leafval, 0, n_total - 1, &idx) : T(0);
  return SR_OK;
}

// The row-sharded step (sr_eval_loss_sharded): this rank's shard through the same launch pipeline as
// a single-GPU call (derived columns, dead-tree probe, two-chunk compile/launch overlap), the packed
// [5, n_trees] partials plus an error word summed by ONE in-place all-reduce on the device, losses
// finalized on the device (Σ / global denominator), the rare BIG-only trees decided by the exact pass
// over the global rows, and the rarer trees whose loss fold the bounds cannot decide folded in row
// order across the shards.  Every rank enters every collective, also after a local failure (its
// partials zeroed, its error word set), and then every rank returns an error.
template <typename T>
int eval_sharded_impl(sr_ctx* ctx, const EvalReq& req, T* out_loss, uint8_t* out_complete) {
  const sr_dataset* const ds = req.ds;
  const int64_t nt = req.trees->n_trees;
  const int nr = ctx->comm_ranks;
  const size_t n5 = size_t(5) * size_t(nt);
  // [5][nt] partials | error word, then the finalized losses (T) and complete codes
  const size_t o_loss = ((n5 + 1) * sizeof(double) + 255) & ~size_t(255);
  const size_t o_comp = o_loss + ((size_t(nt) * sizeof(T) + 255) & ~size_t(255));
  // 1. every buffer this call's collectives use, grown (and agreed on) before the first of them
  const bool need_layout = !(ds->shard_gen == ctx->comm_gen && !ds->shard_offs.empty());
  Prep prep{ctx};
  if (need_layout) prep.need(ctx->coll_buf, sizeof(double) * kLayoutWords * size_t(nr + 1));
  prep.need(ctx->coll_packed, o_comp + size_t(nt) + 16);
  int rc = agree_prep(ctx, prep);
  if (rc != SR_OK) return rc;
  // 2. the shards' layout (first call per dataset and communicator)
  if (need_layout) {
    rc = shard_layout(ctx, ds);
    if (rc != SR_OK) return rc;
  }
  const int64_t n_total = ds->shard_offs[size_t(nr)];
  const ShardCtl sc{ds->shard_max_abs_x, ds->shard_min_rows};
  auto t0 = std::chrono::steady_clock::now();
  ctx->start_phases(t0);
  // 3. this shard
  SrProgramBatch<T> prog;
  BatchWants want;
  want.n_total = n_total;
  want.allow_derived = true;
  want.shard = &sc;
  want.fold = true;  // (the in-order fold's steps and walks follow the ranks' agreement, step 6)
  BatchResult res;
  int local = nt > 0 ? run_batch<T>(ctx, req, want, &prog, &res) : SR_OK;
  hipStream_t s = ctx->stream;
  char* base = ctx->coll_packed.as<char>();
  double* dst = reinterpret_cast<double*>(base);
  if (local == SR_OK && nt > 0) {
    const hipError_t e = sr_launch_pack_partials(ctx->d_out_sum, ctx->d_out_flag, int(nt), dst, s);
    if (e != hipSuccess) local = set_error(SR_ERR_HIP, std::string("pack partials: ") + hipGetErrorString(e));
  }
  double err_word = local != SR_OK ? 1.0 : 0.0;
  if (local != SR_OK && hipMemsetAsync(dst, 0, n5 * sizeof(double), s) != hipSuccess) err_word = NAN;
  if (hipMemcpyAsync(dst + n5, &err_word, sizeof(double), hipMemcpyHostToDevice, s) != hipSuccess && local == SR_OK)
    local = set_error(SR_ERR_HIP, "error word upload failed");
  ctx->mark_phase(1);
  // 4. the path's one exchange step: every rank's partials (and error words), summed in place
  rc = ctx->xport->allreduce_sum(dst, n5 + 1, s);
  if (rc != SR_OK) return local != SR_OK ? local : rc;
  const double denom = ds->w ? ds->shard_wsum : double(n_total);
  T* d_loss = reinterpret_cast<T*>(base + o_loss);
  uint8_t* d_comp = reinterpret_cast<uint8_t*>(base + o_comp);
  double err_sum = 0.0;
  // After the all-reduce a local HIP failure must not return on this rank alone: its peers would
  // enter the exact / fold collectives below without it.  The failure rides in `post`, and the ranks
  // agree on it (one Σ of error words) before any further collective.
  int post = SR_OK;
  auto hip_post = [&](hipError_t e, const char* what) {
    if (e != hipSuccess && post == SR_OK) post = set_error(SR_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
  };
  hip_post(hipMemcpyAsync(&err_sum, dst + n5, sizeof(double), hipMemcpyDeviceToHost, s), "error sum copy");
  const int64_t n_terms = (ds->w && ds->shard_w_min < 0.0) ? 0 : n_total;
  if (post == SR_OK) hip_post(sr_launch_finalize_packed<T>(dst, int(nt), denom, n_terms, d_loss, d_comp, s), "finalize");
  if (nt > 0 && post == SR_OK) {
    hip_post(hipMemcpyAsync(out_loss, d_loss, size_t(nt) * sizeof(T), hipMemcpyDeviceToHost, s), "loss copy");
    hip_post(hipMemcpyAsync(out_complete, d_comp, size_t(nt), hipMemcpyDeviceToHost, s), "flag copy");
  }
  hip_post(hipStreamSynchronize(s), "stream synchronize");
  if (ctx->inject_post > 0) {  // tests: a local failure between the all-reduce and the exact / fold passes
    --ctx->inject_post;
    if (post == SR_OK) post = set_error(SR_ERR_HIP, "injected failure after the all-reduce");
  }
  ctx->timing_pending = local == SR_OK && post == SR_OK && nt > 0;
  if (!ctx->timing_pending) ctx->last_eval_ms = ctx->last_busy_ms = 0.0;
  ctx->mark_phase(2);
  if (nr > 1) {
    rc = agree(ctx, local != SR_OK ? local : post, "failed after the all-reduce");
    if (rc != SR_OK) return local != SR_OK ? local : rc;
  } else if (post != SR_OK) {
    return local != SR_OK ? local : post;
  }
  if (err_sum != 0.0) return local != SR_OK ? local : set_error(SR_ERR_HIP, "the row-sharded step failed on a peer rank");
  // 5. rare: BIG-only trees, DynamicExpressions' exact check over the global rows
  std::vector<int64_t> list;
  for (int64_t t = 0; t < nt; ++t)
    if (out_complete[t] & 2) list.push_back(t);
  std::vector<uint8_t> list_ok;
  ctx->n_exact_last = int64_t(list.size());
  ctx->exact_kernel_ms = 0.0;
  rc = exact_sharded<T>(ctx, req, prog, list, &list_ok);
  if (rc != SR_OK) return rc;
  for (size_t i = 0; i < list.size(); ++i) {
    const int64_t t = list[i];
    out_complete[t] = uint8_t((out_complete[t] & ~3) | (list_ok[i] ? 1 : 0));
    if (!list_ok[i]) out_loss[t] = T(INFINITY);
  }
  ctx->mark_phase(3);
  // 6. every complete tree's in-order fold across the shards (sr_ctx::ref_fold), and — rarer — the trees
  //    whose fold the overflow band or a failed walk leaves to the prediction pass (sr_fold.h)
  std::vector<int64_t> fold_list;
  std::vector<T> rfold;
  std::vector<uint8_t> rok;
  rc = fold_all_sharded<T>(ctx, nt, out_complete, out_loss, &rfold, &rok, &fold_list);
  if (rc != SR_OK) return rc;
  ctx->n_ref_fail_last = int64_t(fold_list.size());
  ctx->n_ref_ok_last = 0;
  for (uint8_t v : rok) ctx->n_ref_ok_last += v;
  for (int64_t t = 0; t < nt; ++t)
    if ((out_complete[t] & 1) && (out_complete[t] & SR_COMP_FOLD)) fold_list.push_back(t);
  std::sort(fold_list.begin(), fold_list.end());
  ctx->n_fold_last = int64_t(fold_list.size());
  ctx->fold_slow_last = ctx->fold_seg_last = 0;
  for (double& v : ctx->fold_ms) v = 0.0;
  std::vector<T> fold;
  rc = fold_sharded<T>(ctx, req, fold_list, &fold);
  if (rc != SR_OK) return rc;
  // mean: total / count, in T; weighted: total / sum(w), the reference's pairwise Base.sum in T
  T fden = T(denom);
  if (ds->w && (!fold_list.empty() || ctx->n_ref_ok_last > 0)) {  // (the same on every rank)
    rc = nr > 1 ? jl_wsum_sharded<T>(ctx, ds, &fden) : (fden = jl_wsum_view<T>(ds, nullptr, ds->n), SR_OK);
    if (rc != SR_OK) return rc;
  }
  for (size_t i = 0; i < fold_list.size(); ++i) out_loss[fold_list[i]] = T(fold[i] / fden);
  for (int64_t t = 0; t < nt; ++t)
    if (rok[size_t(t)]) out_loss[t] = T(rfold[size_t(t)] / fden);
  for (int64_t t = 0; t < nt; ++t) out_complete[t] &= 1;
  ctx->mark_phase(4);
  ctx->last_total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return SR_OK;
}

// Owner rank of every tree for tree sharding: sorted by node count (largest first, stable), dealt in
// snake order 0..N-1, N-1..0, ... (sr_amd.distributed.tree_owners is the same rule).
std::vector<int> tree_owners(const sr_tree_batch* trees, int nr) {
  const int64_t nt = trees->n_trees;
  std::vector<int64_t> order(static_cast<size_t>(nt));
  for (int64_t t = 0; t < nt; ++t) order[size_t(t)] = t;
  auto size_of = [&](int64_t t) { return trees->offsets[t + 1] - trees->offsets[t]; };
  std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return size_of(a) > size_of(b); });
  std::vector<int> owner(static_cast<size_t>(nt));
  for (int64_t k = 0; k < nt; ++k) {
    const int64_t round = k / nr, pos = k % nr;
    owner[size_t(order[size_t(k)])] = int((round & 1) ? (nr - 1 - pos) : pos);
  }
  return owner;
}

// Tree-sharded scoring (sr_eval_loss_tree_sharded): the dataset is replicated, the trees are split over
// the ranks by estimated cost (tree_owners), each rank scores its own trees with the single-GPU call,
// and ONE all-gather of every rank's results ([loss (T) | complete] of its trees, in tree order, and
// an error word) hands every rank every result.
template <typename T>
int eval_tree_sharded_impl(sr_ctx* ctx, const EvalReq& req, T* out_loss, uint8_t* out_complete) {
  const sr_tree_batch* const trees = req.trees;
  const int64_t nt = trees->n_trees;
  const int nr = ctx->comm_ranks, me = ctx->comm_rank;
  const std::vector<int> owner = nr > 1 ? tree_owners(trees, nr) : std::vector<int>(size_t(nt), 0);
  std::vector<std::vector<int64_t>> of(static_cast<size_t>(nr));
  for (int64_t t = 0; t < nt; ++t) of[size_t(owner[size_t(t)])].push_back(t);
  size_t max_cnt = 0;
  for (const auto& v : of) max_cnt = std::max(max_cnt, v.size());
  const size_t o_comp = max_cnt * sizeof(T);
  const size_t o_err = (o_comp + max_cnt + 7) & ~size_t(7);
  const size_t slot = (o_err + sizeof(double) + 255) & ~size_t(255);
  Prep prep{ctx};
  prep.need(ctx->h_coll, slot * size_t(nr + 1));
  prep.need(ctx->coll_buf, slot * size_t(nr + 1));
  int rc = agree_prep(ctx, prep);
  if (rc != SR_OK) return rc;
  const std::vector<int64_t>& mine = of[size_t(me)];
  char* hm = ctx->h_coll.as<char>();  // pinned: this rank's slot, then every rank's
  std::memset(hm, 0, slot);
  int local = SR_OK;
  if (!mine.empty()) {
    T* l = reinterpret_cast<T*>(hm);
    uint8_t* c = reinterpret_cast<uint8_t*>(hm + o_comp);
    if (nr == 1) {  // (one rank owns every tree, in order: no sub-batch)
      local = eval_loss_impl<T>(ctx, req, l, c);
    } else {
      SubBatch<T> sub(*trees, mine.data(), mine.size());
      EvalReq mreq = req;
      mreq.trees = &sub.b;
      local = eval_loss_impl<T>(ctx, mreq, l, c);
    }
  }
  const double err = local != SR_OK ? 1.0 : 0.0;
  if (local != SR_OK) std::memset(hm, 0, slot);
  std::memcpy(hm + o_err, &err, sizeof(double));
  hipStream_t s = ctx->stream;
  char* d = ctx->coll_buf.as<char>();
  if (hipMemcpyAsync(d, hm, slot, hipMemcpyHostToDevice, s) != hipSuccess) {
    std::memset(hm + o_err, 0xff, sizeof(double));
    (void)hipMemcpy(d, hm, slot, hipMemcpyHostToDevice);
  }
  rc = ctx->xport->allgather(d, d + slot, slot, s);
  if (rc != SR_OK) return local != SR_OK ? local : rc;
  char* every = hm + slot;
  SR_HIP_CHECK(hipMemcpyAsync(every, d + slot, slot * size_t(nr), hipMemcpyDeviceToHost, s));
  SR_HIP_CHECK(hipStreamSynchronize(s));
  for (int r = 0; r < nr; ++r) {
    double e = 0.0;
    std::memcpy(&e, every + slot * size_t(r) + o_err, sizeof(double));
    if (e != 0.0) return local != SR_OK ? local : set_error(SR_ERR_HIP, "tree-sharded scoring failed on rank " + std::to_string(r));
  }
  for (int r = 0; r < nr; ++r) {
    const T* l = reinterpret_cast<const T*>(every + slot * size_t(r));
    const uint8_t* c = reinterpret_cast<const uint8_t*>(every + slot * size_t(r) + o_comp);
    const std::vector<int64_t>& v = of[size_t(r)];
    for (size_t i = 0; i < v.size(); ++i) {
      out_loss[v[i]] = l[i];
      out_complete[v[i]] = c[i] ? 1 : 0;
    }
  }
  return SR_OK;
}

// Every event of the context, stated once: f(event, timed) — sr_init creates them (timed: the event records
// times; the others only order streams), destroy_ctx destroys them.
template <typename F>
void for_each_event(sr_ctx* ctx, F f) {
  f(ctx->ev_join, false);
  f(ctx->ev_flags, false);
  for (hipEvent_t& ev : ctx->ev_red) f(ev, false);
  for (hipEvent_t* ev : {&ctx->ev_start, &ctx->ev_k0, &ctx->ev_k1, &ctx->ev_end, &ctx->ev_d0, &ctx->ev_d1}) f(*ev, true);
  for (int c = 0; c < kMaxChunks; ++c)
    for (hipEvent_t* ev : {&ctx->ev_c0[c], &ctx->ev_c1[c], &ctx->ev_fc0[c], &ctx->ev_fc1[c]}) f(*ev, true);
  for (int b = 0; b < sr_ctx::kGradBuckets; ++b)
    for (hipEvent_t* ev : {&ctx->ev_g0[b], &ctx->ev_g1[b]}) f(*ev, true);
  for (hipEvent_t& ev : ctx->ev_f) f(ev, true);
}

// The context's end (sr_shutdown, and sr_init when it fails part-way: what was never created is null and
// skipped).  In the order the device sees: synchronise the streams, drop the transport, destroy the events
// and streams, free the buffers — the DevBuf / HostBuf members free themselves in `delete`.
void destroy_ctx(sr_ctx* ctx) {
  {
    Lock l(ctx);
    (void)hipSetDevice(ctx->device);
    for (hipStream_t s : {ctx->stream, ctx->stream2, ctx->stream3})
      if (s) (void)hipStreamSynchronize(s);
    ctx->xport.reset();
    for_each_event(ctx, [](hipEvent_t& ev, bool) {
      if (ev) (void)hipEventDestroy(ev);
      ev = nullptr;
    });
    for (hipStream_t* s : {&ctx->stream3, &ctx->stream2, &ctx->stream}) {
      if (*s) (void)hipStreamDestroy(*s);
      *s = nullptr;
    }
    // (debug_hint_regrow: the hint array may live inside its reservation, which is freed once)
    if (ctx->hint.p == ctx->hint_reserve) {
      ctx->hint.p = nullptr;
      ctx->hint.cap = 0;
    }
    if (ctx->hint_reserve) (void)hipFree(ctx->hint_reserve);
    ctx->hint_reserve = nullptr;
    for (sr_ctx::LossExpr& e : ctx->loss_exprs) {
      if (e.dev) (void)hipFree(e.dev);
      e.dev = nullptr;
    }
  }
  delete ctx;
}

}  // namespace

// ====================================================================== C ABI
extern "C" {

const char* sr_last_error(void) { return g_last_error.c_str(); }
int sr_version(void) { return SR_AMD_VERSION; }

int sr_device_count(int* count) {
  if (!count) return set_error(SR_ERR_INVALID_ARG, "NULL count");
  int c = 0;
  hipError_t e = hipGetDeviceCount(&c);
  if (e != hipSuccess) {
    *count = 0;
    return set_error(SR_ERR_NO_DEVICE, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
  }
  *count = c;
  return SR_OK;
}

int sr_init(int device, sr_ctx** out) {
  if (!out) return set_error(SR_ERR_INVALID_ARG, "NULL output");
  *out = nullptr;
  int c = 0;
  if (hipGetDeviceCount(&c) != hipSuccess || c <= 0) return set_error(SR_ERR_NO_DEVICE, "no HIP device visible");
  if (device < 0 || device >= c) return set_error(SR_ERR_INVALID_ARG, "device index out of range");
  SR_HIP_CHECK(hipSetDevice(device));
  auto* ctx = new sr_ctx();
  ctx->device = device;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess) ctx->cu_count = prop.multiProcessorCount;
  sr_knobs_from_env(*ctx, [](const char* name) -> const char* { return std::getenv(name); });
  hipError_t e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
  for_each_event(ctx, [&e](hipEvent_t& ev, bool timed) {
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ev, timed ? hipEventDefault : hipEventDisableTiming);
  });
  if (e != hipSuccess) {
    destroy_ctx(ctx);
    return set_error(SR_ERR_HIP, std::string("stream/event creation: ") + hipGetErrorString(e));
  }
  *out = ctx;
  return SR_OK;
}

int sr_shutdown(sr_ctx* ctx) {
  if (ctx) destroy_ctx(ctx);
  return SR_OK;
}

int sr_register_opset(sr_ctx* ctx, int n_unary, const char* const* unary_names, int n_binary,
                      const char* const* binary_names, int* opset_id) {
  if (check_ctx(ctx) != SR_OK) return SR_ERR_INVALID_ARG;
  if (!opset_id || n_unary < 0 || n_binary < 0 || (n_unary > 0 && !unary_names) || (n_binary > 0 && !binary_names))
    return set_error(SR_ERR_INVALID_ARG, "bad operator name arrays");
  if (n_unary > 255 || n_binary > 255) return set_error(SR_ERR_INVALID_ARG, "more than 255 operators of one degree");
  SrOpset o;
  for (int i = 0; i < n_unary; ++i) {
    const uint32_t id = unary_names[i] ? sr_unary_id(unary_names[i]) : 0;
    if (!id) return set_error(SR_ERR_UNSUPPORTED_OP, std::string("unsupported unary operator: ") +
                                                         (unary_names[i] ? unary_names[i] : "(null)"));
    o.unary.push_back(id);
  }
  for (int i = 0; i < n_binary; ++i) {
    const uint32_t id = binary_names[i] ? sr_binary_id(binary_names[i]) : 0;
    if (!id) return set_error(SR_ERR_UNSUPPORTED_OP, std::string("unsupported binary operator: ") +
                                                         (binary_names[i] ? binary_names[i] : "(null)"));
    o.binary.push_back(id);
  }
  Lock l(ctx);
  ctx->opsets.push_back(o);
  ctx->tiers.push_back(tier_of(o));
  *opset_id = int(ctx->opsets.size()) - 1;
  return SR_OK;
}

extern "C++" {
namespace {
// The parameter's domain per loss: delta (Huber), eps (both EpsilonIns), circ (Periodic), gamma (SmoothedL1Hinge),
// q (DWDMargin) and P (LPDist) positive; tau (Quantile) unbounded.  LossFunctions' constructors assert these, as
// far as memory of a package that is not vendored goes; circ and gamma are divisors in sr_elem_loss, so 0 is
// refused whatever the package does.
bool loss_param_in_domain(int kind, double param) {
  switch (kind) {
    case SR_LOSS_LP: case SR_LOSS_HUBER: case SR_LOSS_L1_EPS_INS: case SR_LOSS_L2_EPS_INS: case SR_LOSS_PERIODIC:
    case SR_LOSS_SMOOTH_L1_HINGE: case SR_LOSS_DWD_MARGIN:
      return param > 0.0;
    default: return true;
  }
}
}  // namespace
}

int sr_register_loss(sr_ctx* ctx, int kind, double param, int* loss_code) {
  if (check_ctx(ctx) != SR_OK) return SR_ERR_INVALID_ARG;
  if (!loss_code || kind < 0 || kind >= SR_LOSS_COUNT) return set_error(SR_ERR_INVALID_ARG, "unknown loss kind");
  if (!std::isfinite(param)) return set_error(SR_ERR_INVALID_ARG, "loss parameter must be finite");
  if (!loss_param_in_domain(kind, param))
    return set_error(SR_ERR_INVALID_ARG, "loss parameter outside the loss's domain (delta, eps, circ, gamma, q, P must be positive)");
  Lock l(ctx);
  for (size_t i = 0; i < ctx->losses.size(); ++i)
    if (ctx->losses[i].first == kind && ctx->losses[i].second == param) {
      *loss_code = kLossCodeBase + int(i);
      return SR_OK;
    }
  ctx->losses.emplace_back(kind, param);
  *loss_code = kLossCodeBase + int(ctx->losses.size()) - 1;
  return SR_OK;
}

extern "C++" {
namespace {
// The operator ids of a loss expression's name lists and its one tree's bounds, checked; *key: the
// registration's bytes (names, node fields, constants).
int loss_expr_inputs(int n_unary, const char* const* unary_names, int n_binary, const char* const* binary_names,
                     const sr_tree_batch* tree, SrOpset* ops, int64_t* b0, int64_t* n_nodes, std::string* key) {
  if (n_unary < 0 || n_binary < 0 || n_unary > 255 || n_binary > 255 || (n_unary > 0 && !unary_names) ||
      (n_binary > 0 && !binary_names))
    return set_error(SR_ERR_INVALID_ARG, "bad operator name arrays");
  for (int i = 0; i < n_unary; ++i) {
    const uint32_t id = unary_names[i] ? sr_unary_id(unary_names[i]) : 0;
    if (!id) return set_error(SR_ERR_UNSUPPORTED_OP, std::string("loss expression: unsupported unary operator: ") +
                                                         (unary_names[i] ? unary_names[i] : "(null)"));
    ops->unary.push_back(id);
    if (key) key->append(unary_names[i]).push_back('\0');
  }
  if (key) key->push_back('|');
  for (int i = 0; i < n_binary; ++i) {
    const uint32_t id = binary_names[i] ? sr_binary_id(binary_names[i]) : 0;
    if (!id) return set_error(SR_ERR_UNSUPPORTED_OP, std::string("loss expression: unsupported binary operator: ") +
                                                         (binary_names[i] ? binary_names[i] : "(null)"));
    ops->binary.push_back(id);
    if (key) key->append(binary_names[i]).push_back('\0');
  }
  if (!tree || tree->n_trees != 1 || !tree->offsets)
    return set_error(SR_ERR_INVALID_ARG, "a loss expression is a sr_tree_batch of exactly one tree");
  if (!tree->degree || !tree->op || !tree->feature || !tree->constant || !tree->val)
    return set_error(SR_ERR_INVALID_ARG, "sr_tree_batch has NULL arrays");
  *b0 = tree->offsets[0];
  *n_nodes = tree->offsets[1] - tree->offsets[0];
  if (*b0 < 0 || *n_nodes < 1) return set_error(SR_ERR_INVALID_ARG, "loss expression: empty tree");
  if (*n_nodes > SR_LX_MAX_NODES)
    return set_error(SR_ERR_INVALID_ARG, "loss expression: " + std::to_string(*n_nodes) + " nodes; the limit is " +
                                             std::to_string(SR_LX_MAX_NODES));
  if (key) {
    const size_t n = size_t(*n_nodes);
    key->push_back('|');
    key->append(reinterpret_cast<const char*>(tree->degree + *b0), n);
    key->append(reinterpret_cast<const char*>(tree->op + *b0), n);
    key->append(reinterpret_cast<const char*>(tree->constant + *b0), n);
    key->append(reinterpret_cast<const char*>(tree->feature + *b0), n * sizeof(uint16_t));
    key->append(reinterpret_cast<const char*>(static_cast<const double*>(tree->val) + *b0), n * sizeof(double));
  }
  return SR_OK;
}
template <typename T>
int loss_expr_compile(const SrOpset& ops, const sr_tree_batch* tree, int64_t b0, int64_t n_nodes, SrLossProg<T>* out) {
  std::string err;
  if (sr_lx_compile<T>(ops.unary.data(), int(ops.unary.size()), ops.binary.data(), int(ops.binary.size()), tree->degree + b0,
                       tree->op + b0, tree->feature + b0, tree->constant + b0, static_cast<const double*>(tree->val) + b0,
                       n_nodes, out, &err) != 0)
    return set_error(SR_ERR_INVALID_ARG, err);
  return SR_OK;
}
}  // namespace
}  // extern "C++"

int sr_register_loss_expr(sr_ctx* ctx, int n_unary, const char* const* unary_names, int n_binary,
                          const char* const* binary_names, const sr_tree_batch* tree, int* loss_code) {
  if (check_ctx(ctx) != SR_OK) return SR_ERR_INVALID_ARG;
  if (!loss_code) return set_error(SR_ERR_INVALID_ARG, "NULL loss_code");
  SrOpset ops;
  int64_t b0 = 0, n_nodes = 0;
  std::string key;
  int rc = loss_expr_inputs(n_unary, unary_names, n_binary, binary_names, tree, &ops, &b0, &n_nodes, &key);
  if (rc != SR_OK) return rc;
  Lock l(ctx);
  for (size_t i = 0; i < ctx->loss_exprs.size(); ++i)
    if (ctx->loss_exprs[i].key == key) {
      *loss_code = kLossExprBase + int(i);
      return SR_OK;
    }
  sr_ctx::LossExpr e;
  if ((rc = loss_expr_compile<float>(ops, tree, b0, n_nodes, &e.p32)) != SR_OK) return rc;
  if ((rc = loss_expr_compile<double>(ops, tree, b0, n_nodes, &e.p64)) != SR_OK) return rc;
  e.key = std::move(key);
  SR_HIP_CHECK(hipSetDevice(ctx->device));
  void* dev = nullptr;
  SR_HIP_CHECK(hipMalloc(&dev, sizeof(e.p32.ins) + sizeof(e.p64.ins)));
  hipError_t he = hipMemcpy(dev, e.p32.ins, sizeof(e.p32.ins), hipMemcpyHostToDevice);
  if (he == hipSuccess)
    he = hipMemcpy(static_cast<char*>(dev) + sizeof(e.p32.ins), e.p64.ins, sizeof(e.p64.ins), hipMemcpyHostToDevice);
  if (he != hipSuccess) {
    (void)hipFree(dev);
    return set_error(SR_ERR_HIP, std::string("loss program upload: ") + hipGetErrorString(he));
  }
  e.dev = dev;
  ctx->loss_exprs.push_back(std::move(e));
  *loss_code = kLossExprBase + int(ctx->loss_exprs.size()) - 1;
  return SR_OK;
}

int sr_loss_expr_host(int dtype, int n_unary, const char* const* unary_names, int n_binary,
                      const char* const* binary_names, const sr_tree_batch* tree, int64_t n, const void* pred,
                      const void* y, const void* w, void* out_value, void* out_dvalue) {
  if (dtype != SR_DTYPE_F32 && dtype != SR_DTYPE_F64) return set_error(SR_ERR_INVALID_ARG, "unknown dtype");
  if (n < 0 || (n > 0 && (!pred || !y || !out_value))) return set_error(SR_ERR_INVALID_ARG, "NULL value arrays");
  SrOpset ops;
  int64_t b0 = 0, n_nodes = 0;
  int rc = loss_expr_inputs(n_unary, unary_names, n_binary, binary_names, tree, &ops, &b0, &n_nodes, nullptr);
  if (rc != SR_OK) return rc;
  auto run = [&](auto tag) -> int {
    using T = decltype(tag);
    SrLossProg<T> prog;
    const int r = loss_expr_compile<T>(ops, tree, b0, n_nodes, &prog);
    if (r != SR_OK) return r;
    if (prog.uses_w && !w) return set_error(SR_ERR_INVALID_ARG, "the loss expression references the weight, but w is NULL");
    if (!prog.uses_w && w)
      return set_error(SR_ERR_INVALID_ARG, "weights given, but the loss expression takes (prediction, target) only");
    sr_lx_host_eval<T>(prog, n, static_cast<const T*>(pred), static_cast<const T*>(y), static_cast<const T*>(w),
                       static_cast<T*>(out_value), static_cast<T*>(out_dvalue));
    return SR_OK;
  };
  return dtype == SR_DTYPE_F32 ? run(float{}) : run(double{});
}

int sr_dataset_upload(sr_ctx* ctx, int dtype, const void* X, int64_t nfeatures, int64_t n, const void* y,
                      const void* weights, sr_dataset** out) {
  if (check_ctx(ctx) != SR_OK) return SR_ERR_INVALID_ARG;
  if (!out || !X || nfeatures <= 0 || n <= 0) return set_error(SR_ERR_INVALID_ARG, "bad dataset arguments");
  if (nfeatures > 65535) return set_error(SR_ERR_INVALID_ARG, "nfeatures exceeds Node.feature (UInt16)");
  Lock l(ctx);
  SR_HIP_CHECK(hipSetDevice(ctx->device));
  if (dtype == SR_DTYPE_F32) return upload_impl<float>(ctx, X, nfeatures, n, y, weights, out);
  if (dtype == SR_DTYPE_F64) return upload_impl<double>(ctx, X, nfeatures, n, y, weights, out);
  return set_error(SR_ERR_INVALID_ARG, "unknown dtype");
}

int sr_dataset_upload_classes(sr_ctx* ctx, int dtype, const void* X, int64_t nfeatures, int64_t n, const void* y,
                              const void* weights, const int32_t* cls, int32_t n_classes, sr_dataset** out) {
  if (check_ctx(ctx) != SR_OK) return SR_ERR_INVALID_ARG;
  if (!out || !X || nfeatures <= 0 || n <= 0) return set_error(SR_ERR_INVALID_ARG, "bad dataset arguments");
  if (nfeatures > 65534) return set_error(SR_ERR_INVALID_ARG, "nfeatures (with the class row) exceeds Node.feature (UInt16)");
  if (!cls || n_classes < 1 || n_classes >= (1 << 24)) return set_error(SR_ERR_INVALID_ARG, "bad class column");
  for (int64_t i = 0; i < n; ++i)
    if (cls[i] < 1 || cls[i] > n_classes)
      return set_error(SR_ERR_INVALID_ARG, "row " + std::to_string(i) + ": class " + std::to_string(cls[i]) +
                                               " outside 1.." + std::to_string(n_classes));
  Lock l(ctx);
  SR_HIP_CHECK(hipSetDevice(ctx->device));
  if (dtype == SR_DTYPE_F32) return upload_impl<float>(ctx, X, nfeatures, n, y, weights, out, cls, n_classes);
  if (dtype == SR_DTYPE_F64) return upload_impl<double>(ctx, X, nfeatures, n, y, weights, out, cls, n_classes);
  return set_error(SR_ERR_INVALID_ARG, "unknown dtype");
}

int sr_dataset_free(sr_dataset* ds) {
  if (!ds) return SR_OK;
  if (ds->ctx) {
    Lock l(ds->ctx);
    (void)hipSetDevice(ds->ctx->device);
    (void)hipStreamSynchronize(ds->ctx->stream);
    if (ds->X) (void)hipFree(ds->X);
    if (ds->y) (void)hipFree(ds->y);
    if (ds->w) (void)hipFree(ds->w);
    if (ds->probe_rows) (void)hipFree(ds->probe_rows);
  }
  delete ds;
  return SR_OK;
}

int sr_dataset_info(const sr_dataset* ds, int* dtype, int64_t* nfeatures, int64_t* n) {
  if (!ds) return set_error(SR_ERR_INVALID_ARG, "NULL dataset");
  if (dtype) *dtype = ds->dtype;
  if (nfeatures) *nfeatures = ds->nf;
  if (n) *n = ds->n;
  return SR_OK;
}

int sr_dataset_denominator(const sr_dataset* ds, double* denom) {
  if (!ds || !denom) return set_error(SR_ERR_INVALID_ARG, "NULL argument");
  *denom = ds->w ? ds->wsum : double(ds->n);
  return SR_OK;
}

// The eleven sr_eval_loss_batch* / sr_eval_grad_batch* / sr_eval_tree_array* entry points fill an EvalReq and
// call eval_entry: the refusals in their order, the lock, the device, then the call for the dataset's type.
namespace {
// a parametric call's batch against the dataset and the trees (the one copy of these checks: run_batch's
// stage_param_table and eval_grad_impl rely on them)
int check_params(const sr_dataset* ds, const sr_tree_batch* trees, const sr_param_batch* params) {
  if (!params) return set_error(SR_ERR_INVALID_ARG, "NULL parameter batch");
  if (ds->n_classes <= 0) return set_error(SR_ERR_INVALID_ARG, "a parametric call needs a dataset uploaded with classes");
  if (params->n_classes != ds->n_classes)
    return set_error(SR_ERR_INVALID_ARG, "sr_param_batch n_classes " + std::to_string(params->n_classes) +
                                             " differs from the dataset's " + std::to_string(ds->n_classes));
  if (params->max_parameters < 0 || params->max_parameters > 65535) return set_error(SR_ERR_INVALID_ARG, "bad max_parameters");
  if (trees->n_trees > 0 && (!params->is_parameter || !params->parameter || (params->max_parameters > 0 && !params->parameters)))
    return set_error(SR_ERR_INVALID_ARG, "sr_param_batch has NULL arrays");
  return SR_OK;
}

enum EvalKind { kEvalLoss, kEvalGrad, kEvalPred };

// req: as the entry point filled it — `views` set by the _views variants (several row views in one call,
// per-island minibatches; row_idx / n_idx then hold view_rows / view_len), `params` by the _parametric ones
// (`parametric`: the variant takes a parameter batch, so a NULL one is refused).  out: the losses or the
// predictions.
int eval_entry(sr_ctx* ctx, EvalReq& req, EvalKind kind, bool parametric, void* out, void* out_grad, uint8_t* out_complete) {
  if (parametric && kind != kEvalPred && req.loss_kind >= kLossExprBase) return set_error(SR_ERR_INVALID_ARG, kLossExprOnly);
  int rc = validate_common(ctx, req.ds, req.opset_id, req.trees);
  if (rc != SR_OK) return rc;
  if (parametric && (rc = check_params(req.ds, req.trees, req.params)) != SR_OK) return rc;
  if (req.views && (req.views->n_views < 1 || req.views->view_len < 1 || !req.row_idx ||
                    (req.trees->n_trees > 0 && !req.views->tree_view)))
    return set_error(SR_ERR_INVALID_ARG, "bad row views");
  if (kind == kEvalGrad) {
    if (req.trees->n_trees > 0 && (!out || !out_grad || !out_complete))
      return set_error(SR_ERR_INVALID_ARG, "NULL output buffers");
    if (!req.ds->y) return set_error(SR_ERR_INVALID_ARG, "dataset has no y");
  }
  Lock l(ctx);
  SR_HIP_CHECK(hipSetDevice(ctx->device));
  if (req.views && req.views->n_views == 1) req.views = nullptr;  // (one view: the plain gather path)
  auto go = [&](auto tag) -> int {
    using T = decltype(tag);
    if (kind == kEvalLoss) return eval_loss_impl<T>(ctx, req, out, out_complete);
    if (kind == kEvalGrad) return eval_grad_impl<T>(ctx, req, out, out_grad, out_complete);
    return eval_pred_impl<T>(ctx, req, out, out_complete);
  };
  return req.ds->dtype == SR_DTYPE_F32 ? go(float{}) : go(double{});
}
}  // namespace

int sr_eval_loss_batch(sr_ctx* ctx, const sr_dataset* ds, int opset_id, const sr_tree_batch* trees,
                       const int64_t* row_idx, int64_t n_idx, int loss_kind, void* out_loss, uint8_t* out_complete) {
  EvalReq req{ds, opset_id, trees, nullptr, row_idx, n_idx, nullptr, loss_kind};
  return eval_entry(ctx, req, kEvalLoss, false, out_loss, nullptr, out_complete);
}

int sr_eval_loss_batch_parametric(sr_ctx* ctx, const sr_dataset* ds, int opset_id, const sr_tree_batch* trees,
                                  const sr_param_batch* params, const int64_t* row_idx, int64_t n_idx, int loss_kind,
                                  void* out_loss, uint8_t* out_complete) {
  EvalReq req{ds, opset_id, trees, params, row_idx, n_idx, nullptr, loss_kind};
  return eval_entry(ctx, req, kEvalLoss, true, out_loss, nullptr, out_complete);
}

int sr_eval_loss_batch_views(sr_ctx* ctx, const sr_dataset* ds, int opset_id, const sr_tree_batch* trees,
                             const int32_t* tree_view, int n_views, const int64_t* view_rows, int64_t view_len,
                             int loss_kind, void* out_loss, uint8_t* out_complete) {
  const ViewSpec vs{tree_view, n_views, view_len};
  EvalReq req{ds, opset_id, trees, nullptr, view_rows, view_len, &vs, loss_kind};
  return eval_entry(ctx, req, kEvalLoss, false, out_loss, nullptr, out_complete);
}

int sr_eval_loss_batch_views_parametric(sr_ctx* ctx, const sr_dataset* ds, int opset_id, const sr_tree_batch* trees,
                                        const sr_param_batch* params, const int32_t* tree_view, int n_views,
                                        const int64_t* view_rows, int64_t view_len, int loss_kind, void* out_loss,
                                        uint8_t* out_complete) {
  const ViewSpec vs{tree_view, n_views, view_len};
  EvalReq req{ds, opset_id, trees, params, view_rows, view_len, &vs, loss_kind};
  return eval_entry(ctx, req, kEvalLoss, true, out_loss, nullptr, out_complete);
}

int sr_eval_grad_batch(sr_ctx* ctx, const sr_dataset* ds, int opset_id, const sr_tree_batch* trees,
                       const int64_t* row_idx, int64_t n_idx, int loss_kind, void* out_loss, void* out_grad,
                       uint8_t* out_complete) {
  EvalReq req{ds, opset_id, trees, nullptr, row_idx, n_idx, nullptr, loss_kind};
  return eval_entry(ctx, req, kEvalGrad, false, out_loss, out_grad, out_complete);
}

// Gradients of ParametricExpression trees: per tree [nc constants | K x C parameter entries, column-major]
// (sr_param_pack.h); the loss and flags are sr_eval_loss_batch(_views)_parametric's.
int sr_eval_grad_batch_parametric(sr_ctx* ctx, const sr_dataset* ds, int opset_id, const sr_tree_batch* trees,
                                  const sr_param_batch* params, const int64_t* row_idx, int64_t n_idx, int loss_kind,
                                  void* out_loss, void* out_grad, uint8_t* out_complete) {
  EvalReq req{ds, opset_id, trees, params, row_idx, n_idx, nullptr, loss_kind};
  return eval_entry(ctx, req, kEvalGrad, true, out_loss, out_grad, out_complete);
}

// Gradients with tied / frozen constants (sr_scalar_ties): per tree [n_scalars | K x C when params]; the
// loss and flags are the untied calls'.
int sr_eval_grad_batch_tied(sr_ctx* ctx, const sr_dataset* ds, int opset_id, const sr_tree_batch* trees,
                            const sr_param_batch* params, const sr_scalar_ties* ties, const int64_t* row_idx,
                            int64_t n_idx, int loss_kind, void* out_loss, void* out_grad, uint8_t* out_complete) {
  if (!ties || (trees && trees->n_trees > 0 && (!ties->slot || !ties->n_scalars)))
    return set_error(SR_ERR_INVALID_ARG, "NULL scalar ties");
  EvalReq req{ds, opset_id, trees, params, row_idx, n_idx, nullptr, loss_kind, ties};
  return eval_entry(ctx, req, kEvalGrad, params != nullptr, out_loss, out_grad, out_complete);
}

int sr_eval_grad_batch_views(sr_ctx* ctx, const sr_dataset* ds, int opset_id, const sr_tree_batch* trees,
                             const int32_t* tree_view, int n_views, const int64_t* view_rows, int64_t view_len,
                             int loss_kind, void* out_loss, void* out_grad, uint8_t* out_complete) {
  const ViewSpec vs{tree_view, n_views, view_len};
  EvalReq req{ds, opset_id, trees, nullptr, view_rows, view_len, &vs, loss_kind};
  return eval_entry(ctx, req, kEvalGrad, false, out_loss, out_grad, out_complete);
}

int sr_eval_grad_batch_views_parametric(sr_ctx* ctx, const sr_dataset* ds, int opset_id, const sr_tree_batch* trees,
                                        const sr_param_batch* params, const int32_t* tree_view, int n_views,
                                        const int64_t* view_rows, int64_t view_len, int loss_kind, void* out_loss,
                                        void* out_grad, uint8_t* out_complete) {
  const ViewSpec vs{tree_view, n_views, view_len};
  EvalReq req{ds, opset_id, trees, params, view_rows, view_len, &vs, loss_kind};
  return eval_entry(ctx, req, kEvalGrad, true, out_loss, out_grad, out_complete);
}

int sr_eval_tree_array(sr_ctx* ctx, const sr_dataset* ds, int opset_id, const sr_tree_batch* trees,
                       const int64_t* row_idx, int64_t n_idx, void* out_pred, uint8_t* out_complete) {
  EvalReq req{ds, opset_id, trees, nullptr, row_idx, n_idx, nullptr, SR_LOSS_L2DIST};
  return eval_entry(ctx, req, kEvalPred, false, out_pred, nullptr, out_complete);
}

int sr_eval_tree_array_parametric(sr_ctx* ctx, const sr_dataset* ds, int opset_id, const sr_tree_batch* trees,
                                  const sr_param_batch* params, const int64_t* row_idx, int64_t n_idx, void* out_pred,
                                  uint8_t* out_complete) {
  EvalReq req{ds, opset_id, trees, params, row_idx, n_idx, nullptr, SR_LOSS_L2DIST};
  return eval_entry(ctx, req, kEvalPred, true, out_pred, nullptr, out_complete);
}

namespace {
// the per-row derivative calls' refusals, the lock, the device, then the call for the dataset's type
int row_grad_entry(sr_ctx* ctx, const sr_dataset* ds, int opset_id, const sr_tree_batch* trees, const int64_t* row_idx,
                   int64_t n_idx, int mode, const int32_t* direction, void* out_pred, void* out_grad, uint8_t* out_complete) {
  int rc = validate_common(ctx, ds, opset_id, trees);
  if (rc != SR_OK) return rc;
  if (trees->n_trees > 0 && (!out_pred || !out_grad || !out_complete)) return set_error(SR_ERR_INVALID_ARG, "NULL output buffers");
  if (mode == kRowGradDiff) {
    if (trees->n_trees > 0 && !direction) return set_error(SR_ERR_INVALID_ARG, "NULL direction");
    for (int64_t t = 0; t < trees->n_trees; ++t)
      if (direction[t] < 1 || int64_t(direction[t]) > ds->nf)
        return set_error(SR_ERR_INVALID_ARG, "tree " + std::to_string(t) + ": direction " + std::to_string(direction[t]) +
                                                 " outside 1.." + std::to_string(ds->nf));
  }
  EvalReq req{ds, opset_id, trees, nullptr, row_idx, n_idx, nullptr, SR_LOSS_L2DIST};
  Lock l(ctx);
  SR_HIP_CHECK(hipSetDevice(ctx->device));
  return ds->dtype == SR_DTYPE_F32 ? eval_row_grad_impl<float>(ctx, req, mode, direction, out_pred, out_grad, out_complete)
                                   : eval_row_grad_impl<double>(ctx, req, mode, direction, out_pred, out_grad, out_complete);
}
}  // namespace

int sr_eval_grad_tree_array(sr_ctx* ctx, const sr_dataset* ds, int opset_id, const sr_tree_batch* trees,
                            const int64_t* row_idx, int64_t n_idx, int variable, void* out_pred, void* out_grad,
                            uint8_t* out_complete) {
  return row_grad_entry(ctx, ds, opset_id, trees, row_idx, n_idx, variable ? kRowGradFeatures : kRowGradConsts, nullptr,
                        out_pred, out_grad, out_complete);
}

int sr_eval_diff_tree_array(sr_ctx* ctx, const sr_dataset* ds, int opset_id, const sr_tree_batch* trees,
                            const int64_t* row_idx, int64_t n_idx, const int32_t* direction, void* out_pred,
                            void* out_diff, uint8_t* out_complete) {
  return row_grad_entry(ctx, ds, opset_id, trees, row_idx, n_idx, kRowGradDiff, direction, out_pred, out_diff, out_complete);
}

int sr_eval_loss_partials(sr_ctx* ctx, const sr_dataset* ds, int opset_id, const sr_tree_batch* trees,
                          int64_t n_total, int loss_kind, double* out_sum, uint32_t* out_flags, int out_on_device) {
  if (loss_kind >= kLossExprBase) return set_error(SR_ERR_INVALID_ARG, kLossExprOnly);
  int rc = validate_common(ctx, ds, opset_id, trees);
  if (rc != SR_OK) return rc;
  const int64_t nt = trees->n_trees;
  if (nt > 0 && (!out_sum || !out_flags)) return set_error(SR_ERR_INVALID_ARG, "NULL output buffers");
  if (n_total < ds->n) return set_error(SR_ERR_INVALID_ARG, "n_total smaller than this shard");
  Lock l(ctx);
  SR_HIP_CHECK(hipSetDevice(ctx->device));
  const EvalReq req{ds, opset_id, trees, nullptr, nullptr, 0, nullptr, loss_kind};
  BatchWants want;
  want.n_total = n_total;
  BatchResult res;
  auto t0 = std::chrono::steady_clock::now();
  rc = run_batch_any(ctx, req, want, &res);
  if (rc != SR_OK || nt == 0) return rc;
  hipStream_t s = ctx->stream;
  const hipMemcpyKind kind = out_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  SR_HIP_CHECK(hipMemcpyAsync(out_sum, ctx->d_out_sum, size_t(nt) * sizeof(double), kind, s));
  SR_HIP_CHECK(hipMemcpyAsync(out_flags, ctx->d_out_flag, size_t(nt) * sizeof(uint32_t), kind, s));
  SR_HIP_CHECK(hipStreamSynchronize(s));
  ctx->timing_pending = true;
  ctx->last_total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return SR_OK;
}

int sr_eval_loss_partials_packed(sr_ctx* ctx, const sr_dataset* ds, int opset_id, const sr_tree_batch* trees,
                                 int64_t n_total, int loss_kind, double* out, int out_on_device) {
  if (loss_kind >= kLossExprBase) return set_error(SR_ERR_INVALID_ARG, kLossExprOnly);
  int rc = validate_common(ctx, ds, opset_id, trees);
  if (rc != SR_OK) return rc;
  const int64_t nt = trees->n_trees;
  if (nt > 0 && !out) return set_error(SR_ERR_INVALID_ARG, "NULL output buffer");
  if (n_total < ds->n) return set_error(SR_ERR_INVALID_ARG, "n_total smaller than this shard");
  Lock l(ctx);
  SR_HIP_CHECK(hipSetDevice(ctx->device));
  const EvalReq req{ds, opset_id, trees, nullptr, nullptr, 0, nullptr, loss_kind};
  BatchWants want;
  want.n_total = n_total;
  BatchResult res;
  auto t0 = std::chrono::steady_clock::now();
  rc = run_batch_any(ctx, req, want, &res);
  if (rc != SR_OK || nt == 0) return rc;
  hipStream_t s = ctx->stream;
  const size_t bytes = size_t(5) * size_t(nt) * sizeof(double);
  double* dst = out;
  if (!out_on_device) {
    SR_HIP_CHECK(ctx->packed.ensure(bytes));
    dst = ctx->packed.as<double>();
  }
  SR_HIP_CHECK(sr_launch_pack_partials(ctx->d_out_sum, ctx->d_out_flag, int(nt), dst, s));
  if (!out_on_device) SR_HIP_CHECK(hipMemcpyAsync(out, dst, bytes, hipMemcpyDeviceToHost, s));
  SR_HIP_CHECK(hipStreamSynchronize(s));
  ctx->timing_pending = true;
  ctx->last_total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return SR_OK;
}

int sr_comm_unique_id(void* out_id) {
  if (!out_id) return set_error(SR_ERR_INVALID_ARG, "NULL output");
  if (check_runtime_pair() != SR_OK) return SR_ERR_HIP;
  ncclUniqueId id;
  const ncclResult_t r = ncclGetUniqueId(&id);
  if (r != ncclSuccess) return set_error(SR_ERR_HIP, std::string("ncclGetUniqueId: ") + ncclGetErrorString(r));
  static_assert(sizeof(id) == SR_COMM_ID_BYTES, "RCCL unique id size");
  std::memcpy(out_id, &id, sizeof(id));
  return SR_OK;
}

// A fresh transport: the collective buffers restart empty (every rank of the new group alike), shard
// layouts are re-exchanged (new generation).
static int install_comm(sr_ctx* ctx, std::unique_ptr<SrComm> x, int nranks, int rank) {
  for (DevBuf* b : {&ctx->coll_buf, &ctx->coll_packed}) b->release();
  ctx->h_coll.release();
  SR_HIP_CHECK(ctx->ctl.ensure(256));
  x->nranks = nranks;
  x->rank = rank;
  ctx->xport = std::move(x);
  ctx->comm_ranks = nranks;
  ctx->comm_rank = rank;
  ctx->comm_gen = ++g_comm_gen;
  return SR_OK;
}

int sr_comm_init(sr_ctx* ctx, int nranks, int rank, const void* id_bytes) {
  if (check_ctx(ctx) != SR_OK) return SR_ERR_INVALID_ARG;
  if (!id_bytes || nranks < 1 || rank < 0 || rank >= nranks) return set_error(SR_ERR_INVALID_ARG, "bad communicator arguments");
  Lock l(ctx);
  SR_HIP_CHECK(hipSetDevice(ctx->device));
  ctx->xport.reset();
  ctx->comm_ranks = 0;
  if (check_runtime_pair() != SR_OK) return SR_ERR_HIP;
  ncclUniqueId id;
  std::memcpy(&id, id_bytes, sizeof(id));
  auto x = std::make_unique<SrRcclComm>();
  const ncclResult_t r = ncclCommInitRank(&x->comm, nranks, id, rank);
  if (r != ncclSuccess) {
    x->comm = nullptr;
    return set_error(SR_ERR_HIP, std::string("ncclCommInitRank: ") + ncclGetErrorString(r));
  }
  return install_comm(ctx, std::move(x), nranks, rank);
}

int sr_comm_init_host(sr_ctx* ctx, int nranks, int rank, sr_host_allreduce_fn allreduce, sr_host_allgather_fn allgather,
                      void* user) {
  if (check_ctx(ctx) != SR_OK) return SR_ERR_INVALID_ARG;
  if (!allreduce || !allgather || nranks < 1 || rank < 0 || rank >= nranks)
    return set_error(SR_ERR_INVALID_ARG, "bad host communicator arguments");
  Lock l(ctx);
  SR_HIP_CHECK(hipSetDevice(ctx->device));
  ctx->xport.reset();
  ctx->comm_ranks = 0;
  auto x = std::make_unique<SrHostComm>();
  x->ar = allreduce;
  x->ag = allgather;
  x->user = user;
  return install_comm(ctx, std::move(x), nranks, rank);
}

int sr_comm_destroy(sr_ctx* ctx) {
  if (check_ctx(ctx) != SR_OK) return SR_ERR_INVALID_ARG;
  Lock l(ctx);
  ctx->xport.reset();
  ctx->comm_ranks = 0;
  return SR_OK;
}

// Row-sharded step with the exchange on the device: this shard's packed [5, n_trees] partials
// (sr_eval_loss_partials_packed) summed over every rank by ONE in-place all-reduce on the library's
// stream, then copied to out_host (every rank gets the global sums and flag counts).
int sr_eval_loss_partials_allreduce(sr_ctx* ctx, const sr_dataset* ds, int opset_id, const sr_tree_batch* trees,
                                    int64_t n_total, int loss_kind, double* out_host) {
  if (loss_kind >= kLossExprBase) return set_error(SR_ERR_INVALID_ARG, kLossExprOnly);
  if (check_ctx(ctx) != SR_OK) return SR_ERR_INVALID_ARG;
  if (!ctx->xport) return set_error(SR_ERR_INVALID_ARG, "no communicator: call sr_comm_init first");
  int rc = validate_common(ctx, ds, opset_id, trees);
  if (rc != SR_OK) return rc;
  const int64_t nt = trees->n_trees;
  if (nt > 0 && !out_host) return set_error(SR_ERR_INVALID_ARG, "NULL output buffer");
  if (n_total < ds->n) return set_error(SR_ERR_INVALID_ARG, "n_total smaller than this shard");
  Lock l(ctx);
  SR_HIP_CHECK(hipSetDevice(ctx->device));
  const size_t n = size_t(5) * size_t(nt > 0 ? nt : 0);
  Prep prep{ctx};
  prep.need(ctx->coll_packed, (n + 1) * sizeof(double));
  rc = agree_prep(ctx, prep);
  if (rc != SR_OK) return rc;
  const EvalReq req{ds, opset_id, trees, nullptr, nullptr, 0, nullptr, loss_kind};
  BatchWants want;
  want.n_total = n_total;
  BatchResult res;
  auto t0 = std::chrono::steady_clock::now();
  rc = run_batch_any(ctx, req, want, &res);
  int local = rc;
  hipStream_t s = ctx->stream;
  double* dst = ctx->coll_packed.as<double>();
  if (local == SR_OK && nt > 0 && sr_launch_pack_partials(ctx->d_out_sum, ctx->d_out_flag, int(nt), dst, s) != hipSuccess)
    local = set_error(SR_ERR_HIP, "pack partials failed");
  // every rank enters the collective, also with an empty batch (the counts agree: same trees) and
  // after a local failure (partials zeroed, the error word after them set): then every rank fails
  double err_word = local != SR_OK ? 1.0 : 0.0;
  if (local != SR_OK && hipMemsetAsync(dst, 0, n * sizeof(double), s) != hipSuccess) err_word = NAN;
  (void)hipMemcpyAsync(dst + n, &err_word, sizeof(double), hipMemcpyHostToDevice, s);
  rc = ctx->xport->allreduce_sum(dst, n + 1, s);
  if (rc != SR_OK) return local != SR_OK ? local : rc;
  double err_sum = 0.0;
  SR_HIP_CHECK(hipMemcpyAsync(&err_sum, dst + n, sizeof(double), hipMemcpyDeviceToHost, s));
  if (nt > 0) SR_HIP_CHECK(hipMemcpyAsync(out_host, dst, n * sizeof(double), hipMemcpyDeviceToHost, s));
  SR_HIP_CHECK(hipStreamSynchronize(s));
  if (err_sum != 0.0) return local != SR_OK ? local : set_error(SR_ERR_HIP, "the row-sharded step failed on a peer rank");
  ctx->timing_pending = true;
  ctx->last_total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return SR_OK;
}

int sr_eval_loss_sharded(sr_ctx* ctx, const sr_dataset* ds, int opset_id, const sr_tree_batch* trees, int loss_kind,
                         void* out_loss, uint8_t* out_complete) {
  if (loss_kind >= kLossExprBase) return set_error(SR_ERR_INVALID_ARG, kLossExprOnly);
  if (check_ctx(ctx) != SR_OK) return SR_ERR_INVALID_ARG;
  if (!ctx->xport) return set_error(SR_ERR_INVALID_ARG, "no communicator: call sr_comm_init first");
  int rc = validate_common(ctx, ds, opset_id, trees);
  if (rc != SR_OK) return rc;
  if (trees->n_trees > 0 && (!out_loss || !out_complete)) return set_error(SR_ERR_INVALID_ARG, "NULL output buffers");
  if (!ds->y) return set_error(SR_ERR_INVALID_ARG, "dataset has no y");
  Lock l(ctx);
  SR_HIP_CHECK(hipSetDevice(ctx->device));
  const EvalReq req{ds, opset_id, trees, nullptr, nullptr, 0, nullptr, loss_kind};
  if (ds->dtype == SR_DTYPE_F32)
    return eval_sharded_impl<float>(ctx, req, static_cast<float*>(out_loss), out_complete);
  return eval_sharded_impl<double>(ctx, req, static_cast<double*>(out_loss), out_complete);
}

int sr_eval_loss_tree_sharded(sr_ctx* ctx, const sr_dataset* ds, int opset_id, const sr_tree_batch* trees,
                              int loss_kind, void* out_loss, uint8_t* out_complete) {
  if (loss_kind >= kLossExprBase) return set_error(SR_ERR_INVALID_ARG, kLossExprOnly);
  if (check_ctx(ctx) != SR_OK) return SR_ERR_INVALID_ARG;
  if (!ctx->xport) return set_error(SR_ERR_INVALID_ARG, "no communicator: call sr_comm_init first");
  int rc = validate_common(ctx, ds, opset_id, trees);
  if (rc != SR_OK) return rc;
  if (trees->n_trees > 0 && (!out_loss || !out_complete)) return set_error(SR_ERR_INVALID_ARG, "NULL output buffers");
  if (trees->n_trees > 0 && !trees->offsets) return set_error(SR_ERR_INVALID_ARG, "sr_tree_batch has NULL arrays");
  Lock l(ctx);
  SR_HIP_CHECK(hipSetDevice(ctx->device));
  const EvalReq req{ds, opset_id, trees, nullptr, nullptr, 0, nullptr, loss_kind};
  if (ds->dtype == SR_DTYPE_F32)
    return eval_tree_sharded_impl<float>(ctx, req, static_cast<float*>(out_loss), out_complete);
  return eval_tree_sharded_impl<double>(ctx, req, static_cast<double*>(out_loss), out_complete);
}

int sr_comm_info(sr_ctx* ctx, int* nranks, int* rank, char* paths, int64_t capacity) {
  if (check_ctx(ctx) != SR_OK) return SR_ERR_INVALID_ARG;
  Lock l(ctx);
  if (nranks || rank) {
    if (!ctx->xport) return set_error(SR_ERR_INVALID_ARG, "no communicator: call sr_comm_init first");
    int c = ctx->comm_ranks, r = ctx->comm_rank;
    if (auto* rc = dynamic_cast<SrRcclComm*>(ctx->xport.get())) {  // as RCCL itself reports them
      SR_NCCL_CHECK(ncclCommCount(rc->comm, &c));
      SR_NCCL_CHECK(ncclCommUserRank(rc->comm, &r));
    }
    if (nranks) *nranks = c;
    if (rank) *rank = r;
  }
  if (paths && capacity > 0 && ctx->xport) {  // "transport=rccl|host;hip=...;rccl=..."
    const std::string p = std::string("transport=") + ctx->xport->kind() + ";" + runtime_paths();
    const size_t n = std::min(p.size(), size_t(capacity - 1));
    std::memcpy(paths, p.data(), n);
    paths[n] = '\0';
    return SR_OK;
  }
  return sr_runtime_info(paths, capacity);
}

int sr_runtime_info(char* paths, int64_t capacity) {
  if (!paths || capacity <= 0) return SR_OK;
  const std::string p = runtime_paths();
  const size_t n = std::min(p.size(), size_t(capacity - 1));
  std::memcpy(paths, p.data(), n);
  paths[n] = '\0';
  return SR_OK;
}

int sr_max_checks(sr_ctx* ctx, int dtype, int opset_id, const sr_tree_batch* trees, int* max_checks) {
  if (check_ctx(ctx) != SR_OK) return SR_ERR_INVALID_ARG;
  if (!trees || !max_checks || opset_id < 0 || opset_id >= int(ctx->opsets.size()) ||
      (dtype != SR_DTYPE_F32 && dtype != SR_DTYPE_F64))
    return set_error(SR_ERR_INVALID_ARG, "bad arguments");
  // compiled in the batch's own element type (`val` holds T): the same programs the eval calls build
  std::string err;
  auto go = [&](auto tag) -> int {
    using T = decltype(tag);
    SrProgramBatch<T> prog;
    const int rc = sr_compile_batch<T>(*trees, ctx->opsets[opset_id], 1, 65535, false, &prog, &err);
    if (rc != SR_OK) return set_error(rc, err);
    *max_checks = prog.max_checks;
    return SR_OK;
  };
  return dtype == SR_DTYPE_F32 ? go(0.0f) : go(0.0);
}

int sr_jsum_range_count(int64_t row_offset, int64_t n_local, int64_t n_total, int64_t* out_n_ranges) {
  if (!out_n_ranges || row_offset < 0 || n_local < 1 || row_offset + n_local > n_total)
    return set_error(SR_ERR_INVALID_ARG, "bad shard bounds");
  *out_n_ranges = int64_t(jl_ranges(row_offset, n_local, n_total).size());
  return SR_OK;
}

int sr_jsum_ranges(int64_t row_offset, int64_t n_local, int64_t n_total, int64_t* lo, int64_t* hi, int64_t* leaf,
                   uint8_t* head) {
  if (row_offset < 0 || n_local < 1 || row_offset + n_local > n_total) return set_error(SR_ERR_INVALID_ARG, "bad shard bounds");
  const std::vector<JlRange> r = jl_ranges(row_offset, n_local, n_total);
  for (size_t i = 0; i < r.size(); ++i) {
    if (lo) lo[i] = r[i].lo;
    if (hi) hi[i] = r[i].hi;
    if (leaf) leaf[i] = r[i].leaf;
    if (head) head[i] = r[i].head ? 1 : 0;
  }
  return SR_OK;
}

int sr_jsum_partials(sr_ctx* ctx, const sr_dataset* ds, int opset_id, const sr_tree_batch* trees,
                     const int64_t* tree_list, int64_t n_list, int max_checks, int64_t row_offset, int64_t n_total,
                     void* out_vals) {
  int rc = validate_common(ctx, ds, opset_id, trees);
  if (rc != SR_OK) return rc;
  if (n_list < 0 || (n_list > 0 && (!tree_list || !out_vals)) || max_checks < 0)
    return set_error(SR_ERR_INVALID_ARG, "bad tree list");
  if (row_offset < 0 || row_offset + ds->n > n_total) return set_error(SR_ERR_INVALID_ARG, "bad shard bounds");
  for (int64_t i = 0; i < n_list; ++i)
    if (tree_list[i] < 0 || tree_list[i] >= trees->n_trees) return set_error(SR_ERR_INVALID_ARG, "tree index out of range");
  if (n_list == 0 || max_checks == 0) return SR_OK;
  Lock l(ctx);
  SR_HIP_CHECK(hipSetDevice(ctx->device));
  const EvalReq req{ds, opset_id, trees, nullptr, nullptr, 0, nullptr, SR_LOSS_L2DIST};
  BatchWants want;
  want.n_total = n_total;
  BatchResult res;
  const std::vector<JlRange> ranges = jl_ranges(row_offset, ds->n, n_total);
  auto go = [&](auto tag) -> int {
    using T = decltype(tag);
    SrProgramBatch<T> prog;
    int r = run_batch<T>(ctx, req, want, &prog, &res);
    if (r != SR_OK) return r;
    SR_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (prog.max_checks > max_checks) return set_error(SR_ERR_INVALID_ARG, "max_checks too small");
    return run_exact<T>(ctx, req, prog, tree_list, n_list, max_checks, ranges, static_cast<T*>(out_vals));
  };
  return ds->dtype == SR_DTYPE_F32 ? go(float{}) : go(double{});
}

int sr_jsum_finite(int dtype, int64_t n_total, int n_ranks, const int64_t* row_offsets, const void* const* rank_vals,
                   int64_t n_arrays, uint8_t* out_finite) {
  if (n_total < 1 || n_ranks < 1 || !row_offsets || !rank_vals || n_arrays < 0 || (n_arrays > 0 && !out_finite))
    return set_error(SR_ERR_INVALID_ARG, "bad arguments");
  if (row_offsets[0] != 0 || row_offsets[n_ranks] != n_total) return set_error(SR_ERR_INVALID_ARG, "shards must cover [0, n_total)");
  for (int r = 0; r < n_ranks; ++r)
    if (row_offsets[r + 1] <= row_offsets[r] || !rank_vals[r]) return set_error(SR_ERR_INVALID_ARG, "bad shard bounds");
  if (dtype == SR_DTYPE_F32)
    jl_finite<float>(n_total, n_ranks, row_offsets, reinterpret_cast<const float* const*>(rank_vals), n_arrays, out_finite);
  else if (dtype == SR_DTYPE_F64)
    jl_finite<double>(n_total, n_ranks, row_offsets, reinterpret_cast<const double* const*>(rank_vals), n_arrays,
                      out_finite);
  else
    return set_error(SR_ERR_INVALID_ARG, "unknown dtype");
  return SR_OK;
}

int sr_finalize_losses(int dtype, int64_t n_trees, const double* sums, const uint32_t* flags, double denom,
                       const int64_t* tree_list, int64_t n_list, const uint8_t* list_ok, void* out_loss,
                       uint8_t* out_complete) {
  if (n_trees < 0 || (n_trees > 0 && (!sums || !flags || !out_loss || !out_complete)))
    return set_error(SR_ERR_INVALID_ARG, "bad arguments");
  if (n_list > 0 && (!tree_list || !list_ok)) return set_error(SR_ERR_INVALID_ARG, "NULL tree list");
  for (int64_t i = 0; i < n_list; ++i)
    if (tree_list[i] < 0 || tree_list[i] >= n_trees) return set_error(SR_ERR_INVALID_ARG, "tree index out of range");
  if (dtype == SR_DTYPE_F32)
    finalize<float>(n_trees, sums, flags, denom, tree_list, n_list, list_ok, static_cast<float*>(out_loss), out_complete);
  else if (dtype == SR_DTYPE_F64)
    finalize<double>(n_trees, sums, flags, denom, tree_list, n_list, list_ok, static_cast<double*>(out_loss),
                     out_complete);
  else
    return set_error(SR_ERR_INVALID_ARG, "unknown dtype");
  return SR_OK;
}

static int compile_info_impl(int dtype, int n_unary, const char* const* unary_names, int n_binary,
                             const char* const* binary_names, const sr_tree_batch* trees, const SrParamNodes* pn,
                             int64_t n_rows, int64_t nfeatures, int32_t* out_len, uint8_t* out_static_bad,
                             int32_t* out_max_depth, void* out_code, int64_t code_capacity, bool grad = false,
                             const sr_scalar_ties* ties = nullptr) {
  if (!trees || n_unary < 0 || n_binary < 0 || (n_unary > 0 && !unary_names) || (n_binary > 0 && !binary_names))
    return set_error(SR_ERR_INVALID_ARG, "bad arguments");
  SrOpset o;
  for (int i = 0; i < n_unary; ++i) {
    const uint32_t id = unary_names[i] ? sr_unary_id(unary_names[i]) : 0;
    if (!id) return set_error(SR_ERR_UNSUPPORTED_OP, std::string("unsupported unary operator: ") +
                                                         (unary_names[i] ? unary_names[i] : "(null)"));
    o.unary.push_back(id);
  }
  for (int i = 0; i < n_binary; ++i) {
    const uint32_t id = binary_names[i] ? sr_binary_id(binary_names[i]) : 0;
    if (!id) return set_error(SR_ERR_UNSUPPORTED_OP, std::string("unsupported binary operator: ") +
                                                         (binary_names[i] ? binary_names[i] : "(null)"));
    o.binary.push_back(id);
  }
  std::string err;
  auto report = [&](auto& prog) -> int {
    const int64_t nt = trees->n_trees;
    for (int64_t t = 0; t < nt; ++t) {
      if (out_len) out_len[t] = int32_t(prog.offsets[size_t(t) + 1] - prog.offsets[size_t(t)]);
      if (out_static_bad) out_static_bad[t] = prog.static_bad[size_t(t)];
    }
    if (out_max_depth) *out_max_depth = prog.max_depth;
    if (out_code) {
      const int64_t n = int64_t(prog.code.size()) < code_capacity ? int64_t(prog.code.size()) : code_capacity;
      std::memcpy(out_code, prog.code.data(), size_t(n) * 16);
    }
    return SR_OK;
  };
  if (dtype == SR_DTYPE_F32) {
    SrProgramBatch<float> prog;
    int rc = sr_compile_batch<float>(*trees, o, n_rows, nfeatures, grad, &prog, &err, nullptr, pn, ties);
    if (rc != SR_OK) return set_error(rc, err);
    return report(prog);
  }
  if (dtype == SR_DTYPE_F64) {
    SrProgramBatch<double> prog;
    int rc = sr_compile_batch<double>(*trees, o, n_rows, nfeatures, grad, &prog, &err, nullptr, pn, ties);
    if (rc != SR_OK) return set_error(rc, err);
    return report(prog);
  }
  return set_error(SR_ERR_INVALID_ARG, "unknown dtype");
}

int sr_compile_info(int dtype, int n_unary, const char* const* unary_names, int n_binary,
                    const char* const* binary_names, const sr_tree_batch* trees, int64_t n_rows,
                    int64_t nfeatures, int32_t* out_len, uint8_t* out_static_bad, int32_t* out_max_depth,
                    void* out_code, int64_t code_capacity) {
  return compile_info_impl(dtype, n_unary, unary_names, n_binary, binary_names, trees, nullptr, n_rows, nfeatures,
                           out_len, out_static_bad, out_max_depth, out_code, code_capacity);
}

int sr_compile_info_parametric(int dtype, int n_unary, const char* const* unary_names, int n_binary,
                               const char* const* binary_names, const sr_tree_batch* trees,
                               const sr_param_batch* params, int64_t n_rows, int64_t nfeatures, int32_t* out_len,
                               uint8_t* out_static_bad, int32_t* out_max_depth, void* out_code,
                               int64_t code_capacity) {
  if (!params) return set_error(SR_ERR_INVALID_ARG, "NULL parameter batch");
  if (params->max_parameters < 0 || params->max_parameters > 65535) return set_error(SR_ERR_INVALID_ARG, "bad max_parameters");
  const SrParamNodes pn{params->is_parameter, params->parameter, params->max_parameters};
  return compile_info_impl(dtype, n_unary, unary_names, n_binary, binary_names, trees, &pn, n_rows, nfeatures, out_len,
                           out_static_bad, out_max_depth, out_code, code_capacity);
}

int sr_compile_info_grad(int dtype, int n_unary, const char* const* unary_names, int n_binary,
                         const char* const* binary_names, const sr_tree_batch* trees, int64_t n_rows,
                         int64_t nfeatures, int32_t* out_len, uint8_t* out_static_bad, int32_t* out_max_depth,
                         void* out_code, int64_t code_capacity) {
  return compile_info_impl(dtype, n_unary, unary_names, n_binary, binary_names, trees, nullptr, n_rows, nfeatures,
                           out_len, out_static_bad, out_max_depth, out_code, code_capacity, true);
}

int sr_compile_info_grad_parametric(int dtype, int n_unary, const char* const* unary_names, int n_binary,
                                    const char* const* binary_names, const sr_tree_batch* trees,
                                    const sr_param_batch* params, int64_t n_rows, int64_t nfeatures,
                                    int32_t* out_len, uint8_t* out_static_bad, int32_t* out_max_depth,
                                    void* out_code, int64_t code_capacity) {
  if (!params) return set_error(SR_ERR_INVALID_ARG, "NULL parameter batch");
  if (params->max_parameters < 0 || params->max_parameters > 65535) return set_error(SR_ERR_INVALID_ARG, "bad max_parameters");
  const SrParamNodes pn{params->is_parameter, params->parameter, params->max_parameters};
  return compile_info_impl(dtype, n_unary, unary_names, n_binary, binary_names, trees, &pn, n_rows, nfeatures, out_len,
                           out_static_bad, out_max_depth, out_code, code_capacity, true);
}

int sr_compile_info_grad_tied(int dtype, int n_unary, const char* const* unary_names, int n_binary,
                              const char* const* binary_names, const sr_tree_batch* trees,
                              const sr_param_batch* params, const sr_scalar_ties* ties, int64_t n_rows,
                              int64_t nfeatures, int32_t* out_len, uint8_t* out_static_bad, int32_t* out_max_depth,
                              void* out_code, int64_t code_capacity) {
  if (!ties) return set_error(SR_ERR_INVALID_ARG, "NULL scalar ties");
  if (params && (params->max_parameters < 0 || params->max_parameters > 65535)) return set_error(SR_ERR_INVALID_ARG, "bad max_parameters");
  SrParamNodes pn{};
  if (params) pn = SrParamNodes{params->is_parameter, params->parameter, params->max_parameters};
  return compile_info_impl(dtype, n_unary, unary_names, n_binary, binary_names, trees, params ? &pn : nullptr, n_rows,
                           nfeatures, out_len, out_static_bad, out_max_depth, out_code, code_capacity, true, ties);
}

int sr_host_unary(int dtype, const char* name, int64_t n, const void* x, void* out) {
  const uint32_t id = name ? sr_unary_id(name) : 0;
  if (!id) return set_error(SR_ERR_UNSUPPORTED_OP, std::string("unsupported unary operator: ") + (name ? name : "(null)"));
  if (n < 0 || (n > 0 && (!x || !out))) return set_error(SR_ERR_INVALID_ARG, "bad arguments");
  if (dtype == SR_DTYPE_F32) {
    for (int64_t i = 0; i < n; ++i) static_cast<float*>(out)[i] = sr_unary<float>(id, static_cast<const float*>(x)[i]);
  } else if (dtype == SR_DTYPE_F64) {
    for (int64_t i = 0; i < n; ++i) static_cast<double*>(out)[i] = sr_unary<double>(id, static_cast<const double*>(x)[i]);
  } else {
    return set_error(SR_ERR_INVALID_ARG, "unknown dtype");
  }
  return SR_OK;
}

int sr_host_elem_loss(int dtype, int kind, double param, int64_t n, const void* pred, const void* target,
                      void* out_value, void* out_deriv) {
  if (kind < 0 || kind >= SR_LOSS_COUNT) return set_error(SR_ERR_INVALID_ARG, "unknown loss kind");
  if (n < 0 || (n > 0 && (!pred || !target || !out_value || !out_deriv))) return set_error(SR_ERR_INVALID_ARG, "bad arguments");
  if (dtype == SR_DTYPE_F32) {
    const float* p = static_cast<const float*>(pred);
    const float* t = static_cast<const float*>(target);
    for (int64_t i = 0; i < n; ++i) {
      static_cast<float*>(out_value)[i] = sr_elem_loss<float>(kind, p[i], t[i], float(param));
      static_cast<float*>(out_deriv)[i] = sr_elem_loss_deriv<float>(kind, p[i], t[i], float(param));
    }
  } else if (dtype == SR_DTYPE_F64) {
    const double* p = static_cast<const double*>(pred);
    const double* t = static_cast<const double*>(target);
    for (int64_t i = 0; i < n; ++i) {
      static_cast<double*>(out_value)[i] = sr_elem_loss<double>(kind, p[i], t[i], param);
      static_cast<double*>(out_deriv)[i] = sr_elem_loss_deriv<double>(kind, p[i], t[i], param);
    }
  } else {
    return set_error(SR_ERR_INVALID_ARG, "unknown dtype");
  }
  return SR_OK;
}

// the last call's kernel / busy times from its events (computed on first request)
static void settle_timing(sr_ctx* ctx) {
  if (!ctx->timing_pending) return;
  ctx->timing_pending = false;
  ctx->last_eval_ms = chunk_kernel_ms(ctx);
  ctx->last_busy_ms = chunk_busy_ms(ctx);
  ctx->fold_kernel_ms_last = 0.0;
  if (ctx->last.fold_timed)
    for (int c = 0; c < ctx->last.n_chunks; ++c) {
      float m = 0.f;
      if (hipEventElapsedTime(&m, ctx->ev_fc0[c], ctx->ev_fc1[c]) == hipSuccess) ctx->fold_kernel_ms_last += double(m);
    }
}

int sr_last_phase_ms(sr_ctx* ctx, double* out, int n) {
  if (check_ctx(ctx) != SR_OK) return SR_ERR_INVALID_ARG;
  Lock l(ctx);
  if (n > 8) settle_timing(ctx);
  for (int i = 0; i < n && i < 5; ++i) out[i] = ctx->phase_ms[i];
  if (n > 5) out[5] = double(ctx->last.n_chunks);
  if (n > 6) out[6] = ctx->exact_kernel_ms;
  if (n > 7) out[7] = double(ctx->last.rows);
  if (n > 8) out[8] = ctx->last_busy_ms;
  if (n > 9) out[9] = double(ctx->n_fold_last);
  if (n > 10) out[10] = double(ctx->fold_slow_last);
  if (n > 11) out[11] = double(ctx->fold_seg_last);
  for (int i = 0; i < 4; ++i)
    if (n > 12 + i) out[12 + i] = ctx->fold_ms[i];
  if (n > 16 && !ctx->last.loss_list_read) {  // (the last call's listed loss launches: their counters, read once)
    int32_t h[kMaxChunks * kLossListCnt] = {};
    SR_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (ctx->stream2) SR_HIP_CHECK(hipStreamSynchronize(ctx->stream2));
    SR_HIP_CHECK(hipMemcpy(h, ctx->loss_list.as<char>() + sr_loss_list_cnt_off(ctx->last.loss_list_nt), sizeof(h),
                           hipMemcpyDeviceToHost));
    for (int c = 0; c < kMaxChunks; ++c) {
      if (ctx->last.loss_listed_np[c] <= 0) continue;
      ++ctx->last.n_loss_listed_launches;
      ctx->last.n_loss_live += h[c * kLossListCnt];
      ctx->last.n_loss_excl += ctx->last.loss_listed_np[c] - h[c * kLossListCnt];
    }
    ctx->last.loss_list_read = true;
  }
  if (n > 16) out[16] = double(ctx->last.n_loss_listed_launches);
  if (n > 17) out[17] = double(ctx->last.n_loss_live);
  if (n > 18) out[18] = double(ctx->last.n_loss_excl);
  // the last call's compacted FOLD launches, region r (sr_fold_region: 2 chunk, + 1 for the LDS-stack launch) at
  // out[19 + 4 r ..]: {live workgroups, listed entries, entries per workgroup g, the longest row block's list};
  // zeros for a region without such a launch
  if (n > 19 && !ctx->last.fold_wg_read) {
    SR_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (ctx->stream2) SR_HIP_CHECK(hipStreamSynchronize(ctx->stream2));
    std::vector<int32_t> h(sr_fold_wg_words(ctx->last.fold_wg_stride_rb));
    SR_HIP_CHECK(hipMemcpy(h.data(), ctx->fold_wg.p, h.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (int r = 0; r < 2 * kMaxChunks; ++r) {
      const int nrb = ctx->last.fold_wg_nrb[r];
      if (nrb <= 0) continue;
      const int32_t* cnt = h.data() + sr_fold_wg_off(r, ctx->last.fold_wg_stride_rb);
      const int32_t* wg0 = cnt + ctx->last.fold_wg_stride_rb;
      int64_t entries = 0, longest = 0;
      for (int b = 0; b < nrb; ++b) {
        entries += cnt[b];
        longest = std::max<int64_t>(longest, cnt[b]);
      }
      ctx->last.fold_wg_info[r][0] = double(wg0[nrb]);
      ctx->last.fold_wg_info[r][1] = double(entries);
      ctx->last.fold_wg_info[r][2] = double(wg0[nrb + 1]);
      ctx->last.fold_wg_info[r][3] = double(longest);
    }
    ctx->last.fold_wg_read = true;
  }
  for (int r = 0; r < 2 * kMaxChunks; ++r)
    for (int k = 0; k < 4; ++k)
      if (n > 19 + 4 * r + k) out[19 + 4 * r + k] = ctx->last.fold_wg_info[r][k];
  return SR_OK;
}

int sr_set_tuning(sr_ctx* ctx, const char* name, int64_t value) {
  if (check_ctx(ctx) != SR_OK) return SR_ERR_INVALID_ARG;
  if (!name) return set_error(SR_ERR_INVALID_ARG, "tuning knob name is NULL");
  Lock l(ctx);
  std::string err;
  return sr_knob_set(*ctx, name, value, &err) == 0 ? SR_OK : set_error(SR_ERR_INVALID_ARG, err);
}

int sr_last_grad_info(sr_ctx* ctx, int n, double* kernel_ms, double* flops, int64_t* items, int* rows_per_lane) {
  if (check_ctx(ctx) != SR_OK) return SR_ERR_INVALID_ARG;
  Lock l(ctx);
  for (int b = 0; b < n && b < sr_ctx::kGradBuckets; ++b) {
    float m = 0.f;
    if (kernel_ms)
      kernel_ms[b] = ctx->grad_ms_done[b] +
                     ((ctx->grad_timed[b] && hipEventElapsedTime(&m, ctx->ev_g0[b], ctx->ev_g1[b]) == hipSuccess) ? double(m) : 0.0);
    if (flops) flops[b] = ctx->grad_flops[b];
    if (items) items[b] = ctx->grad_items[b];
    if (rows_per_lane) rows_per_lane[b] = ctx->grad_rows[b];
  }
  return SR_OK;
}

int sr_tuning_info(sr_ctx* ctx, int* used_derived_columns, int64_t* exact_trees) {
  if (check_ctx(ctx) != SR_OK) return SR_ERR_INVALID_ARG;
  if (used_derived_columns) *used_derived_columns = ctx->last.n_derived;
  if (exact_trees) *exact_trees = ctx->n_exact_last;
  return SR_OK;
}

int sr_ref_fold_info(sr_ctx* ctx, int* path, int64_t* n_folded, int64_t* n_fallback, double* fold_kernel_ms) {
  if (check_ctx(ctx) != SR_OK) return SR_ERR_INVALID_ARG;
  Lock l(ctx);
  settle_timing(ctx);
  if (path) *path = ctx->last.fold_path;
  if (n_folded) *n_folded = ctx->n_ref_ok_last;
  if (n_fallback) *n_fallback = ctx->n_ref_fail_last;
  if (fold_kernel_ms) *fold_kernel_ms = ctx->fold_kernel_ms_last;
  return SR_OK;
}

int sr_last_fold_cand(sr_ctx* ctx, int64_t* taken, int64_t* rerun) {
  if (check_ctx(ctx) != SR_OK) return SR_ERR_INVALID_ARG;
  Lock l(ctx);
  if (!ctx->last.fold_cand_read) {  // (the plan's counters of the last FOLD-mode call, read once)
    int h[4] = {0, 0, 0, 0};
    SR_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (ctx->stream2) SR_HIP_CHECK(hipStreamSynchronize(ctx->stream2));
    SR_HIP_CHECK(hipMemcpy(h, ctx->fold_ctl.p, sizeof(h), hipMemcpyDeviceToHost));
    ctx->last.n_cand_taken = h[1];
    ctx->last.n_cand_rerun = h[2];
    ctx->last.fold_cand_read = true;
  }
  if (taken) *taken = ctx->last.n_cand_taken;
  if (rerun) *rerun = ctx->last.n_cand_rerun;
  return SR_OK;
}

#ifdef SR_STAMPS
// latency-analysis builds only (not in include/sr_amd.h): the last main launch's stamps
// [block][wave][SR_NSTAMPS] (wall clock, 100 MHz) and their count
int sr_debug_stamps(sr_ctx* ctx, uint64_t* out, int64_t cap, int64_t* n) {
  if (check_ctx(ctx) != SR_OK) return SR_ERR_INVALID_ARG;
  Lock lk(ctx);
  *n = ctx->n_stamps;
  if (ctx->n_stamps > 0 && out && cap >= ctx->n_stamps) {
    SR_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    SR_HIP_CHECK(hipMemcpy(out, ctx->stamps.p, size_t(ctx->n_stamps) * sizeof(uint64_t), hipMemcpyDeviceToHost));
  }
  return SR_OK;
}
#endif

int sr_last_kernel_ms(sr_ctx* ctx, double* eval_ms, double* total_ms) {
  if (check_ctx(ctx) != SR_OK) return SR_ERR_INVALID_ARG;
  Lock l(ctx);
  settle_timing(ctx);
  if (eval_ms) *eval_ms = ctx->last_eval_ms;
  if (total_ms) *total_ms = ctx->last_total_ms;
  return SR_OK;
}

}  // extern "C"
