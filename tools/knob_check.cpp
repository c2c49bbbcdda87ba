// knob_check.cpp — stand-alone host check of the tuning-knob table (csrc/sr_knobs.h; no GPU, no HIP, no
// Python).
//
// Build and run through `make -C symbolicregression.jl_amd knob-check`, which compiles this file with
// -fsanitize=address,undefined.  The expectations below are written out value by value from the rules the
// knobs had when each was spelled out in sr_init and sr_set_tuning, so the table cannot drift from them
// unnoticed: every default; what sr_set_tuning stores (or refuses, and with which message) for the inputs
// -5, 0, 1, 2, 7, 100 and 2^40; the names sr_set_tuning and the environment accept, no more and no fewer;
// the environment's rule (the same range, always clamped, inverse-sense variables).  Exit status 0 and
// "knob_check: ok" on success.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <string>

#include "../symbolicregression.jl_amd/csrc/sr_knobs.h"
#include "../symbolicregression.jl_amd/csrc/sr_plan.h"

namespace {

int g_failed = 0;
#define CHECK(cond)                                                         \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::fprintf(stderr, "knob_check: %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      if (++g_failed > 20) std::exit(1);                                    \
    }                                                                       \
  } while (0)

constexpr int64_t B = int64_t(1) << 40;
constexpr int64_t R = INT64_MIN;  // "refused: the member keeps its value"
constexpr int kInputs = 7;
constexpr int64_t kIn[kInputs] = {-5, 0, 1, 2, 7, 100, B};

void check_defaults() {
  const SrKnobs k;
  CHECK(k.tail_chunk == 4);
  CHECK(k.exact_early == 1);
  CHECK(k.fold_seg == -1);
  CHECK(k.host_reduce == 8192);
  CHECK(k.host_io == 1);
  CHECK(k.debug_hint_regrow == 0);
  CHECK(k.exact_g == 0);
  CHECK(k.exact_w == 4);
  CHECK(k.derived == 1);
  CHECK(k.stress_probe == 1);
  CHECK(k.code_cache == 1);
  CHECK(k.vstk_rows == 0);
  CHECK(k.grad_rows_force == 0);
  CHECK(k.grad_sort == 1);
  CHECK(k.grad_lane_bins == 1);
  CHECK(k.grad_stage_bytes == (int64_t(256) << 20));
  CHECK(k.first_chunk == 6);
  CHECK(k.chunk_min == 1024);
  CHECK(k.inject_fail == 0 && k.inject_post == 0 && k.inject_post_exact == 0 && k.inject_post_gather == 0 &&
        k.inject_post_wsum == 0);
  CHECK(k.timing == 1);
  CHECK(k.rows_override == 0);
  CHECK(k.tree_group == 0);
  CHECK(k.waves_override == 0);
  CHECK(k.cost_order == true);
  CHECK(k.balance_groups == true);
  CHECK(k.dead_hints == true);
  CHECK(k.max_row_blocks == 512);
  CHECK(k.chunks == 2);
  CHECK(k.probe == 2);
  CHECK(k.ref_fold == 1);
  CHECK(k.fold_store_mb == 512);
  CHECK(k.fold_slot_mb == 24576);
  CHECK(k.fold_delta_log2 == 8);
  CHECK(k.fold_seg_max == 16384);
  CHECK(k.fold_rows_max == (int64_t(1) << 24));
  CHECK(k.fold_debug_fail == 0);
  CHECK(k.fold_single_pass == 1);
  CHECK(k.fold_compact == 1);
  CHECK(k.fold_list_wgs == 2048);
  CHECK(k.loss_compact == 1);
  CHECK(k.loss_list_groups == 0);
  CHECK(k.fold_cand_est == 1);
  CHECK(k.fold_cand_est_min == 4);
  CHECK(k.fold_stats == 0);
}

// What sr_set_tuning(name, kIn[i]) leaves in the member `get` reads.
struct Expect {
  const char* name;
  int64_t (*get)(const SrKnobs&);
  int64_t out[kInputs];
  const char* refusal;
};
#define GET(field) [](const SrKnobs& k) { return int64_t(k.field); }
#define FLAG {1, 0, 1, 1, 1, 1, 1}      /* value != 0 */
#define RAW {-5, 0, 1, 2, 7, 100, 0}    /* int(value): 2^40 keeps its low 32 bits */
const Expect kExpect[] = {
    {"derived", GET(derived), FLAG, nullptr},
    {"grad_lane_bins", GET(grad_lane_bins), FLAG, nullptr},
    {"grad_sort", GET(grad_sort), FLAG, nullptr},
    {"grad_stage_bytes", GET(grad_stage_bytes), {1, 1, 1, 2, 7, 100, B}, nullptr},
    {"chunk_min", GET(chunk_min), {1, 1, 1, 2, 7, 100, B}, nullptr},
    {"first_chunk", GET(first_chunk), {2, 2, 2, 2, 7, 64, 64}, nullptr},
    {"max_row_blocks", GET(max_row_blocks), {1, 1, 1, 2, 7, 100, 65536}, nullptr},
    {"probe", GET(probe), RAW, nullptr},
    {"host_io", GET(host_io), {R, 0, 1, R, R, R, R}, "host_io must be 0 or 1"},
    {"vstk_rows", GET(vstk_rows), RAW, nullptr},
    {"grad_rows", GET(grad_rows_force), RAW, nullptr},
    {"host_reduce", GET(host_reduce), {0, 0, 1, 2, 7, 100, B}, nullptr},
    {"ref_fold", GET(ref_fold), FLAG, nullptr},
    {"fold_store_mb", GET(fold_store_mb), {0, 0, 1, 2, 7, 100, B}, nullptr},
    {"fold_slot_mb", GET(fold_slot_mb), {1, 1, 1, 2, 7, 100, B}, nullptr},
    {"fold_single_pass", GET(fold_single_pass), FLAG, nullptr},
    {"fold_compact", GET(fold_compact), FLAG, nullptr},
    {"trees_per_block", GET(tree_group), {R, 0, 1, 2, 7, 100, R}, "trees_per_block: 0, or 1..256 (4 waves of 64 slots)"},
    {"fold_list_wgs", GET(fold_list_wgs), {0, 0, 1, 2, 7, 100, kFoldListWgsMax}, nullptr},
    {"loss_compact", GET(loss_compact), FLAG, nullptr},
    {"loss_list_groups", GET(loss_list_groups), {0, 0, 1, 2, 7, 100, 1 << 20}, nullptr},
    {"tail_chunk", GET(tail_chunk), {R, 0, 1, 2, R, R, R}, "tail_chunk: 0, or the last chunk's twelfths 1..6"},
    {"exact_early", GET(exact_early), FLAG, nullptr},
    {"fold_cand_est", GET(fold_cand_est), FLAG, nullptr},
    {"fold_cand_est_min", GET(fold_cand_est_min), {1, 1, 1, 2, 7, 100, 1 << 30}, nullptr},
    {"fold_debug_fail", GET(fold_debug_fail), {0, 0, 1, 2, 7, 100, 0}, nullptr},
    {"fold_delta_log2", GET(fold_delta_log2), {1, 1, 1, 2, 7, 40, 40}, nullptr},
    {"fold_seg_max", GET(fold_seg_max), {0, 0, 1, 2, 7, 100, B}, nullptr},
    {"fold_rows_max", GET(fold_rows_max), {0, 0, 1, 2, 7, 100, B}, nullptr},
    {"fold_seg", GET(fold_seg), {-1, 0, 1, 2, 7, 100, B}, nullptr},
    {"exact_w", GET(exact_w), {4, 4, 1, 4, 4, 4, 4}, nullptr},
    {"exact_g", GET(exact_g), {0, 0, 1, 2, 7, 64, 64}, nullptr},
    {"code_cache", GET(code_cache), FLAG, nullptr},
    {"timing", GET(timing), FLAG, nullptr},
    {"stress_probe", GET(stress_probe), FLAG, nullptr},
    {"rows_per_lane", GET(rows_override), RAW, nullptr},
    {"balance", GET(balance_groups), FLAG, nullptr},
    {"debug_hint_regrow", GET(debug_hint_regrow), FLAG, nullptr},
    {"inject_failure_post", GET(inject_post), RAW, nullptr},
    {"inject_failure_post_exact", GET(inject_post_exact), RAW, nullptr},
    {"inject_failure_post_wsum", GET(inject_post_wsum), RAW, nullptr},
    {"inject_failure_post_gather", GET(inject_post_gather), RAW, nullptr},
    {"inject_failure", GET(inject_fail), RAW, nullptr},
};

void check_set() {
  std::set<std::string> expected_names;
  for (const Expect& e : kExpect) {
    expected_names.insert(e.name);
    for (int i = 0; i < kInputs; ++i) {
      SrKnobs k;
      const int64_t before = e.get(k);
      std::string err = "untouched";
      const int rc = sr_knob_set(k, e.name, kIn[i], &err);
      const int64_t after = e.get(k);
      bool ok;
      if (e.out[i] == R)
        ok = rc != 0 && after == before && e.refusal && err == e.refusal;
      else
        ok = rc == 0 && after == e.out[i] && err == "untouched";
      if (!ok) {
        std::fprintf(stderr, "knob_check: %s <- %lld: rc %d, stored %lld (was %lld), message '%s'\n", e.name,
                     (long long)kIn[i], rc, (long long)after, (long long)before, err.c_str());
        ++g_failed;
      }
    }
  }
  {  // the refusing knobs' edges
    SrKnobs k;
    std::string err;
    CHECK(sr_knob_set(k, "trees_per_block", 256, &err) == 0 && k.tree_group == 256);
    CHECK(sr_knob_set(k, "trees_per_block", 257, &err) != 0 && k.tree_group == 256);
    CHECK(err == "trees_per_block: 0, or 1..256 (4 waves of 64 slots)");
    CHECK(sr_knob_set(k, "tail_chunk", kTailTwelfths, &err) == 0 && k.tail_chunk == 6);
    CHECK(sr_knob_set(k, "tail_chunk", 7, &err) != 0 && k.tail_chunk == 6);
    CHECK(err == "tail_chunk: 0, or the last chunk's twelfths 1..6");
    CHECK(sr_knob_set(k, "host_io", 0, &err) == 0 && k.host_io == 0);
    CHECK(sr_knob_set(k, "host_io", 2, &err) != 0 && k.host_io == 0);
    CHECK(err == "host_io must be 0 or 1");
    CHECK(sr_knob_set(k, "host_io", 2, nullptr) != 0);  // (the message is optional)
  }
  // removed and made-up names, and the environment-only knobs, are unknown to sr_set_tuning
  for (const char* name : {"fused_reduce", "exact_list_host", "par_stage", "fold_reduce", "fold_pre_start", "fold_walk_dbg",
                           "no_such_knob", "", "chunks", "waves", "fold_stats", "SR_AMD_PROBE"}) {
    SrKnobs k;
    std::string err;
    CHECK(sr_knob_set(k, name, 1, &err) != 0);
    CHECK(err == std::string("unknown tuning knob '") + name + "'");
  }
  // the table's tuning names are exactly the expected ones, each once
  std::set<std::string> names;
  for (const SrKnobRow& r : kSrKnobs) {
    if (!r.name) continue;
    CHECK(names.insert(r.name).second);
    CHECK(expected_names.count(r.name) == 1);
  }
  CHECK(names.size() == expected_names.size());
}

std::map<std::string, std::string> g_env;
const char* fake_get(const char* name) {
  const auto it = g_env.find(name);
  return it == g_env.end() ? nullptr : it->second.c_str();
}
SrKnobs from_env(std::map<std::string, std::string> env) {
  g_env = std::move(env);
  SrKnobs k;
  sr_knobs_from_env(k, fake_get);
  return k;
}

void check_env() {
  // the variables sr_init reads: these and no others, each once
  const std::set<std::string> expected = {
      "SR_AMD_ROWS_PER_LANE", "SR_AMD_TREES_PER_BLOCK", "SR_AMD_WAVES", "SR_AMD_NO_SORT", "SR_AMD_BALANCE",
      "SR_AMD_NO_HINT", "SR_AMD_CHUNKS", "SR_AMD_PROBE", "SR_AMD_FOLD_SEG", "SR_AMD_HOST_REDUCE",
      "SR_AMD_STRESS_PROBE", "SR_AMD_CODE_CACHE", "SR_AMD_GRAD_ROWS", "SR_AMD_GRAD_SORT", "SR_AMD_VSTK_ROWS",
      "SR_AMD_FIRST_CHUNK", "SR_AMD_CHUNK_MIN", "SR_AMD_HOST_IO", "SR_AMD_EXACT_G", "SR_AMD_EXACT_W", "SR_AMD_DERIVED",
      "SR_AMD_MAX_ROW_BLOCKS", "SR_AMD_REF_FOLD", "SR_AMD_FOLD_STORE_MB", "SR_AMD_FOLD_SLOT_MB", "SR_AMD_FOLD_STATS",
      "SR_AMD_FOLD_DELTA_LOG2", "SR_AMD_FOLD_SEG_MAX", "SR_AMD_FOLD_ROWS_MAX", "SR_AMD_FOLD_SINGLE_PASS",
      "SR_AMD_FOLD_COMPACT", "SR_AMD_FOLD_LIST_WGS", "SR_AMD_LOSS_COMPACT", "SR_AMD_LOSS_LIST_GROUPS",
      "SR_AMD_FOLD_CAND_EST", "SR_AMD_FOLD_CAND_EST_MIN", "SR_AMD_TAIL_CHUNK", "SR_AMD_EXACT_EARLY"};
  std::set<std::string> envs;
  for (const SrKnobRow& r : kSrKnobs) {
    CHECK(r.name || r.env);
    CHECK((r.i32 != nullptr) + (r.i64 != nullptr) + (r.flag != nullptr) == 1);
    CHECK(r.lo <= r.hi);
    if (!r.env) continue;
    CHECK(envs.insert(r.env).second);
    CHECK(expected.count(r.env) == 1);
  }
  CHECK(envs.size() == expected.size());

  {  // nothing set: the defaults (byte for byte: SrKnobs holds plain integers and flags)
    const SrKnobs a = from_env({}), b;
    CHECK(a.tail_chunk == b.tail_chunk && a.host_reduce == b.host_reduce && a.cost_order == b.cost_order &&
          a.dead_hints == b.dead_hints && a.exact_w == b.exact_w && a.tree_group == b.tree_group &&
          a.first_chunk == b.first_chunk && a.fold_seg == b.fold_seg && a.probe == b.probe && a.chunks == b.chunks);
  }
  CHECK(from_env({{"SR_AMD_NO_SORT", "1"}}).cost_order == false);
  CHECK(from_env({{"SR_AMD_NO_SORT", "0"}}).cost_order == true);
  CHECK(from_env({{"SR_AMD_NO_HINT", "1"}}).dead_hints == false);
  CHECK(from_env({{"SR_AMD_NO_HINT", "0"}}).dead_hints == true);
  CHECK(from_env({{"SR_AMD_BALANCE", "0"}}).balance_groups == false);
  CHECK(from_env({{"SR_AMD_BALANCE", "3"}}).balance_groups == true);
  CHECK(from_env({{"SR_AMD_EXACT_W", "2"}}).exact_w == 4);
  CHECK(from_env({{"SR_AMD_EXACT_W", "1"}}).exact_w == 1);
  // the same range as sr_set_tuning, clamped: never refused
  CHECK(from_env({{"SR_AMD_TREES_PER_BLOCK", "1000"}}).tree_group == 256);
  CHECK(from_env({{"SR_AMD_TREES_PER_BLOCK", "-3"}}).tree_group == 0);
  CHECK(from_env({{"SR_AMD_TREES_PER_BLOCK", "64"}}).tree_group == 64);
  CHECK(from_env({{"SR_AMD_FIRST_CHUNK", "1"}}).first_chunk == 2);
  CHECK(from_env({{"SR_AMD_FIRST_CHUNK", "1000"}}).first_chunk == 64);
  CHECK(from_env({{"SR_AMD_MAX_ROW_BLOCKS", "0"}}).max_row_blocks == 1);
  CHECK(from_env({{"SR_AMD_MAX_ROW_BLOCKS", "1000000"}}).max_row_blocks == 65536);
  CHECK(from_env({{"SR_AMD_HOST_IO", "2"}}).host_io == 1);
  CHECK(from_env({{"SR_AMD_HOST_IO", "0"}}).host_io == 0);
  CHECK(from_env({{"SR_AMD_TAIL_CHUNK", "9"}}).tail_chunk == 6);
  CHECK(from_env({{"SR_AMD_EXACT_G", "100"}}).exact_g == 64);
  CHECK(from_env({{"SR_AMD_EXACT_G", "-1"}}).exact_g == 0);
  CHECK(from_env({{"SR_AMD_HOST_REDUCE", "-1"}}).host_reduce == 0);
  CHECK(from_env({{"SR_AMD_FOLD_SEG", "-7"}}).fold_seg == -1);
  CHECK(from_env({{"SR_AMD_FOLD_SEG", "4096"}}).fold_seg == 4096);
  CHECK(from_env({{"SR_AMD_DERIVED", "5"}}).derived == 1);
  CHECK(from_env({{"SR_AMD_STRESS_PROBE", "-2"}}).stress_probe == 1);
  CHECK(from_env({{"SR_AMD_FOLD_LIST_WGS", "99999999999"}}).fold_list_wgs == kFoldListWgsMax);
  CHECK(from_env({{"SR_AMD_FOLD_ROWS_MAX", "1099511627776"}}).fold_rows_max == B);
  // environment-only knobs, stored as given
  CHECK(from_env({{"SR_AMD_CHUNKS", "1"}}).chunks == 1);
  CHECK(from_env({{"SR_AMD_WAVES", "8"}}).waves_override == 8);
  CHECK(from_env({{"SR_AMD_FOLD_STATS", "2"}}).fold_stats == 2);
  CHECK(from_env({{"SR_AMD_PROBE", "0"}}).probe == 0);
  {  // removed variables, and sr_set_tuning-only knobs, change nothing
    const SrKnobs k = from_env({{"SR_AMD_FUSED_REDUCE", "5"}, {"SR_AMD_EXACT_LIST_HOST", "0"}, {"SR_AMD_PAR_STAGE", "0"},
                                {"SR_AMD_TIMING", "0"}, {"SR_AMD_GRAD_LANE_BINS", "0"}, {"SR_AMD_INJECT_FAILURE", "3"}});
    CHECK(k.timing == 1 && k.grad_lane_bins == 1 && k.inject_fail == 0 && k.host_reduce == 8192);
  }
}

}  // namespace

int main() {
  check_defaults();
  check_set();
  check_env();
  if (g_failed) {
    std::fprintf(stderr, "knob_check: %d check(s) failed\n", g_failed);
    return 1;
  }
  std::printf("knob_check: ok\n");
  return 0;
}
