// cvr_wpool_select.h - which k_wpool instance (cvr_wpool.hip) a wave-pool launch runs: the one
// statement of the rule.  Plain C++17, no HIP (tests/cpp/wpool_select.cpp, tests/test_wpool_select.py).
#pragma once

namespace cvr {
// kMed: the medium layout an instance is compiled for (kMedDense any dense medium, its cells,
// bounds, uniform albedo and storage format read at run time; kMedSparse leaves + brick words;
// kMedDenseFull a dense medium with density cells and brick bounds; kMedDenseFullUniform the
// same with a uniform albedo, MediumParams::albedo_uniform).
enum : int { kMedDense = 0, kMedSparse = 1, kMedDenseFull = 2, kMedDenseFullUniform = 3 };
// Or-ed into kMed (k_wpool's kMedMk):
constexpr int kMedMK = 4;        // naiveMK's walk: d_init, every segment re-seeded as d_extend does (Q12)
constexpr int kMedCount = 8;     // CVR_OPT_COUNT_WORDS, sparse only: also counts the brick words loaded
constexpr int kMedHalf = 16;     // the half format pinned, as albedo_uniform is; kMedDense reads it at run time
constexpr int kMedMoments = 32;  // CVR_OPT_MOMENTS: an escape adds its squares and a count behind the tile
constexpr int kMedEnv = 64;      // cvr_set_environment: an escape's T is multiplied by the map's radiance in its direction
// Waves per SIMD of every feature instance, the default budget; CVR_OPT_WAVES 3, 4, 6: generic layouts only.
constexpr int kWpoolWaves = 5;
// What a launch asks of the kernel.
struct WpoolRequest {
  bool scatter_eps;
  int waves;  // CVR_OPT_WAVES: 3, 4, 5 or 6
  bool sparse, full, uniform;  // leaves + brick words; dense with cells and bounds, its albedo uniform
  bool half, naive_mk, count_words, moments;
  bool record, flush;  // cvr_trace_launch; cvr_render_frame's in-launch output
  bool env;            // an environment map is set (last, so that shorter initialisers leave it false)
};
struct WpoolInstance { bool eps; int waves, med; bool record, flush; };  // k_wpool's template arguments
constexpr bool operator==(const WpoolInstance& a, const WpoolInstance& b) {
  return a.eps == b.eps && a.waves == b.waves && a.med == b.med && a.record == b.record && a.flush == b.flush;
}

// The instance that runs request q, or false: no instance runs it.
constexpr bool wpool_select(const WpoolRequest& q, WpoolInstance* out) {
  const bool w5 = q.waves == kWpoolWaves;
  // 1. refusals.  Moments: no records, in-launch output, naiveMK walk, word counts or sparse half medium
  if (q.moments && (q.naive_mk || q.count_words || q.record || q.flush || (q.sparse && q.half))) return false;
  if (!w5 && (q.flush || q.half || q.naive_mk || q.moments)) return false;
  if (q.record + q.flush + q.naive_mk > 1 || (q.half && q.count_words)) return false;
  if (q.record && !w5 && !(q.sparse && q.waves == 4)) return false;  // record budgets: 5, sparse also 4
  // Environment: the default budget, no naiveMK walk, word counts, records or in-launch output
  if (q.env && (!w5 || q.naive_mk || q.count_words || q.record || q.flush)) return false;
  // 2. degradation.  Records, moments, an environment and the other budgets take the generic layout (dense: the format is read at
  // run time), a sparse medium's other budgets its 4-wave instance; word counts are dropped where none counts
  const bool generic = q.record || q.moments || q.env || !w5;
  const int layout = q.sparse            ? kMedSparse
                     : generic || !q.full ? kMedDense
                     : q.uniform          ? kMedDenseFullUniform
                                          : kMedDenseFull;
  const bool count = q.count_words && q.sparse && w5 && !q.record && !q.flush && !q.naive_mk;
  // 3. the result (naiveMK: scatter -eps always)
  const int waves = w5 ? kWpoolWaves : q.sparse ? 4 : (q.waves == 6 || q.waves == 3) ? q.waves : 4;
  const int med = layout | (q.half && layout != kMedDense ? kMedHalf : 0) | (q.naive_mk ? kMedMK : 0) |
                  (count ? kMedCount : 0) | (q.moments ? kMedMoments : 0) | (q.env ? kMedEnv : 0);
  *out = {q.scatter_eps || q.naive_mk, waves, med, q.record, q.flush};
  return true;
}

// Request i of the whole space, for the sweeps (cvr_wpool.hip's static_assert, tests/cpp/wpool_select.cpp):
// 2 scatter modes x 4 budgets x 4 layouts (sparse, dense, full, full + uniform) x 2^6 features.
// The upper half of kWpoolRequestsAll is the same space with an environment set.
constexpr int kWpoolRequests = 2 * 4 * 4 * 64, kWpoolRequestsAll = 2 * kWpoolRequests;
constexpr WpoolRequest wpool_request_at(int i) {
  const int layout = i >> 6 & 3;
  return {(i >> 10 & 1) != 0, 3 + (i >> 8 & 3), layout == 0, layout >= 2, layout == 3,
          (i & 32) != 0, (i & 16) != 0, (i & 8) != 0, (i & 4) != 0, (i & 2) != 0, (i & 1) != 0,
          (i >> 11 & 1) != 0};
}

}  // namespace cvr
