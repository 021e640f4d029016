// Host check of the regeneration burst's bookkeeping (csrc/cvr_regen_plan.h; no HIP): the
// functions k_wpool's regeneration phase calls, against a unit-by-unit model.
//   1. every (free, remaining, over, hit mask) whose burst is at most 8 wide;
//   2. random 64-wide masks at every free count;
//   3. chained bursts over a chunked stream of units with a fixed hit pattern, the free slots
//      refilled at random between bursts: every unit is committed once, in order, and a
//      committed hit always has a slot.
// Prints one summary line and exits 0, or names the first failing case and exits 1.
// (tests/test_regen_plan.py; `make regen-plan-asan` builds and runs it with ASan and UBSan.)
#include <cstdint>
#include <cstdio>
#include <vector>

#include "cvr_regen_plan.h"

using namespace cvr;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// The burst, one unit at a time: units are committed in lane order until a hit finds no slot.
static RegenBurst model(uint64_t hits, uint32_t width, uint32_t free) {
  RegenBurst b{0, 0};
  for (uint32_t l = 0; l < width; ++l) {
    if ((hits >> l) & 1ull) {
      if (b.accepted == free) break;
      ++b.accepted;
    }
    ++b.committed;
  }
  return b;
}

static int check(uint64_t hits, uint32_t width, uint32_t free, const char* what) {
  const RegenBurst got = regen_plan(hits, width, free), want = model(hits, width, free);
  const bool inv = got.accepted <= free && got.committed <= width && (width == 0 || free == 0 || got.committed >= 1);
  if (got.accepted != want.accepted || got.committed != want.committed || !inv || !regen_plan_holds(hits, width, free)) {
    std::printf("FAIL %s: hits %016llx width %u free %u -> accepted %u committed %u (model %u %u)\n", what,
                (unsigned long long)hits, width, free, got.accepted, got.committed, want.accepted, want.committed);
    return 1;
  }
  return 0;
}

int main() {
  unsigned long long cases = 0;
  // 1. small widths, exhaustively, through regen_width
  for (uint32_t over = 1; over <= 3; ++over)
    for (uint32_t free = 0; free <= 9; ++free)
      for (uint32_t remaining = 0; remaining <= 9; ++remaining) {
        const uint32_t w = regen_width(free, remaining, over);
        const uint32_t want_w = free * over < remaining ? free * over : remaining;  // (all below 64 here)
        if (w != want_w) {
          std::printf("FAIL width: free %u remaining %u over %u -> %u (want %u)\n", free, remaining, over, w, want_w);
          return 1;
        }
        if (w > 8) continue;
        for (uint64_t m = 0; m < (1ull << w); ++m, ++cases)
          if (check(m, w, free, "small")) return 1;
      }
  // every mask of every width <= 8 at every free count, whatever width regen_width would choose
  for (uint32_t w = 0; w <= 8; ++w)
    for (uint32_t free = 0; free <= 9; ++free)
      for (uint64_t m = 0; m < (1ull << w); ++m, ++cases)
        if (check(m, w, free, "width<=8")) return 1;
  // the width's clamps
  for (uint32_t free = 0; free <= 300; ++free)
    for (uint32_t remaining : {0u, 1u, 63u, 64u, 65u, 256u, 0xFFFFFFFFu})
      for (uint32_t over : {1u, 2u, 3u, 64u}) {
        const uint64_t want = (uint64_t)free * over;
        const uint64_t w = want < 64 ? want : 64;
        if (regen_width(free, remaining, over) != (uint32_t)(w < remaining ? w : remaining)) {
          std::printf("FAIL width clamp: free %u remaining %u over %u\n", free, remaining, over);
          return 1;
        }
      }
  // 2. random wide masks: dense, sparse and plain random, with stray bits above the width
  for (int i = 0; i < 200000; ++i, ++cases) {
    uint64_t m = rnd();
    if (i % 3 == 1) m &= rnd();
    if (i % 3 == 2) m |= rnd();
    const uint32_t w = i % 5 == 0 ? (uint32_t)(rnd() % 65) : 64u;
    const uint32_t free = (uint32_t)(rnd() % 130);
    const uint64_t in = w >= 64 ? m : m & ((1ull << w) - 1ull);
    const RegenBurst a = regen_plan(m, w, free), b = regen_plan(in, w, free);
    if (a.accepted != b.accepted || a.committed != b.committed) {
      std::printf("FAIL stray bits: hits %016llx width %u free %u\n", (unsigned long long)m, w, free);
      return 1;
    }
    if (check(in, w, free, "random")) return 1;
  }
  // 3. chained bursts: a stream of units in chunks, a hit pattern fixed per unit
  for (int trial = 0; trial < 300; ++trial) {
    const uint32_t n_units = 1 + (uint32_t)(rnd() % 3000), chunk = 1 + (uint32_t)(rnd() % 300);
    const uint32_t over = 1 + (uint32_t)(rnd() % 3), slots = 1 + (uint32_t)(rnd() % 122);
    const uint32_t hit_pct = (uint32_t)(rnd() % 101);
    std::vector<uint8_t> hit(n_units), done(n_units, 0);
    for (auto& h : hit) h = rnd() % 100 < hit_pct;
    uint32_t cursor = 0, free = slots, bursts = 0;
    while (cursor < n_units) {
      if (free == 0) {  // (paths end elsewhere and free their slots)
        free = 1 + (uint32_t)(rnd() % slots);
        continue;
      }
      const uint32_t cend = (cursor / chunk + 1) * chunk < n_units ? (cursor / chunk + 1) * chunk : n_units;
      const uint32_t w = regen_width(free, cend - cursor, over);
      uint64_t m = 0;
      for (uint32_t l = 0; l < w; ++l) m |= (uint64_t)hit[cursor + l] << l;
      const RegenBurst b = regen_plan(m, w, free);
      if (b.committed == 0 || b.accepted > free) {
        std::printf("FAIL chain: no progress or too many hits at unit %u (width %u free %u)\n", cursor, w, free);
        return 1;
      }
      uint32_t acc = 0;
      for (uint32_t l = 0; l < b.committed; ++l) {
        if (done[cursor + l]++) {
          std::printf("FAIL chain: unit %u committed twice\n", cursor + l);
          return 1;
        }
        acc += hit[cursor + l];
      }
      if (acc != b.accepted) {
        std::printf("FAIL chain: %u hits committed, %u accepted at unit %u\n", acc, b.accepted, cursor);
        return 1;
      }
      cursor += b.committed;
      free -= b.accepted;
      if (rnd() % 4 == 0) free += (uint32_t)(rnd() % (slots - free + 1));
      ++bursts;
      ++cases;
    }
    for (uint32_t u = 0; u < n_units; ++u)
      if (done[u] != 1) {
        std::printf("FAIL chain: unit %u committed %u times\n", u, done[u]);
        return 1;
      }
  }
  std::printf("regen_plan ok: %llu cases\n", cases);
  return 0;
}
