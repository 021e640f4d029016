// cvr_regen_plan.h - bookkeeping of one regeneration burst of the wave pool (k_wpool's
// regeneration phase, cvr_wpool.hip).  Plain C++, no HIP: the kernel calls these functions
// on wave-uniform values, and tests/cpp/regen_plan.cpp sweeps them on the host.
//
// A burst makes the next `width` consecutive units of the wave's chunk, one per lane, and
// tests each camera ray against the box.  `hits` has bit l set iff lane l's path hits.  A
// hit needs a free pool slot; a miss ends at once and needs none.  With `free` slots:
//   * the first min(popcount(hits), free) hits are accepted, hit number r (in lane order)
//     into free-stack entry free - 1 - r;
//   * if every hit is accepted the whole burst is committed; otherwise the burst commits
//     exactly the units before the first rejected hit, and the cursor goes back to that
//     unit: nothing from it on has had a side effect, and a later burst makes it again.
// So no unit is committed twice or skipped, whatever the mask.
#pragma once
#include <cstdint>

namespace cvr {

constexpr uint32_t kRegenLanes = 64;

struct RegenBurst {
  uint32_t accepted;   // hits that take a slot: lanes below `committed` whose bit is set
  uint32_t committed;  // units [cursor, cursor + committed) are done; the new cursor is their end
};

// Lanes of a burst: over * free (some paths will miss: more are made than there are slots), at
// most a wave, at most what is left of the chunk.  0 only when free or remaining is 0.
constexpr uint32_t regen_width(uint32_t free, uint32_t remaining, uint32_t over) {
  const uint32_t want = free > kRegenLanes / over ? kRegenLanes : free * over;  // (no overflow)
  const uint32_t w = want < kRegenLanes ? want : kRegenLanes;
  return w < remaining ? w : remaining;
}

constexpr uint32_t regen_popcount(uint64_t m) { return (uint32_t)__builtin_popcountll(m); }

// Index of the n-th (0-based) set bit of m; popcount(m) > n.  Six halvings, each one popcount.
constexpr uint32_t regen_nth_set(uint64_t m, uint32_t n) {
  uint32_t pos = 0;
  for (uint32_t w = 32; w != 0; w >>= 1) {
    const uint32_t c = regen_popcount((m >> pos) & ((1ull << w) - 1ull));
    if (n >= c) {
      n -= c;
      pos += w;
    }
  }
  return pos;
}

// width <= 64; bits of hits at or above width are ignored.
constexpr RegenBurst regen_plan(uint64_t hits, uint32_t width, uint32_t free) {
  const uint64_t h = width >= kRegenLanes ? hits : hits & ((1ull << width) - 1ull);
  const uint32_t n = regen_popcount(h);
  if (n <= free) return RegenBurst{n, width};
  return RegenBurst{free, regen_nth_set(h, free)};  // the first rejected hit is hit number `free`
}

// ---- a sweep at compile time: every (free, width, mask) of widths <= 6 -----------------
// (tests/cpp/regen_plan.cpp goes on to width 8, random 64-wide masks and chained bursts)
constexpr bool regen_plan_holds(uint64_t hits, uint32_t width, uint32_t free) {
  const RegenBurst b = regen_plan(hits, width, free);
  if (b.accepted > free || b.committed > width) return false;
  if (width != 0 && free != 0 && b.committed == 0) return false;  // a burst with a free slot commits its first unit
  uint32_t in = 0;  // hits among the committed units: all of them accepted, and no other
  for (uint32_t l = 0; l < b.committed; ++l) in += (uint32_t)((hits >> l) & 1ull);
  if (in != b.accepted) return false;
  // cut short only in front of a hit that found no slot
  if (b.committed < width && !(((hits >> b.committed) & 1ull) && b.accepted == free)) return false;
  return true;
}
constexpr bool regen_plan_sweep() {
  for (uint32_t width = 0; width <= 6; ++width)
    for (uint32_t free = 0; free <= 7; ++free)
      for (uint64_t m = 0; m < (1ull << width); ++m)
        if (!regen_plan_holds(m, width, free)) return false;
  return regen_plan_holds(~0ull, 64, 64) && regen_plan_holds(~0ull, 64, 1) && regen_plan_holds(1ull << 63, 64, 0) &&
         regen_nth_set(1ull << 63, 0) == 63 && regen_nth_set(~0ull, 37) == 37;
}
static_assert(regen_plan_sweep(), "regen_plan: a burst's accepted hits and committed units disagree");
static_assert(regen_width(1, 256, 2) == 2 && regen_width(40, 256, 2) == 64 && regen_width(115, 3, 2) == 3 &&
                  regen_width(0, 9, 2) == 0 && regen_width(5, 0, 2) == 0 && regen_width(3, 256, 64) == 64,
              "regen_width");

}  // namespace cvr
