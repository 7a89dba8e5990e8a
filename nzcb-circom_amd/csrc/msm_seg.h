// Sizes and bounds of the segment plan of the dense fixed-base accumulation (msm.hip
// msm_seg_*_kernel, msm_accumulate29_seg_kernel). Plain C++: tests/native/msm_seg_host.cpp
// checks them on the CPU against a brute-force plan.
#pragma once
#include <cstddef>
#include <cstdint>

namespace nzcb {

// Longest segment. At c = 20 a bucket holds ~52 entries and the top window's 15 bits put
// another 128 into each of the first 2^14 buckets (~180, at most ~240 at 2^21 scalars): 256
// keeps every bucket of random scalars whole, so the finalize finds nothing to add. At most
// 256: the plan's counting sort scans the length classes with one 256-thread workgroup.
#ifndef NZ_SEG_MAX
#define NZ_SEG_MAX 256
#endif
constexpr uint32_t kSegMax = NZ_SEG_MAX;
static_assert(kSegMax >= 4 && kSegMax <= 256, "segment cap: 4..256");

// buckets per wave of the plan's histogram and scatter kernels (a tile of the counting sort):
// 1024 waves of 8 steps at 2^19 buckets. The plan of an isolated 2^21 MSM took 75 us with tiles
// of 2048, 47 us with 1024 and 37 us with 512 (profiles/acc_segments_probe.txt).
#ifndef NZ_SEG_TILE
#define NZ_SEG_TILE 512
#endif
constexpr uint32_t kSegTile = NZ_SEG_TILE;
static_assert(kSegTile % 64 == 0, "whole waves of buckets");

// A bucket of len entries: len / kSegMax whole segments, then the rest.
constexpr uint32_t seg_count(uint32_t len, uint32_t cap = kSegMax) { return (len + cap - 1) / cap; }

// Segments of any bucketing of `entries` entries into at most `nkeys` buckets: every bucket has
// at most one segment shorter than the cap, and the whole ones hold cap entries each.
constexpr size_t seg_bound(size_t entries, size_t nkeys, size_t cap = kSegMax) { return entries / cap + nkeys; }

// Whole (cap-entry) segments: they index the carries of the buckets cut into pieces.
constexpr size_t seg_whole_bound(size_t entries, size_t cap = kSegMax) { return entries / cap; }

// Buckets with more than one segment (each holds more than cap entries).
constexpr size_t seg_multi_bound(size_t entries, size_t nkeys, size_t cap = kSegMax) {
  return entries / (cap + 1) < nkeys ? entries / (cap + 1) : nkeys;
}

// Carries of all the buckets cut into pieces: their whole segments and one rest each.
constexpr size_t seg_carry_bound(size_t entries, size_t nkeys, size_t cap = kSegMax) {
  return seg_whole_bound(entries, cap) + seg_multi_bound(entries, nkeys, cap);
}

// tiles of the plan's counting sort, and its (length class, tile) counters
constexpr size_t seg_tiles(size_t nkeys) { return (nkeys + kSegTile - 1) / kSegTile; }
constexpr size_t seg_counters(size_t nkeys, size_t cap = kSegMax) { return cap * seg_tiles(nkeys) + 256; }

}  // namespace nzcb
