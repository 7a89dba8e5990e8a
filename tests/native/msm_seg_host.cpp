// csrc/msm_seg.h's bounds against brute-force segment plans: every way of sizing up to four
// buckets with small counts and caps, then random bucketings at the sizes the prover runs.
// Prints "ok <plans checked>" or the first bound a plan exceeds.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../nzcb-circom_amd/csrc/msm_seg.h"

using namespace nzcb;

static size_t checked = 0;

static void check(const std::vector<uint32_t>& sizes, size_t cap) {
  size_t entries = 0, segs = 0, whole = 0, multi = 0, carries = 0, pieces = 0, longest = 0;
  for (uint32_t len : sizes) {
    const size_t w = len / cap, r = len % cap, n = w + (r ? 1 : 0);
    entries += len;
    segs += n;
    whole += w;
    if (n != seg_count(len, (uint32_t)cap)) {
      printf("seg_count(%u, %zu) = %u, plan has %zu\n", len, cap, seg_count(len, (uint32_t)cap), n);
      exit(1);
    }
    if (n > 1) {
      multi++;
      carries += n;
      pieces += (n + 255) / 256;  // msm.hip kPieceCarries
    }
    if (r > longest) longest = r;
    if (w && cap > longest) longest = cap;
  }
  const size_t nkeys = sizes.size();
  auto need = [&](const char* what, size_t got, size_t bound) {
    if (got > bound) {
      printf("%s: %zu > bound %zu (entries %zu, keys %zu, cap %zu)\n", what, got, bound, entries, nkeys, cap);
      exit(1);
    }
  };
  need("segments", segs, seg_bound(entries, nkeys, cap));
  need("whole segments", whole, seg_whole_bound(entries, cap));
  need("cut buckets", multi, seg_multi_bound(entries, nkeys, cap));
  need("carries", carries, seg_carry_bound(entries, nkeys, cap));
  // MsmScratch::init's piece array: carries / 256 + cut buckets
  need("pieces", pieces, seg_carry_bound(entries, nkeys, cap) / 256 + seg_multi_bound(entries, nkeys, cap));
  need("longest segment", longest, cap);
  checked++;
}

int main() {
  // exhaustive: up to 4 buckets of 0..13 entries, caps 4..6
  for (size_t cap = 4; cap <= 6; cap++)
    for (uint32_t nk = 1; nk <= 4; nk++) {
      std::vector<uint32_t> sizes(nk, 0);
      for (;;) {
        check(sizes, cap);
        uint32_t i = 0;
        while (i < nk && ++sizes[i] > 13) sizes[i++] = 0;
        if (i == nk) break;
      }
    }
  // random bucketings: uniform, one heavy bucket, all in one bucket, at the caps measured
  std::mt19937_64 rng(12345);
  for (size_t cap : {(size_t)64, (size_t)kSegMax})
    for (int rep = 0; rep < 60; rep++) {
      const size_t nkeys = (size_t)1 << (9 + rep % 8);
      const size_t entries = rng() % (nkeys * 200) + 1;
      std::vector<uint32_t> sizes(nkeys, 0);
      const int kind = rep % 3;
      for (size_t e = 0; e < entries; e++) {
        size_t k = rng() % nkeys;
        if (kind == 1 && (rng() & 1)) k = 7;
        if (kind == 2) k = nkeys - 1;
        sizes[k]++;
      }
      check(sizes, cap);
    }
  // the counting sort's tiles and counters
  if (seg_tiles(1) != 1 || seg_tiles(kSegTile) != 1 || seg_tiles(kSegTile + 1) != 2 ||
      seg_counters((size_t)1 << 19) != kSegMax * (((size_t)1 << 19) / kSegTile) + 256) {
    printf("seg_tiles / seg_counters\n");
    return 1;
  }
  printf("ok %zu\n", checked);
  return 0;
}
