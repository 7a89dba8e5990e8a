// Witness check against an r1cs on the GPU: snarkjs `wtns check <r1cs> <wtns>` and
// circom_tester's checkConstraints for a batch of witnesses (include/nzcb.h nzcb_r1cs_*).
//
// Constraint k of witness w fails iff (A_k . w)(B_k . w) != C_k . w in Fr. The r1cs is parsed
// once (r1cs_reader.h) into a resident object:
//   ptr  : 3 n_constraints + 1 offsets; side s of row k is the terms [ptr[3k+s], ptr[3k+s+1])
//   wire : the term's wire            } structure of arrays, one u32 each per term
//   cid  : the term's coefficient id  }
//   coef : the distinct coefficients, Montgomery form; ids 0 and 1 are +1 and r - 1
// Witness values are in normal form, so coef (Montgomery) x value (normal) is the product in
// normal form after one Montgomery multiplication (the k_additions trick), and terms with
// coefficient +1 or r - 1 are one modular addition or subtraction. Values >= r count modulo r:
// the product absorbs them (one factor < r is enough), the +-1 path reduces them first.
// a b = c is tested as mont(a, b) = mont(c, 1), one more product per side.
//
// Two paths, chosen per row when the object is built:
//   rows with fewer than long_row_threshold terms (A, B and C together): one lane per
//     constraint (k_r1cs_rows); the lanes of a wave own 64 consecutive constraints, so a wave's
//     ballot is one 64-bit word of the witness's bitmap, written with a plain store
//   longer rows (nzcp_live has rows of 836 terms): one wave per constraint (k_r1cs_long_rows),
//     lanes stride over the terms, partial sums are added across the lanes; lane 0 sets the
//     row's bit in the bitmap (the short path wrote a 0 there: it skips long rows)
// Both are templates over a tile of W witnesses per row (a term's wire, id and coefficient
// loaded once, only the witness values gathered per witness; 4, then 2, then 1 for what is
// left of the batch). Measured on nzcp_live, W = 1 (grid y = the witness) is the fastest: the
// structure re-read per witness comes from L2, and the smaller register footprint (69 VGPRs
// against 142) keeps more gathers in flight (profiles/r1cs_check.txt). So W = 1 is what the
// library runs; the larger tiles stay behind nzcb_engine_r1cs_create for that measurement.
// k_r1cs_collect (one workgroup per witness) turns the bitmap into
// n_bad, first_bad and the ascending list, so the list needs no sort and no list cursor.
// The field arithmetic is exact, so the outputs do not depend on the tile, the threshold, the
// batch or the launch geometry, and the host path (device = NZCB_R1CS_HOST: lc_sum and
// row_fails compiled for the host) gives the same bytes.
//
// A call owns its stream (unless the caller passes one) and its device buffers and needs no
// prover context; it may run while a context proves on the same device.
#include <algorithm>
#include <cstring>
#include <map>
#include <vector>

#include "devcall.h"
#include "r1cs_reader.h"
#include "zkey.h"

namespace nzcb {

namespace {

constexpr uint32_t kCoefOne = 0, kCoefMinusOne = 1;
// Rows with at least this many terms take the wave-per-row path. The fastest on MI355X of 8,
// 16, 32, 64, 256 and "no long rows" on nzcp_live at count = 64 (DESIGN.md "Witness check",
// profiles/r1cs_check.txt): 16, 32 and 64 are within 2 % of each other, 8 and 256 are not.
constexpr uint32_t kLongRowThreshold = 16;
constexpr int kWitnessTile = 1;  // witnesses per lane / wave and row (see above)
constexpr unsigned kRowBlock = 256;
constexpr uint32_t kNone = 0xffffffffu;
constexpr size_t kChunkBytes = size_t(256) << 20;  // per-call witness staging / bitmap budget

struct R1csView {
  const uint32_t* ptr;
  const uint32_t* wire;
  const uint32_t* cid;
  const Fr* coef;
  const uint32_t* long_rows;
  uint32_t n_cons, n_long, threshold;
};

// a 32-byte LE witness value; device pointers are 16-byte aligned (checked by the caller)
NZ_HD Fr load_value(const uint8_t* p) {
  Fr v;
#if defined(__HIP_DEVICE_COMPILE__)
  const uint4 lo = reinterpret_cast<const uint4*>(p)[0], hi = reinterpret_cast<const uint4*>(p)[1];
  v.v[0] = lo.x; v.v[1] = lo.y; v.v[2] = lo.z; v.v[3] = lo.w;
  v.v[4] = hi.x; v.v[5] = hi.y; v.v[6] = hi.z; v.v[7] = hi.w;
#else
  memcpy(v.v, p, 32);
#endif
  return v;
}

// any 256-bit value -> [0, r): 2^256 < 6 r, and a top limb below r's means the value is below r
NZ_HD Fr reduce_full(Fr v) {
#pragma unroll 1
  for (int i = 0; i < 5 && v.v[7] >= FrParams::P[7]; i++) v = reduce_once(v);
  return v;
}

// acc[j] += sum over the terms lo, lo + step, ... < hi of coef * witness_j[wire]
template <int W>
NZ_HD void lc_sum(const R1csView& v, uint32_t lo, uint32_t hi, uint32_t step, const uint8_t* const (&wit)[W],
                  Fr (&acc)[W]) {
  for (uint32_t t = lo; t < hi; t += step) {
    const size_t off = size_t(32) * v.wire[t];
    const uint32_t cid = v.cid[t];
    if (cid == kCoefOne) {
#pragma unroll
      for (int j = 0; j < W; j++) acc[j] = acc[j] + reduce_full(load_value(wit[j] + off));
    } else if (cid == kCoefMinusOne) {
#pragma unroll
      for (int j = 0; j < W; j++) acc[j] = acc[j] - reduce_full(load_value(wit[j] + off));
    } else {
      const Fr c = v.coef[cid];
#pragma unroll
      for (int j = 0; j < W; j++) acc[j] = acc[j] + c * load_value(wit[j] + off);
    }
    if (hi - t <= step) break;  // t + step may wrap past 2^32
  }
}

NZ_HD bool row_fails(const Fr& a, const Fr& b, const Fr& c) { return a * b != from_mont(c); }

template <int W>
NZ_HD void zero_all(Fr (&acc)[W]) {
#pragma unroll
  for (int j = 0; j < W; j++) acc[j] = Fr::zero();
}

// One lane per constraint, witnesses [w0 + W blockIdx.y, + W). bitmap: `words` 64-bit words per
// witness, bit k % 64 of word k / 64 = constraint k fails. Grid x covers n_cons exactly.
template <int W>
__global__ __launch_bounds__(kRowBlock) void k_r1cs_rows(R1csView v, const uint8_t* __restrict__ wit, size_t stride,
                                                          uint32_t w0, unsigned long long* __restrict__ bitmap,
                                                          uint32_t words) {
  const uint32_t k = blockIdx.x * kRowBlock + threadIdx.x;
  const uint32_t w = w0 + blockIdx.y * W;
  bool fail[W];
#pragma unroll
  for (int j = 0; j < W; j++) fail[j] = false;
  if (k < v.n_cons) {
    const uint32_t* p = v.ptr + size_t(3) * k;
    const uint32_t p0 = p[0], p1 = p[1], p2 = p[2], p3 = p[3];
    if (p3 - p0 < v.threshold) {
      const uint8_t* wp[W];
#pragma unroll
      for (int j = 0; j < W; j++) wp[j] = wit + stride * (w + j);
      Fr a[W], b[W];
      zero_all(a);
      lc_sum<W>(v, p0, p1, 1, wp, a);
      zero_all(b);
      lc_sum<W>(v, p1, p2, 1, wp, b);
#pragma unroll
      for (int j = 0; j < W; j++) a[j] = a[j] * b[j];
      zero_all(b);
      lc_sum<W>(v, p2, p3, 1, wp, b);
#pragma unroll
      for (int j = 0; j < W; j++) fail[j] = a[j] != from_mont(b[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < W; j++) {
    const unsigned long long m = __ballot(fail[j]);
    if ((threadIdx.x & 63) == 0 && k < v.n_cons) bitmap[size_t(w + j) * words + (k >> 6)] = m;
  }
}

NZ_HD Fr fr_words(const uint32_t (&x)[8]) {
  Fr r;
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = x[i];
  return r;
}

// the sum of `a` over the 64 lanes, in every lane
__device__ __forceinline__ Fr wave_sum(Fr a) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    uint32_t o[8];
#pragma unroll
    for (int i = 0; i < 8; i++) o[i] = (uint32_t)__shfl_xor((int)a.v[i], off, 64);
    a = a + fr_words(o);
  }
  return a;
}

// One wave per long row (long_rows[j], ascending), witnesses as k_r1cs_rows. Runs after
// k_r1cs_rows on the same stream: it ORs the row's bit into the word that kernel stored.
template <int W>
__global__ __launch_bounds__(kRowBlock) void k_r1cs_long_rows(R1csView v, const uint8_t* __restrict__ wit,
                                                               size_t stride, uint32_t w0,
                                                               unsigned long long* __restrict__ bitmap,
                                                               uint32_t words) {
  const uint32_t j0 = blockIdx.x * (kRowBlock / 64) + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63;
  if (j0 >= v.n_long) return;  // the whole wave leaves
  const uint32_t k = v.long_rows[j0];
  const uint32_t w = w0 + blockIdx.y * W;
  const uint32_t* p = v.ptr + size_t(3) * k;
  const uint32_t p0 = p[0], p1 = p[1], p2 = p[2], p3 = p[3];
  const uint8_t* wp[W];
#pragma unroll
  for (int j = 0; j < W; j++) wp[j] = wit + stride * (w + j);
  Fr a[W], b[W];
  zero_all(a);
  if (lane < p1 - p0) lc_sum<W>(v, p0 + lane, p1, 64, wp, a);
  zero_all(b);
  if (lane < p2 - p1) lc_sum<W>(v, p1 + lane, p2, 64, wp, b);
#pragma unroll
  for (int j = 0; j < W; j++) a[j] = wave_sum(a[j]) * wave_sum(b[j]);
  zero_all(b);
  if (lane < p3 - p2) lc_sum<W>(v, p2 + lane, p3, 64, wp, b);
#pragma unroll
  for (int j = 0; j < W; j++) {
    const bool fail = a[j] != from_mont(wave_sum(b[j]));
    if (lane == 0 && fail) atomicOr(&bitmap[size_t(w + j) * words + (k >> 6)], 1ull << (k & 63));
  }
}

// One workgroup per witness: n_bad, first_bad and the lowest min(n_bad, cap) failing indices
// (ascending, the rest 0xffffffff) from the witness's bitmap. cap = 0: bad is not touched.
__global__ __launch_bounds__(kRowBlock) void k_r1cs_collect(const unsigned long long* __restrict__ bitmap,
                                                             uint32_t words, nzcb_r1cs_result* __restrict__ res,
                                                             uint32_t* __restrict__ bad, uint32_t cap) {
  __shared__ uint32_t s_cnt[kRowBlock];
  __shared__ uint32_t s_first;
  const uint32_t tid = threadIdx.x;
  const unsigned long long* bm = bitmap + size_t(blockIdx.x) * words;
  uint32_t* out = bad + size_t(blockIdx.x) * cap;
  uint32_t base = 0;  // failing constraints below this chunk (the same in every thread)
  for (uint32_t c0 = 0; c0 < words; c0 += kRowBlock) {
    const uint32_t idx = c0 + tid;
    unsigned long long m = idx < words ? bm[idx] : 0ull;
    if (!__syncthreads_or(m != 0)) continue;
    const uint32_t n = (uint32_t)__popcll(m);
    s_cnt[tid] = n;
    __syncthreads();
    for (uint32_t d = 1; d < kRowBlock; d <<= 1) {  // inclusive scan
      const uint32_t t = tid >= d ? s_cnt[tid - d] : 0u;
      __syncthreads();
      s_cnt[tid] += t;
      __syncthreads();
    }
    uint32_t pos = base + s_cnt[tid] - n;
    const uint32_t total = s_cnt[kRowBlock - 1];
    if (n && pos == 0) s_first = idx * 64u + (uint32_t)(__ffsll((long long)m) - 1);
    while (m && pos < cap) {
      out[pos++] = idx * 64u + (uint32_t)(__ffsll((long long)m) - 1);
      m &= m - 1;
    }
    base += total;
    __syncthreads();  // s_cnt is rewritten by the next chunk
  }
  for (uint32_t i = base + tid; i < cap; i += kRowBlock) out[i] = kNone;
  __syncthreads();
  if (tid == 0) {
    res[blockIdx.x].n_bad = base;
    res[blockIdx.x].first_bad = base ? s_first : kNone;
  }
}

// kernel milliseconds of the calling thread's last device check: rows, long rows, collect
thread_local double g_times[3] = {0, 0, 0};

}  // namespace

}  // namespace nzcb

using namespace nzcb;

struct nzcb_r1cs {
  uint32_t n_wires = 0, n_out = 0, n_pub_in = 0, n_prv_in = 0, n_cons = 0, n_terms = 0;
  uint32_t threshold = kLongRowThreshold, n_long = 0;
  int tile = kWitnessTile;  // the largest witness tile used: 4 means 4, then 2, then 1 for the rest
  // host path (dev.p is NULL): the arrays; device path: one allocation holding them
  std::vector<uint32_t> ptr, wire, cid, long_rows;
  std::vector<Fr> coef;
  DeviceBlock dev;
  R1csView view{};
};

namespace nzcb {
namespace {

struct FrLess {
  bool operator()(const Fr& a, const Fr& b) const { return std::memcmp(a.v, b.v, 32) < 0; }
};

void build(nzcb_r1cs& r, const uint8_t* d, size_t len, int device, uint32_t threshold, int tile) {
  if (tile != 0 && tile != 1 && tile != 2 && tile != 4) throw Error(NZCB_ERR_ARG, "witness tile must be 0, 1, 2 or 4");
  R1csFile f = r1cs_open(d, len, "r1cs: curve not supported (the prime is not BN254's r)");
  // every constraint takes at least three counts: a header that promises more than the section
  // holds is truncated, before anything is sized by it
  if ((uint64_t)f.n_cons * 12 > f.constraints.left) throw Error(NZCB_ERR_FORMAT, "r1cs: truncated");
  if (f.n_cons >= (1u << 31)) throw Error(NZCB_ERR_FORMAT, "r1cs: too many constraints");
  r.n_wires = f.n_wires;
  r.n_out = f.n_out;
  r.n_pub_in = f.n_pub_in;
  r.n_prv_in = f.n_prv_in;
  r.n_cons = f.n_cons;
  r.threshold = threshold ? threshold : kLongRowThreshold;
  r.tile = tile ? tile : kWitnessTile;
  r.coef = {Fr::one(), neg(Fr::one())};
  std::map<Fr, uint32_t, FrLess> ids{{r.coef[0], kCoefOne}, {r.coef[1], kCoefMinusOne}};
  r.ptr.reserve(size_t(3) * f.n_cons + 1);
  r.ptr.push_back(0);
  uint64_t n_terms = 0;
  for (uint32_t k = 0; k < f.n_cons; k++) {
    const uint64_t row0 = n_terms;
    for (int s = 0; s < 3; s++) {
      r1cs_read_lc(f.constraints, f.n_wires, [&](uint32_t w, const Fr& c) {
        if (++n_terms >> 32) throw Error(NZCB_ERR_FORMAT, "r1cs: 2^32 or more terms");
        uint32_t id = kCoefOne;
        if (c == r.coef[kCoefMinusOne]) {
          id = kCoefMinusOne;
        } else if (c != r.coef[kCoefOne]) {
          auto it = ids.find(c);
          if (it == ids.end()) {
            it = ids.emplace(c, (uint32_t)r.coef.size()).first;
            r.coef.push_back(c);
          }
          id = it->second;
        }
        r.wire.push_back(w);
        r.cid.push_back(id);
      });
      r.ptr.push_back((uint32_t)n_terms);
    }
    if (n_terms - row0 >= r.threshold) r.long_rows.push_back(k);
  }
  r.n_terms = (uint32_t)n_terms;
  r.n_long = (uint32_t)r.long_rows.size();
  r.view = R1csView{r.ptr.data(), r.wire.data(), r.cid.data(), r.coef.data(), r.long_rows.data(),
                    r.n_cons, r.n_long, r.threshold};
  if (device == NZCB_R1CS_HOST) return;
  DeviceScope scope(device);
  BlockLayout lay;
  const size_t o_ptr = lay.take(4 * r.ptr.size()), o_wire = lay.take(4 * r.wire.size()),
               o_cid = lay.take(4 * r.cid.size()), o_coef = lay.take(32 * r.coef.size()),
               o_long = lay.take(4 * r.long_rows.size());
  r.dev.alloc(lay.total);  // never 0: ptr and coef are not empty
  auto put = [&](size_t off, const void* src, size_t bytes) {
    if (bytes) NZ_HIP(hipMemcpy(r.dev.p + off, src, bytes, hipMemcpyHostToDevice));
  };
  put(o_ptr, r.ptr.data(), 4 * r.ptr.size());
  put(o_wire, r.wire.data(), 4 * r.wire.size());
  put(o_cid, r.cid.data(), 4 * r.cid.size());
  put(o_coef, r.coef.data(), 32 * r.coef.size());
  put(o_long, r.long_rows.data(), 4 * r.long_rows.size());
  r.view = R1csView{r.dev.at<uint32_t>(o_ptr), r.dev.at<uint32_t>(o_wire), r.dev.at<uint32_t>(o_cid),
                    r.dev.at<Fr>(o_coef), r.dev.at<uint32_t>(o_long), r.n_cons, r.n_long, r.threshold};
  // the device object keeps no host copy of the matrices
  for (auto* vec : {&r.ptr, &r.wire, &r.cid, &r.long_rows}) std::vector<uint32_t>().swap(*vec);
  std::vector<Fr>().swap(r.coef);
}

void fill_bad(uint32_t* bad, uint32_t from, uint32_t cap) {
  for (uint32_t i = from; i < cap; i++) bad[i] = kNone;
}

void check_host(const nzcb_r1cs& r, const uint8_t* wit, size_t stride, int count, nzcb_r1cs_result* results,
                uint32_t* bad_out, uint32_t cap) {
  const R1csView& v = r.view;
  for (int i = 0; i < count; i++) {
    const uint8_t* const wp[1] = {wit + stride * (size_t)i};
    uint32_t* bad = bad_out ? bad_out + (size_t)cap * i : nullptr;
    nzcb_r1cs_result res{0, kNone};
    for (uint32_t k = 0; k < v.n_cons; k++) {
      const uint32_t* p = v.ptr + size_t(3) * k;
      Fr a[1], b[1], c[1];
      zero_all(a);
      zero_all(b);
      zero_all(c);
      lc_sum<1>(v, p[0], p[1], 1, wp, a);
      lc_sum<1>(v, p[1], p[2], 1, wp, b);
      lc_sum<1>(v, p[2], p[3], 1, wp, c);
      if (!row_fails(a[0], b[0], c[0])) continue;
      if (!res.n_bad) res.first_bad = k;
      if (bad && res.n_bad < cap) bad[res.n_bad] = k;
      res.n_bad++;
    }
    if (bad) fill_bad(bad, std::min(res.n_bad, cap), cap);
    results[i] = res;
  }
}

template <int W>
void launch_tiles(const nzcb_r1cs& r, const uint8_t* wit, size_t stride, uint32_t w0, uint32_t tiles,
                  unsigned long long* bitmap, uint32_t words, hipStream_t st, bool long_rows) {
  if (!long_rows)
    k_r1cs_rows<W><<<dim3((r.n_cons + kRowBlock - 1) / kRowBlock, tiles), kRowBlock, 0, st>>>(r.view, wit, stride, w0,
                                                                                               bitmap, words);
  else
    k_r1cs_long_rows<W><<<dim3((r.n_long + kRowBlock / 64 - 1) / (kRowBlock / 64), tiles), kRowBlock, 0, st>>>(
        r.view, wit, stride, w0, bitmap, words);
}

// every row kernel of a chunk: tiles of r.tile witnesses, then the smaller tiles for the rest
void launch_rows(const nzcb_r1cs& r, const uint8_t* wit, size_t stride, uint32_t count, unsigned long long* bitmap,
                 uint32_t words, hipStream_t st, bool long_rows) {
  uint32_t w0 = 0;
  for (int W = r.tile; W >= 1; W >>= 1) {
    const uint32_t tiles = (count - w0) / (uint32_t)W;
    if (!tiles) continue;
    if (W == 4) launch_tiles<4>(r, wit, stride, w0, tiles, bitmap, words, st, long_rows);
    if (W == 2) launch_tiles<2>(r, wit, stride, w0, tiles, bitmap, words, st, long_rows);
    if (W == 1) launch_tiles<1>(r, wit, stride, w0, tiles, bitmap, words, st, long_rows);
    w0 += tiles * (uint32_t)W;
  }
}

void check_device(const nzcb_r1cs& r, const uint8_t* wit, size_t stride, bool on_device, int count,
                  nzcb_r1cs_result* results, uint32_t* bad_out, uint32_t cap, void* stream) {
  for (auto& t : g_times) t = 0;
  const uint32_t dcap = std::min(cap, r.n_cons);  // no list is longer than the constraints
  if (!r.n_cons) {
    for (int i = 0; i < count; i++) {
      results[i] = nzcb_r1cs_result{0, kNone};
      if (bad_out) fill_bad(bad_out + (size_t)cap * i, 0, cap);
    }
    return;
  }
  CallScope cs(r.dev.device, stream, 4);
  const uint32_t words = (r.n_cons + 63) / 64;
  const size_t wbytes = size_t(32) * r.n_wires;
  // witnesses per pass: the bitmap, the lists and (host witnesses) the staging buffer within the
  // budget; a tile count must fit grid.y
  size_t per = size_t(8) * words + size_t(4) * dcap + (on_device ? 0 : wbytes);
  const uint32_t chunk = (uint32_t)std::min<size_t>({(size_t)count, std::max<size_t>(1, kChunkBytes / per), 65532});
  auto* d_bitmap = cs.alloc<unsigned long long>(size_t(8) * words * chunk);
  auto* d_res = cs.alloc<nzcb_r1cs_result>(sizeof(nzcb_r1cs_result) * chunk);
  uint32_t* d_bad = cs.alloc<uint32_t>(size_t(4) * dcap * chunk);
  uint8_t* d_wit = on_device ? nullptr : cs.alloc<uint8_t>(wbytes * chunk);
  std::vector<uint32_t> lists(bad_out && dcap < cap ? size_t(dcap) * chunk : 0);
  for (uint32_t done = 0; done < (uint32_t)count; done += chunk) {
    const uint32_t n = std::min(chunk, (uint32_t)count - done);
    const uint8_t* src = wit + stride * done;
    size_t src_stride = stride;
    if (!on_device) {
      if (stride == wbytes) {
        NZ_HIP(hipMemcpyAsync(d_wit, src, wbytes * n, hipMemcpyHostToDevice, cs.st));
      } else {
        for (uint32_t i = 0; i < n; i++)
          NZ_HIP(hipMemcpyAsync(d_wit + wbytes * i, src + stride * i, wbytes, hipMemcpyHostToDevice, cs.st));
      }
      src = d_wit;
      src_stride = wbytes;
    }
    cs.record(0);
    launch_rows(r, src, src_stride, n, d_bitmap, words, cs.st, false);
    cs.record(1);
    if (r.n_long) launch_rows(r, src, src_stride, n, d_bitmap, words, cs.st, true);
    cs.record(2);
    k_r1cs_collect<<<n, kRowBlock, 0, cs.st>>>(d_bitmap, words, d_res, d_bad, bad_out ? dcap : 0u);
    cs.record(3);
    NZ_HIP(hipGetLastError());
    NZ_HIP(hipMemcpyAsync(results + done, d_res, sizeof(nzcb_r1cs_result) * n, hipMemcpyDeviceToHost, cs.st));
    if (bad_out && dcap) {
      uint32_t* dst = dcap == cap ? bad_out + (size_t)cap * done : lists.data();
      NZ_HIP(hipMemcpyAsync(dst, d_bad, size_t(4) * dcap * n, hipMemcpyDeviceToHost, cs.st));
    }
    NZ_HIP(hipStreamSynchronize(cs.st));
    if (bad_out && dcap < cap)
      for (uint32_t i = 0; i < n; i++) {
        uint32_t* row = bad_out + (size_t)cap * (done + i);
        std::memcpy(row, lists.data() + size_t(dcap) * i, size_t(4) * dcap);
        fill_bad(row, dcap, cap);
      }
    for (int e = 0; e < 3; e++) g_times[e] += cs.elapsed(e, e + 1);
  }
}

void check(nzcb_r1cs* r, const void* witness, size_t n, int kind, int count, size_t stride,
           nzcb_r1cs_result* results, uint32_t* bad_out, uint32_t cap, void* stream) {
  if (!r || count < 0) throw Error(NZCB_ERR_ARG, "bad argument");
  if (kind != NZCB_WITNESS_WTNS && kind != NZCB_WITNESS_HOST && kind != NZCB_WITNESS_DEVICE)
    throw Error(NZCB_ERR_ARG, "unknown witness kind");
  if (!count) return;
  if (!witness || !results) throw Error(NZCB_ERR_ARG, "null argument");
  const uint8_t* values = static_cast<const uint8_t*>(witness);
  if (kind == NZCB_WITNESS_WTNS) {
    if (count != 1) throw Error(NZCB_ERR_ARG, "a wtns file holds one witness");
    const Wtns w = parse_wtns(values, n);
    if (!w.q_is_r) throw Error(NZCB_ERR_CURVE, "Curve of the witness does not match the curve of the r1cs");
    values = w.values;
    n = w.nWitness;
  }
  if (n != r->n_wires)
    throw Error(NZCB_ERR_WITNESS_LEN, "Invalid witness length. Circuit: " + std::to_string(r->n_wires) +
                                          ", witness: " + std::to_string(n));
  const size_t wbytes = size_t(32) * r->n_wires;
  if (kind == NZCB_WITNESS_WTNS || (count == 1 && stride == 0)) stride = wbytes;
  if (stride < wbytes) throw Error(NZCB_ERR_ARG, "witness stride is shorter than a witness");
  if (!bad_out) cap = 0;
  const bool on_device = kind == NZCB_WITNESS_DEVICE;
  if (!r->dev.p) {
    if (on_device) throw Error(NZCB_ERR_ARG, "a host r1cs object cannot read device witnesses");
    check_host(*r, values, stride, count, results, bad_out, cap);
    return;
  }
  if (on_device && ((reinterpret_cast<uintptr_t>(values) | stride) & 15))
    throw Error(NZCB_ERR_ARG, "device witnesses and their stride must be 16-byte aligned");
  check_device(*r, values, stride, on_device, count, results, bad_out, cap, stream);
}

nzcb_r1cs* create(const uint8_t* d, size_t len, int device, uint32_t threshold, int tile, nzcb_err* err) {
  return guarded_new<nzcb_r1cs>(err, [&] {
    if (!d) throw Error(NZCB_ERR_ARG, "null argument");
    auto r = std::make_unique<nzcb_r1cs>();
    build(*r, d, len, device, threshold, tile);
    return r;
  });
}

}  // namespace
}  // namespace nzcb

extern "C" {

nzcb_r1cs* nzcb_engine_r1cs_create(const uint8_t* r1cs, size_t len, int device, uint32_t long_row_threshold,
                                   int witness_tile, nzcb_err* err) {
  return create(r1cs, len, device, long_row_threshold, witness_tile, err);
}

nzcb_r1cs* nzcb_r1cs_create(const uint8_t* r1cs, size_t len, int device, nzcb_err* err) {
  return create(r1cs, len, device, 0, 0, err);
}

nzcb_r1cs* nzcb_r1cs_create_file(const char* path, int device, nzcb_err* err) {
  return guarded_new<nzcb_r1cs>(err, [&] {
    if (!path) throw Error(NZCB_ERR_ARG, "null r1cs path");
    const MappedFile f(path, "the r1cs", "r1cs: invalid file format");
    auto r = std::make_unique<nzcb_r1cs>();
    build(*r, f.data, f.size, device, 0, 0);
    return r;
  });
}

int nzcb_r1cs_info(const nzcb_r1cs* r, uint32_t info[8]) {
  if (!r || !info) return NZCB_ERR_ARG;
  info[0] = r->n_wires;
  info[1] = r->n_out;
  info[2] = r->n_pub_in;
  info[3] = r->n_prv_in;
  info[4] = r->n_cons;
  info[5] = r->n_terms;
  info[6] = r->threshold;
  info[7] = r->n_long;
  return 0;
}

int nzcb_r1cs_check(nzcb_r1cs* r, const void* witness, size_t n, int kind, int count, size_t witness_stride,
                    nzcb_r1cs_result* results, uint32_t* bad_out, uint32_t bad_cap, void* stream, nzcb_err* err) {
  return guarded(err, [&] {
    check(r, witness, n, kind, count, witness_stride, results, bad_out, bad_cap, stream);
  });
}

int nzcb_debug_r1cs_check_timings(double* ms, int cap) {
  int k = 0;
  for (; ms && k < cap && k < 3; k++) ms[k] = g_times[k];
  return k;
}

void nzcb_r1cs_destroy(nzcb_r1cs* r) { delete r; }

}  // extern "C"
