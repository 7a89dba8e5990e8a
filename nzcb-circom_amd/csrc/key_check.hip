// Key material check: powers-of-tau files and PLONK zkeys examined on the GPU before use
// (include/nzcb.h nzcb_ptau_check, nzcb_zkey_check).
//
// The SRS check (srs_check): one curve test per point (k_srs_points), then the pairing equation
// of the whole sequence under random 128-bit weights rho_i,
//   e(-sum rho_i P_i, T) * e(sum rho_i P_(i+1), [1]_2) = 1,
// whose two sums are generic MSMs (msm.h) over the same weights (k_srs_weights), the second
// over the base array moved by one point. The points pass through the device in chunks that
// overlap by one point, so the pair that straddles two chunks is covered and HBM use does not
// grow with the file. A failing equation is bisected over index ranges with sub-sums of the
// same terms.
//
// The zkey check adds, per polynomial of the key, the canonical-value test and the comparison
// of the stored evaluations with the transform of the stored coefficients (k_fr_compare after
// ntt.h's transform), and the commitment in the header against an MSM over the key's own PTau.
//
// Both run the same driver over a backend: the device one here, or the host one (NZCB_KEY_HOST),
// which calls the same NZ_HD functions of key_check.h and gives the same findings and sums.
// A call owns its stream and buffers (devcall.h CallScope) and needs no prover context.
#include <sys/random.h>

#include <algorithm>
#include <cerrno>
#include <chrono>
#include <cstring>
#include <memory>
#include <vector>

#include "devcall.h"
#include "key_check.h"
#include "msm.h"
#include "ntt.h"
#include "verify.h"
#include "zkey.h"

namespace nzcb {

namespace {

constexpr unsigned kKcBlock = 256;
constexpr uint32_t kDefaultChunk = 1u << 20;  // points per chunk: 64 MiB of points, ~0.4 GiB of MSM scratch
constexpr uint32_t kMaxChunk = 1u << 22;

// ---------------------------------------------------------------- kernels
// res[0] += defective items of the block, res[1] = min(res[1], lowest key of the block): per-wave
// ballot and shuffle, per-block LDS, then one integer atomicAdd and one atomicMin per block that
// has something to report (deterministic). Every thread of the block calls it.
__device__ __forceinline__ void kc_block_report(bool bad, uint64_t key, unsigned long long* res) {
  __shared__ uint32_t s_cnt[kKcBlock / 64];
  __shared__ unsigned long long s_min[kKcBlock / 64];
  const uint32_t cnt = (uint32_t)__popcll(__ballot(bad));
  unsigned long long k = bad ? key : kNoBadKey;
#pragma unroll
  for (int off = 32; off; off >>= 1) {
    const unsigned long long o = __shfl_down(k, off, 64);
    k = o < k ? o : k;
  }
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  if (lane == 0) {
    s_cnt[wave] = cnt;
    s_min[wave] = k;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t total = 0;
    unsigned long long m = kNoBadKey;
#pragma unroll
    for (unsigned w = 0; w < kKcBlock / 64; w++) {
      total += s_cnt[w];
      m = s_min[w] < m ? s_min[w] : m;
    }
    if (total) {
      atomicAdd(&res[0], (unsigned long long)total);
      atomicMin(&res[1], m);
    }
  }
}

// one point per lane (four 16-byte loads); the grid covers n
__global__ __launch_bounds__(kKcBlock) void k_srs_points(const uint4* __restrict__ pts, uint32_t n,
                                                         uint64_t first_index, unsigned long long* res) {
  const uint32_t i = blockIdx.x * kKcBlock + threadIdx.x;
  int st = NZCB_KEY_OK;
  if (i < n) {
    uint32_t w[16];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const uint4 v = pts[size_t(4) * i + k];
      w[4 * k] = v.x;
      w[4 * k + 1] = v.y;
      w[4 * k + 2] = v.z;
      w[4 * k + 3] = v.w;
    }
    st = srs_point_status(w);
  }
  kc_block_report(st != NZCB_KEY_OK, srs_bad_key(first_index + i, st), res);
}

// out[k] = rho_(first + k), 32-byte normal form; the grid covers n
__global__ __launch_bounds__(kKcBlock) void k_srs_weights(uint64_t s0, uint64_t s1, uint64_t s2, uint64_t s3,
                                                          uint32_t first, uint32_t n, uint4* __restrict__ out) {
  const uint32_t k = blockIdx.x * kKcBlock + threadIdx.x;
  if (k >= n) return;
  const uint64_t seed[4] = {s0, s1, s2, s3};
  uint32_t w[8];
  srs_weight(seed, first + k, w);
  out[size_t(2) * k] = make_uint4(w[0], w[1], w[2], w[3]);
  out[size_t(2) * k + 1] = make_uint4(0, 0, 0, 0);
}

// Over n values of 32 bytes. mode 0: a[i] differs from b[i]; 1: a[i] >= r; 2: a[i] differs from
// the unit vector e_unit (Montgomery one at `unit`, zero elsewhere). Count and lowest index.
enum { kCmpEqual = 0, kCmpRange = 1, kCmpUnit = 2 };
__global__ __launch_bounds__(kKcBlock) void k_fr_compare(const uint4* __restrict__ a, const uint4* __restrict__ b,
                                                         uint64_t n, int mode, uint64_t unit,
                                                         unsigned long long* res) {
  const uint64_t i = (uint64_t)blockIdx.x * kKcBlock + threadIdx.x;
  bool bad = false;
  if (i < n) {
    const uint4 lo = a[2 * i], hi = a[2 * i + 1];
    const uint32_t x[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    if (mode == kCmpRange) {
      bad = fr_noncanonical(x);
    } else if (mode == kCmpEqual) {
      const uint4 l2 = b[2 * i], h2 = b[2 * i + 1];
      const uint32_t y[8] = {l2.x, l2.y, l2.z, l2.w, h2.x, h2.y, h2.z, h2.w};
      bad = words8_differ(x, y);
    } else {
      uint32_t y[8];
#pragma unroll
      for (int k = 0; k < 8; k++) y[k] = i == unit ? FrParams::ONE[k] : 0u;
      bad = words8_differ(x, y);
    }
  }
  kc_block_report(bad, i, res);
}

// ---------------------------------------------------------------- timings
// of the calling thread's last check (nzcb_debug_key_check_timings)
enum { kMsPoints, kMsWeights, kMsMsm, kMsDevice, kMsPairing, kMsCall, kMsNtt, kMsCompare, kMsCommit, kMsCount };
thread_local double g_ms[kMsCount] = {0};

using Clock = std::chrono::steady_clock;
double ms_since(const Clock::time_point& t0) {
  return std::chrono::duration<double, std::milli>(Clock::now() - t0).count();
}

// ---------------------------------------------------------------- backends
struct SrsSums {
  G1xyzz l = G1xyzz::inf(), r = G1xyzz::inf();
};
struct Tally {  // defective items and the lowest one's key
  uint64_t n_bad = 0, key = kNoBadKey;
};

struct Backend {
  virtual ~Backend() {}
  // SRS: every point of [0, m)
  virtual Tally points(const uint8_t* pts, uint64_t m) = 0;
  // SRS: L, R over the pairs [lo, hi)
  virtual SrsSums sums(const uint8_t* pts, uint64_t lo, uint64_t hi, const uint64_t seed[4]) = 0;
  // zkey: the n PTau points the commitments are over
  virtual void load_ptau(const uint8_t* pts, uint64_t n) = 0;
  // zkey: one part, n coefficients then 4n evaluations
  virtual void load_part(const uint8_t* part, int power) = 0;
  virtual Tally part_range() = 0;                 // over the 5n values
  virtual Tally part_lagrange(uint64_t unit) = 0;  // NTT_n(coeffs) against e_unit
  virtual Tally part_evals() = 0;                 // NTT_4n(coeffs || 0) against the stored evaluations
  virtual G1Affine part_commit() = 0;             // MSM(PTau[0..n), coeffs)
};

// ---- host
// Bucket method over xyzz_add_affine: sum_i s_i B_i for `bits`-bit scalars (8 LE words each,
// normal form) and bases that are on the curve and not infinity.
G1xyzz host_msm(const G1Affine* bases, const uint32_t* scalars, size_t n, int bits) {
  const int c = n < 128 ? 4 : 8, nw = (bits + c - 1) / c;
  const size_t nb = (size_t(1) << c) - 1;
  std::vector<G1xyzz> bk(nb * (size_t)nw, G1xyzz::inf());
  for (size_t i = 0; i < n; i++) {
    const uint32_t* s = scalars + 8 * i;
    for (int w = 0; w < nw; w++) {
      const int bit = w * c;  // c divides 32: a digit lies in one word
      const uint32_t d = (s[bit >> 5] >> (bit & 31)) & (uint32_t)nb;
      if (d) {
        G1xyzz& b = bk[(size_t)w * nb + d - 1];
        b = xyzz_add_affine(b, bases[i].x, bases[i].y);
      }
    }
  }
  G1xyzz res = G1xyzz::inf();
  for (int w = nw - 1; w >= 0; w--) {
    for (int k = 0; k < c; k++) res = xyzz_dbl(res);
    G1xyzz run = G1xyzz::inf(), sum = G1xyzz::inf();
    for (size_t d = nb; d >= 1; d--) {
      run = xyzz_add(run, bk[(size_t)w * nb + d - 1]);
      sum = xyzz_add(sum, run);
    }
    res = xyzz_add(res, sum);
  }
  return res;
}

// out[i] = sum_j in[j] w^(ij), w = fr_root_of_unity(log_n): the plain forward transform (ntt.h)
void host_ntt(std::vector<Fr>& a, int log_n) {
  const size_t n = size_t(1) << log_n;
  for (size_t i = 0; i < n; i++) {
    size_t j = 0;
    for (int b = 0; b < log_n; b++) j |= ((i >> b) & 1) << (log_n - 1 - b);
    if (i < j) std::swap(a[i], a[j]);
  }
  for (int s = 1; s <= log_n; s++) {
    const size_t half = size_t(1) << (s - 1);
    const Fr wm = fr_root_of_unity(s);
    for (size_t k = 0; k < n; k += 2 * half) {
      Fr w = Fr::one();
      for (size_t j = 0; j < half; j++) {
        const Fr t = w * a[k + j + half], u = a[k + j];
        a[k + j] = u + t;
        a[k + j + half] = u - t;
        w = w * wm;
      }
    }
  }
}

struct HostBackend : Backend {
  std::vector<G1Affine> ptau;
  const uint8_t* part = nullptr;
  int power = 0;

  Tally points(const uint8_t* pts, uint64_t m) override {
    Tally t;
    for (uint64_t i = 0; i < m; i++) {
      uint32_t w[16];
      std::memcpy(w, pts + 64 * i, 64);
      const int st = srs_point_status(w);
      if (st == NZCB_KEY_OK) continue;
      t.n_bad++;
      t.key = std::min(t.key, srs_bad_key(i, st));
    }
    return t;
  }
  SrsSums sums(const uint8_t* pts, uint64_t lo, uint64_t hi, const uint64_t seed[4]) override {
    const size_t n = (size_t)(hi - lo);
    std::vector<G1Affine> b(n + 1);
    std::memcpy((void*)b.data(), pts + 64 * lo, 64 * (n + 1));
    std::vector<uint32_t> s(8 * n);
    for (size_t k = 0; k < n; k++) srs_weight(seed, (uint32_t)(lo + k), s.data() + 8 * k);
    SrsSums r;
    r.l = host_msm(b.data(), s.data(), n, 128);
    r.r = host_msm(b.data() + 1, s.data(), n, 128);
    return r;
  }
  void load_ptau(const uint8_t* pts, uint64_t n) override {
    ptau.resize((size_t)n);
    std::memcpy((void*)ptau.data(), pts, 64 * (size_t)n);
  }
  void load_part(const uint8_t* p, int pw) override {
    part = p;
    power = pw;
  }
  std::vector<Fr> coeffs(size_t len) const {
    const size_t n = size_t(1) << power;
    std::vector<Fr> a(len, Fr::zero());
    std::memcpy((void*)a.data(), part, 32 * n);
    return a;
  }
  static Tally differ(const std::vector<Fr>& got, const uint8_t* want, const Fr* unit_at, uint64_t unit) {
    Tally t;
    for (size_t i = 0; i < got.size(); i++) {
      uint32_t y[8];
      if (want)
        std::memcpy(y, want + 32 * i, 32);
      else
        for (int k = 0; k < 8; k++) y[k] = i == unit ? unit_at->v[k] : 0u;
      if (!words8_differ(got[i].v, y)) continue;
      t.n_bad++;
      t.key = std::min<uint64_t>(t.key, i);
    }
    return t;
  }
  Tally part_range() override {
    Tally t;
    const size_t n5 = size_t(5) << power;
    for (size_t i = 0; i < n5; i++) {
      uint32_t x[8];
      std::memcpy(x, part + 32 * i, 32);
      if (!fr_noncanonical(x)) continue;
      t.n_bad++;
      t.key = std::min<uint64_t>(t.key, i);
    }
    return t;
  }
  Tally part_lagrange(uint64_t unit) override {
    std::vector<Fr> a = coeffs(size_t(1) << power);
    host_ntt(a, power);
    const Fr one = Fr::one();
    return differ(a, nullptr, &one, unit);
  }
  Tally part_evals() override {
    std::vector<Fr> a = coeffs(size_t(4) << power);
    host_ntt(a, power + 2);
    return differ(a, part + (size_t(32) << power), nullptr, 0);
  }
  G1Affine part_commit() override {
    const size_t n = size_t(1) << power;
    std::vector<G1Affine> b;
    std::vector<uint32_t> sv;
    for (size_t i = 0; i < n; i++) {
      Fr v;
      std::memcpy(v.v, part + 32 * i, 32);
      v = from_mont(v);
      if (v.is_zero()) continue;  // and a base at a zero coefficient is never touched
      b.push_back(ptau[i]);
      sv.insert(sv.end(), v.v, v.v + 8);
    }
    return xyzz_to_affine(host_msm(b.data(), sv.data(), b.size(), 256));
  }
};

// ---- device
struct DeviceBackend : Backend {
  CallScope cs;  // first: the members below are freed on its device
  uint32_t chunk;
  MsmScratch sc;
  NttTables ntt_tables;
  uint8_t* d_pts = nullptr;  // `chunk` points
  uint8_t* d_w = nullptr;    // chunk - 1 weights
  unsigned long long* d_res = nullptr;
  // zkey
  DevBuf<G1Affine> d_ptau;
  DevBuf<Fr> d_part, d_pad, d_out;
  int power = 0;

  // msm_points: the largest MSM of the call; max_log_ntt < 0: no transforms
  DeviceBackend(int device, uint32_t chunk_points, size_t msm_points, int max_log_ntt)
      : cs(device, nullptr, 2), chunk(chunk_points) {
    d_pts = cs.alloc<uint8_t>(size_t(64) * chunk);
    d_w = cs.alloc<uint8_t>(size_t(32) * chunk);
    d_res = cs.alloc<unsigned long long>(16);
    if (msm_points) sc.init(msm_points);
    if (max_log_ntt >= 0) ntt_tables.init(max_log_ntt, cs.st);
  }
  ~DeviceBackend() override { (void)hipStreamSynchronize(cs.st); }

  void res_reset() {
    const unsigned long long init[2] = {0, kNoBadKey};
    NZ_HIP(hipMemcpyAsync(d_res, init, sizeof init, hipMemcpyHostToDevice, cs.st));
    NZ_HIP(hipStreamSynchronize(cs.st));  // `init` leaves scope
  }
  Tally res_read() {
    unsigned long long h[2];
    NZ_HIP(hipMemcpyAsync(h, d_res, sizeof h, hipMemcpyDeviceToHost, cs.st));
    NZ_HIP(hipStreamSynchronize(cs.st));
    Tally t;
    t.n_bad = h[0];
    t.key = h[1];
    return t;
  }

  Tally points(const uint8_t* pts, uint64_t m) override {
    const auto t0 = Clock::now();
    res_reset();
    for (uint64_t a = 0; a < m; a += chunk) {
      const uint32_t np = (uint32_t)std::min<uint64_t>(chunk, m - a);
      NZ_HIP(hipMemcpyAsync(d_pts, pts + 64 * a, size_t(64) * np, hipMemcpyHostToDevice, cs.st));
      cs.record(0);
      k_srs_points<<<grid_for(np, kKcBlock), kKcBlock, 0, cs.st>>>(reinterpret_cast<const uint4*>(d_pts), np, a,
                                                                    d_res);
      NZ_HIP(hipGetLastError());
      cs.record(1);
      NZ_HIP(hipStreamSynchronize(cs.st));
      g_ms[kMsPoints] += cs.elapsed(0, 1);
    }
    const Tally t = res_read();
    g_ms[kMsDevice] += ms_since(t0);
    return t;
  }

  SrsSums sums(const uint8_t* pts, uint64_t lo, uint64_t hi, const uint64_t seed[4]) override {
    const auto t0 = Clock::now();
    double msm_ms = 0;
    SrsSums r;
    for (uint64_t a = lo; a < hi;) {
      const uint32_t np = (uint32_t)std::min<uint64_t>(chunk - 1, hi - a);  // pairs; np + 1 <= chunk points
      NZ_HIP(hipMemcpyAsync(d_pts, pts + 64 * a, size_t(64) * (np + 1), hipMemcpyHostToDevice, cs.st));
      cs.record(0);
      k_srs_weights<<<grid_for(np, kKcBlock), kKcBlock, 0, cs.st>>>(seed[0], seed[1], seed[2], seed[3], (uint32_t)a,
                                                                     np, reinterpret_cast<uint4*>(d_w));
      NZ_HIP(hipGetLastError());
      cs.record(1);
      const auto t1 = Clock::now();
      const G1Affine* b = reinterpret_cast<const G1Affine*>(d_pts);
      r.l = xyzz_add(r.l, msm(sc, b, reinterpret_cast<const Fr*>(d_w), np, false, cs.st));
      r.r = xyzz_add(r.r, msm(sc, b + 1, reinterpret_cast<const Fr*>(d_w), np, false, cs.st));
      NZ_HIP(hipStreamSynchronize(cs.st));  // d_pts and d_w are written again by the next chunk
      msm_ms += ms_since(t1);
      g_ms[kMsWeights] += cs.elapsed(0, 1);
      a += np;
    }
    g_ms[kMsMsm] += msm_ms;
    g_ms[kMsDevice] += ms_since(t0) - msm_ms;
    return r;
  }

  void load_ptau(const uint8_t* pts, uint64_t n) override {
    d_ptau.alloc((size_t)n);
    NZ_HIP(hipMemcpyAsync(d_ptau.p, pts, 64 * (size_t)n, hipMemcpyHostToDevice, cs.st));
    NZ_HIP(hipStreamSynchronize(cs.st));
  }
  void load_part(const uint8_t* part, int pw) override {
    const size_t n = size_t(1) << pw;
    if (d_part.n != 5 * n) {
      d_part.alloc(5 * n);
      d_pad.alloc(4 * n);
      d_out.alloc(4 * n);
    }
    power = pw;
    const auto t0 = Clock::now();
    NZ_HIP(hipMemcpyAsync(d_part.p, part, 32 * 5 * n, hipMemcpyHostToDevice, cs.st));
    NZ_HIP(hipStreamSynchronize(cs.st));
    g_ms[kMsDevice] += ms_since(t0);
  }
  Tally compare(const Fr* a, const Fr* b, uint64_t n, int mode, uint64_t unit) {
    res_reset();
    cs.record(0);
    k_fr_compare<<<grid_for(n, kKcBlock, 1u << 30), kKcBlock, 0, cs.st>>>(
        reinterpret_cast<const uint4*>(a), reinterpret_cast<const uint4*>(b), n, mode, unit, d_res);
    NZ_HIP(hipGetLastError());
    cs.record(1);
    const Tally t = res_read();
    g_ms[kMsCompare] += cs.elapsed(0, 1);
    return t;
  }
  void transform(const Fr* in, int log_n) {
    cs.record(0);
    ntt(ntt_tables, in, d_out.p, log_n, false, cs.st);
    cs.record(1);
    NZ_HIP(hipStreamSynchronize(cs.st));
    g_ms[kMsNtt] += cs.elapsed(0, 1);
  }
  Tally part_range() override { return compare(d_part.p, nullptr, uint64_t(5) << power, kCmpRange, 0); }
  Tally part_lagrange(uint64_t unit) override {
    transform(d_part.p, power);
    return compare(d_out.p, nullptr, uint64_t(1) << power, kCmpUnit, unit);
  }
  Tally part_evals() override {
    const size_t n = size_t(1) << power;
    NZ_HIP(hipMemcpyAsync(d_pad.p, d_part.p, 32 * n, hipMemcpyDeviceToDevice, cs.st));
    NZ_HIP(hipMemsetAsync(d_pad.p + n, 0, 32 * 3 * n, cs.st));
    transform(d_pad.p, power + 2);
    return compare(d_out.p, d_part.p + n, 4 * (uint64_t)n, kCmpEqual, 0);
  }
  G1Affine part_commit() override {
    const auto t0 = Clock::now();
    const G1Affine a = xyzz_to_affine(msm(sc, d_ptau.p, d_part.p, size_t(1) << power, true, cs.st));
    g_ms[kMsCommit] += ms_since(t0);
    return a;
  }
};

// ---------------------------------------------------------------- the SRS check
void os_seed(uint8_t* b, size_t len) {
  size_t got = 0;
  while (got < len) {
    const ssize_t k = getrandom(b + got, len - got, 0);
    if (k < 0) {
      if (errno == EINTR || errno == EAGAIN) continue;
      throw Error(NZCB_ERR_INTERNAL, std::string("getrandom failed: ") + std::strerror(errno) +
                                         " (no entropy for the check's weights)");
    }
    got += (size_t)k;
  }
}

// 128 B, the layout of X_2 (x.c0, x.c1, y.c0, y.c1, LE Montgomery). False: a coordinate >= q,
// the point at infinity, not on the twist, or outside the subgroup of order r.
bool g2_read(const uint8_t* b, P2* out) {
  Fq c[4];
  bool zero = true;
  for (int i = 0; i < 4; i++) {
    std::memcpy(c[i].v, b + 32 * i, 32);
    if (!(reduce_once(c[i]) == c[i])) return false;
    zero = zero && c[i].is_zero();
  }
  if (zero) return false;
  out->x = {c[0], c[1]};
  out->y = {c[2], c[3]};
  out->inf = false;
  if (!p2_on_twist(*out)) return false;
  P2 acc;
  acc.inf = true;
  for (int bit = 255; bit >= 0; bit--) {
    acc = p2_sum(acc, acc);
    if ((FrParams::P[bit >> 5] >> (bit & 31)) & 1u) acc = p2_sum(acc, *out);
  }
  return acc.inf;
}

void g2_generator_bytes(uint8_t out[128]) {
  const P2 g = g2_generator();
  std::memcpy(out, g.x.a.v, 32);
  std::memcpy(out + 32, g.x.b.v, 32);
  std::memcpy(out + 64, g.y.a.v, 32);
  std::memcpy(out + 96, g.y.b.v, 32);
}

// The steps of include/nzcb.h in their order. g2_first (may be NULL): the file's tauG2[0], which
// the generator step wants equal to the G2 generator.
void srs_check(Backend& be, const uint8_t* pts, uint64_t m, const uint8_t* g2, const uint8_t* g2_first,
               const uint8_t* seed_bytes, nzcb_key_finding* f, uint8_t* lr_out) {
  *f = nzcb_key_finding{};
  if (lr_out) std::memset(lr_out, 0, 128);
  if (m < 1 || m > 0xffffffffull) throw Error(NZCB_ERR_ARG, "key check: 1 <= points < 2^32");
  // G2
  P2 T;
  if (!g2_read(g2, &T)) {
    f->status = NZCB_KEY_ERR_G2;
    return;
  }
  // points
  f->checked = m;
  const Tally t = be.points(pts, m);
  if (t.n_bad) {
    f->status = (int32_t)(t.key & 7u);
    f->index = t.key >> 3;
    f->n_bad = t.n_bad;
    return;
  }
  // generator
  G1Affine g;
  g.x = Fq::one();
  g.y = g.x + g.x;
  uint8_t g2gen[128];
  g2_generator_bytes(g2gen);
  if (std::memcmp(pts, &g, 64) != 0 || (g2_first && std::memcmp(g2_first, g2gen, 128) != 0)) {
    f->status = NZCB_KEY_ERR_GENERATOR;
    return;
  }
  if (m < 2) return;
  // sequence
  uint64_t seed[4];
  uint8_t own[32];
  if (!seed_bytes) {
    os_seed(own, 32);
    seed_bytes = own;
  }
  std::memcpy(seed, seed_bytes, 32);
  const P2 g2one = g2_generator();
  auto holds = [&](const SrsSums& s) {
    const auto t0 = Clock::now();
    f->pairing_checks++;
    const bool ok = pairing_check({{g1_neg(xyzz_to_affine(s.l)), T}, {xyzz_to_affine(s.r), g2one}});
    g_ms[kMsPairing] += ms_since(t0);
    return ok;
  };
  const SrsSums all = be.sums(pts, 0, m - 1, seed);
  if (lr_out) {
    g1_to_le(xyzz_to_affine(all.l), lr_out);
    g1_to_le(xyzz_to_affine(all.r), lr_out + 64);
  }
  if (holds(all)) return;
  // the pairs below lo hold, the first that does not lies in [lo, hi)
  uint64_t lo = 0, hi = m - 1;
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (holds(be.sums(pts, lo, mid, seed)))
      lo = mid;
    else
      hi = mid;
  }
  f->status = NZCB_KEY_ERR_SEQUENCE;
  f->index = lo + 1;  // pair i ties P_i to P_(i+1)
}

uint32_t chunk_of(uint32_t chunk_points) {
  if (chunk_points == 0) return kDefaultChunk;
  if (chunk_points < 2 || chunk_points > kMaxChunk) throw Error(NZCB_ERR_ARG, "key check: chunk_points is 0 or 2..2^22");
  return chunk_points;
}

struct CallClock {
  Clock::time_point t0 = Clock::now();
  CallClock() {
    for (auto& t : g_ms) t = 0;
  }
  ~CallClock() { g_ms[kMsCall] = ms_since(t0); }
};

void srs_check_on(int device, const uint8_t* pts, uint64_t m, const uint8_t* g2, const uint8_t* g2_first,
                  const uint8_t* seed, uint32_t chunk_points, nzcb_key_finding* f, uint8_t* lr_out) {
  if (!pts || !g2 || !f) throw Error(NZCB_ERR_ARG, "null argument");
  CallClock clock;
  const uint32_t chunk = chunk_of(chunk_points);
  if (device == NZCB_KEY_HOST) {
    HostBackend be;
    srs_check(be, pts, m, g2, g2_first, seed, f, lr_out);
  } else {
    const uint32_t c = (uint32_t)std::max<uint64_t>(2, std::min<uint64_t>(chunk, m));
    DeviceBackend be(device, c, c, -1);
    srs_check(be, pts, m, g2, g2_first, seed, f, lr_out);
  }
}

void ptau_check(const uint8_t* ptau, size_t len, uint64_t count, int device, const uint8_t* seed,
                nzcb_key_finding* out) {
  if (!out) throw Error(NZCB_ERR_ARG, "null argument");
  const PtauView v = ptau_open(ptau, len, count);
  srs_check_on(device, v.g1, v.count, v.g2_1, v.g2_0, seed, 0, out, nullptr);
}

// ---------------------------------------------------------------- the zkey check
void zkey_check(const uint8_t* zk, size_t len, int device, const uint8_t* seed, int* ok, nzcb_key_finding* header_srs,
                nzcb_key_finding* parts, uint32_t parts_cap, uint32_t* n_parts) {
  if (!ok || !header_srs || !n_parts || (parts_cap && !parts)) throw Error(NZCB_ERR_ARG, "null argument");
  CallClock clock;
  const Zkey z = parse_zkey(zk, len);
  const uint64_t n = z.domainSize;
  const uint32_t n_lag = z.nPublic ? z.nPublic : 1, total = 8 + n_lag;
  *n_parts = total;
  std::unique_ptr<Backend> be;
  if (device == NZCB_KEY_HOST) {
    be.reset(new HostBackend());
  } else {
    const uint32_t c = (uint32_t)std::min<uint64_t>(kDefaultChunk, n + 6);
    be.reset(new DeviceBackend(device, c, (size_t)std::max<uint64_t>(c, n), z.power + 2));
  }
  bool all = true;
  // cosets: <w>, k1 <w> and k2 <w> must be disjoint
  nzcb_key_finding& hc = header_srs[0];
  hc = nzcb_key_finding{};
  hc.checked = 2;
  if (fr_noncanonical(z.k1.v) || fr_noncanonical(z.k2.v)) {
    hc.status = NZCB_KEY_ERR_NONCANONICAL;
    hc.index = fr_noncanonical(z.k1.v) ? 0 : 1;
  } else {
    const Fr a = pow_u64(z.k1, n), b = pow_u64(z.k2, n), one = Fr::one();
    if (a.is_zero() || b.is_zero() || a == one || b == one || a == b) hc.status = NZCB_KEY_ERR_COSETS;
  }
  all = all && hc.status == NZCB_KEY_OK;
  // the key's own PTau against X_2
  nzcb_key_finding& hs = header_srs[1];
  srs_check(*be, z.ptau.p, n + 6, z.X2, nullptr, seed, &hs, nullptr);
  const bool srs_ok = hs.status == NZCB_KEY_OK;
  all = all && srs_ok;
  if (srs_ok) be->load_ptau(z.ptau.p, n);
  const G1Affine* header_pts[8] = {&z.Qm, &z.Ql, &z.Qr, &z.Qo, &z.Qc, &z.S1, &z.S2, &z.S3};
  const size_t part_bytes = (size_t)5 * n * 32;
  for (uint32_t k = 0; k < total; k++) {
    const uint8_t* p;
    if (k < 5) {
      const Section* q[5] = {&z.qm, &z.ql, &z.qr, &z.qo, &z.qc};
      p = q[k]->p;
    } else if (k < 8) {
      p = z.sigma.p + part_bytes * (k - 5);
    } else {
      p = z.lagrange.p + part_bytes * (k - 8);
    }
    nzcb_key_finding f{};
    f.checked = 5 * n;
    be->load_part(p, z.power);
    Tally t = be->part_range();
    if (t.n_bad) {
      f.status = NZCB_KEY_ERR_NONCANONICAL;
    } else if (k >= 8 && (t = be->part_lagrange(k - 8)).n_bad) {
      f.status = NZCB_KEY_ERR_LAGRANGE;
    } else if ((t = be->part_evals()).n_bad) {
      f.status = NZCB_KEY_ERR_EVALS;
    } else if (k < 8 && srs_ok) {
      f.pairing_checks = 1;  // commit_checked
      const G1Affine c = be->part_commit();
      if (std::memcmp(&c, header_pts[k], 64) != 0) f.status = NZCB_KEY_ERR_COMMIT;
    }
    if (t.n_bad) {
      f.index = t.key;
      f.n_bad = t.n_bad;
    }
    all = all && f.status == NZCB_KEY_OK;
    if (k < parts_cap) parts[k] = f;
  }
  *ok = all ? 1 : 0;
}

}  // namespace

}  // namespace nzcb

using namespace nzcb;

extern "C" {

int nzcb_engine_srs_check(int device, const uint8_t* points, uint64_t m, const uint8_t* g2, const uint8_t* seed,
                          uint32_t chunk_points, nzcb_key_finding* finding, uint8_t* lr_out, nzcb_err* err) {
  return guarded(err, [&] { srs_check_on(device, points, m, g2, nullptr, seed, chunk_points, finding, lr_out); });
}

int nzcb_debug_key_check_timings(double* ms, int cap) {
  int k = 0;
  for (; ms && k < cap && k < kMsCount; k++) ms[k] = g_ms[k];
  return k;
}

int nzcb_ptau_check(const uint8_t* ptau, size_t len, uint64_t count, int device, const uint8_t* seed,
                    nzcb_key_finding* out, nzcb_err* err) {
  return guarded(err, [&] { ptau_check(ptau, len, count, device, seed, out); });
}

int nzcb_ptau_check_file(const char* path, uint64_t count, int device, const uint8_t* seed, nzcb_key_finding* out,
                         nzcb_err* err) {
  return guarded(err, [&] {
    if (!path) throw Error(NZCB_ERR_ARG, "null argument");
    MappedFile mf(path, "the ptau", "ptau: invalid file format");
    ptau_check(mf.data, mf.size, count, device, seed, out);
  });
}

int nzcb_zkey_check(const uint8_t* zkey, size_t len, int device, const uint8_t* seed, int* ok,
                    nzcb_key_finding* header_srs, nzcb_key_finding* parts, uint32_t parts_cap, uint32_t* n_parts,
                    nzcb_err* err) {
  return guarded(err, [&] { zkey_check(zkey, len, device, seed, ok, header_srs, parts, parts_cap, n_parts); });
}

int nzcb_zkey_check_file(const char* path, int device, const uint8_t* seed, int* ok, nzcb_key_finding* header_srs,
                         nzcb_key_finding* parts, uint32_t parts_cap, uint32_t* n_parts, nzcb_err* err) {
  return guarded(err, [&] {
    if (!path) throw Error(NZCB_ERR_ARG, "null argument");
    MappedFile mf(path, "the zkey", "zkey: Invalid File format");
    zkey_check(mf.data, mf.size, device, seed, ok, header_srs, parts, parts_cap, n_parts);
  });
}

}  // extern "C"
