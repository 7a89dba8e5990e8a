// Powers of tau on the GPU: contribute and prepare phase 2 (include/nzcb.h nzcb_ptau_new,
// nzcb_ptau_contribute, nzcb_ptau_prepare_phase2; the `phase1` recipe of snarkjs).
//
// Every kernel is a template over the coordinate field, Fq for G1 and Fq2 for G2 (ptau_ops.h):
//   k_pt_test     one lane per stored point: range and curve equation, count and lowest index;
//   k_pt_scale    one lane per point: the scalar c tau^i derived in the lane, double-and-add with
//                 the affine input as the mixed addend, one inversion back to affine;
//   k_intt_*      the inverse DFT of a run of points, out[k] = sum_i (1/n) w^(-ik) P_i: radix-2
//                 DIT over XYZZ points as lagrange.hip does it for one size of G1, a scaled
//                 bit-reversed load, log n butterfly stages whose twiddle product is a 254-bit
//                 scalar multiplication, an affine store. Lanes of a wave share their twiddle
//                 while a stage has >= 64 groups. The levels of a section up to 16 run side by side,
//                 one launch per stage for all of them; each larger level runs alone.
// A section is held resident whole (power 24: 2 GiB of G2 points, 4 GiB of XYZZ work space).
// Both operations run the same driver over a backend: the device one here, or the host one
// (NZCB_PTAU_HOST), which calls the same NZ_HD functions and gives the same bytes. A call owns
// its stream and buffers (devcall.h CallScope) and needs no prover context.
#include <sys/random.h>

#include <algorithm>
#include <cerrno>
#include <chrono>
#include <cstring>
#include <thread>
#include <vector>

#include "devcall.h"
#include "ptau_ops.h"

namespace nzcb {

namespace {

constexpr unsigned kPB = 256;

// ---------------------------------------------------------------- kernels
__device__ __forceinline__ uint32_t bitrev(uint32_t x, int bits) { return __brev(x) >> (32 - bits); }

// res[0] += defective points, res[1] = min(res[1], their keys): defects are rare, one atomic pair each
template <class F>
__global__ __launch_bounds__(kPB) void k_pt_test(const PtAffine<F>* __restrict__ pts, uint64_t n, Fq2 b2,
                                                 unsigned long long* res) {
  const uint64_t i = (uint64_t)blockIdx.x * kPB + threadIdx.x;
  if (i >= n) return;
  const PtAffine<F> p = pts[i];
  const int st = pt_status<F>(&p, b2);
  if (st != NZCB_KEY_OK) {
    atomicAdd(&res[0], 1ull);
    atomicMin(&res[1], (unsigned long long)srs_bad_key(i, st));
  }
}

// pts[i] = (c tau^i) pts[i]; sec = {c, tau}, Montgomery, in device memory the call wipes
template <class F>
__global__ __launch_bounds__(kPB) void k_pt_scale(PtAffine<F>* __restrict__ pts, uint64_t n,
                                                  const Fr* __restrict__ sec) {
  const uint64_t i = (uint64_t)blockIdx.x * kPB + threadIdx.x;
  if (i >= n) return;
  const Fr k = ptau_scalar(sec[0], sec[1], i);
  const PtAffine<F> p = pts[i];
  pts[i] = pt_to_affine(pt_mul_affine(p, k));
}

// tw[k] = w^-k (normal form) for k < half
__global__ void k_intt_twiddles(Fr* __restrict__ tw, Fr winv, uint32_t half) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= half) return;
  tw[k] = from_mont(pow_u64(winv, (uint64_t)k));
}

// The transforms of the levels lo..hi of one section run side by side: level p works on the 2^p
// points of X from 2^p - 2^lo on (the order of the levels in the file), and a stage is one launch
// for all of them, so a section costs hi launches and not their sum over the levels.
//
// Thread t of 2^lo <= t < 2^(hi+1) loads point e = t - 2^p of level p = floor(log2 t):
// X[bitrev(e)] = (1/2^p) src[e]; a point past n_src is the point at infinity. inv_n[p]: normal form.
template <class F>
__global__ __launch_bounds__(kPB) void k_intt_load(const PtAffine<F>* __restrict__ src, uint64_t n_src, int lo,
                                                   uint32_t count, const Fr* __restrict__ inv_n,
                                                   PtXyzz<F>* __restrict__ X) {
  const uint32_t tid = blockIdx.x * kPB + threadIdx.x;
  if (tid >= count) return;
  const uint32_t t = tid + (1u << lo);
  const int p = 31 - __clz(t);
  const uint32_t e = t - (1u << p);
  PtXyzz<F> r = PtXyzz<F>::inf();
  if (e < n_src) {
    const PtAffine<F> a = src[e];
    r = p ? pt_mul_affine(a, inv_n[p]) : pt_from_affine(a);
  }
  X[(size_t)(1u << p) - (1u << lo) + (p ? bitrev(e, p) : 0u)] = r;
}

// Stage s of every level p > s: blocks of 2 half = 2^(s+1) points, butterfly (u, v) ->
// (u + w v, u - w v). Thread t of t0 <= t < 2^hi (t0 = 2^(lo-1), or 0 for lo = 0, where t = 0
// idles so that a level begins on a wave) is butterfly b = t - 2^(p-1) of level p =
// floor(log2 t) + 1. tw: the table of level hi, so w_(2^p)^-j = tw[j 2^(hi-p)].
template <class F>
__global__ __launch_bounds__(kPB) void k_intt_stage(PtXyzz<F>* __restrict__ X, int lo, int hi, uint32_t count, int s,
                                                    const Fr* __restrict__ tw) {
  const uint32_t tid = blockIdx.x * kPB + threadIdx.x;
  if (tid >= count) return;
  const uint32_t t = tid + (lo ? 1u << (lo - 1) : 0u);
  if (t == 0) return;
  const int p = 32 - __clz(t);
  if (s >= p) return;
  const uint32_t b = t - (1u << (p - 1));
  const uint32_t half = 1u << s;
  const uint32_t groups = 1u << (p - 1 - s);
  uint32_t g, j;
  if (groups >= 64) {  // consecutive threads: same j (a wave-uniform twiddle), different groups
    j = b / groups;
    g = b % groups;
  } else {
    g = b / half;
    j = b % half;
  }
  const size_t i0 = (size_t)(1u << p) - (1u << lo) + g * 2 * half + j, i1 = i0 + half;
  PtXyzz<F> v = X[i1];
  if (j) v = pt_mul(v, tw[j << (hi - 1 - s)]);
  const PtXyzz<F> u = X[i0];  // after the product: u is not live across its loop
  X[i0] = pt_add(u, v);
  X[i1] = pt_add(u, pt_neg(v));
}

template <class F>
__global__ __launch_bounds__(kPB) void k_intt_store(const PtXyzz<F>* __restrict__ X, uint32_t n,
                                                    PtAffine<F>* __restrict__ out) {
  const uint32_t k = blockIdx.x * kPB + threadIdx.x;
  if (k >= n) return;
  out[k] = pt_to_affine(X[k]);
}

// ---------------------------------------------------------------- timings
// of the calling thread's last operation (nzcb_debug_ptau_timings)
enum { kMsKernels, kMsCall, kMsCount };
thread_local double g_ms[kMsCount] = {0};
using Clock = std::chrono::steady_clock;
struct CallClock {
  Clock::time_point t0 = Clock::now();
  CallClock() {
    for (auto& t : g_ms) t = 0;
  }
  ~CallClock() { g_ms[kMsCall] = std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }
};

// the highest level that shares a run with the levels below it (nzcb_debug_ptau_batch_top)
constexpr int kDefaultBatchTop = 16;
int g_batch_top = kDefaultBatchTop;

// ---------------------------------------------------------------- backends
uint32_t bitrev_host(uint32_t x, int bits) {
  uint32_t r = 0;
  for (int b = 0; b < bits; b++) r |= ((x >> b) & 1u) << (bits - 1 - b);
  return r;
}

struct HostBackend {
  Fq2 b2 = g2_twist_b();

  template <class F>
  Tally test(const uint8_t* pts, uint64_t n) {
    Tally t;
    for (uint64_t i = 0; i < n; i++) {
      PtAffine<F> p;
      std::memcpy((void*)&p, pts + sizeof p * i, sizeof p);
      const int st = pt_status<F>(&p, b2);
      if (st == NZCB_KEY_OK) continue;
      t.n_bad++;
      t.key = std::min(t.key, srs_bad_key(i, st));
    }
    return t;
  }
  template <class F>
  void scale(const uint8_t* src, uint64_t n, const Fr& c, const Fr& tau, uint8_t* dst) {
    parallel_for(n, [&](uint64_t i) {
      PtAffine<F> p;
      std::memcpy((void*)&p, src + sizeof p * i, sizeof p);
      Fr k = ptau_scalar(c, tau, i);
      p = pt_to_affine(pt_mul_affine(p, k));
      std::memcpy(dst + sizeof p * i, &p, sizeof p);
      wipe(&k, sizeof k);
    });
  }
  // levels 0..top of the n_src points at src, back to back at dst
  template <class F>
  void lagrange(const uint8_t* src, uint64_t n_src, int top, uint8_t* dst) {
    std::vector<PtXyzz<F>> X;
    std::vector<Fr> tw;
    for (int p = 0; p <= top; p++) {
      const uint32_t n = 1u << p;
      uint8_t* out = dst + sizeof(PtAffine<F>) * (uint64_t)(n - 1);
      if (p == 0) {
        std::memcpy(out, src, sizeof(PtAffine<F>));
        continue;
      }
      X.assign(n, PtXyzz<F>::inf());
      tw.resize(n / 2);
      const Fr winv = inverse(ptau_root_of_unity(p)), inv_n = ptau_inv_n(p);
      tw[0] = from_mont(Fr::one());
      Fr acc = Fr::one();
      for (uint32_t k = 1; k < n / 2; k++) {
        acc = acc * winv;
        tw[k] = from_mont(acc);
      }
      parallel_for(std::min<uint64_t>(n, n_src), [&](uint64_t i) {
        PtAffine<F> a;
        std::memcpy((void*)&a, src + sizeof a * i, sizeof a);
        X[bitrev_host((uint32_t)i, p)] = pt_mul_affine(a, inv_n);
      });
      for (int s = 0; s < p; s++) {
        const uint32_t half = 1u << s;
        parallel_for(n / 2, [&](uint64_t b) {
          const uint32_t g = (uint32_t)b / half, j = (uint32_t)b % half;
          const uint32_t i0 = g * 2 * half + j, i1 = i0 + half;
          PtXyzz<F> v = X[i1];
          if (j) v = pt_mul(v, tw[(size_t)j << (p - 1 - s)]);
          const PtXyzz<F> u = X[i0];
          X[i0] = pt_add(u, v);
          X[i1] = pt_add(u, pt_neg(v));
        });
      }
      parallel_for(n, [&](uint64_t k) {
        const PtAffine<F> a = pt_to_affine(X[k]);
        std::memcpy(out + sizeof a * k, &a, sizeof a);
      });
    }
  }
};

struct DeviceBackend {
  CallScope cs;  // first: the buffers below are freed on its device
  Fq2 b2 = g2_twist_b();
  unsigned long long* d_res;
  Fr* d_sec;  // c, tau of the section being scaled
  int batch_top = g_batch_top;

  explicit DeviceBackend(int device) : cs(device, nullptr, 2) {
    d_res = cs.alloc<unsigned long long>(16);
    d_sec = cs.alloc<Fr>(2 * sizeof(Fr));
  }
  ~DeviceBackend() {
    (void)hipMemsetAsync(d_sec, 0, 2 * sizeof(Fr), cs.st);
    (void)hipStreamSynchronize(cs.st);
  }
  template <class F>
  Tally test(const uint8_t* pts, uint64_t n) {
    DevBuf<uint8_t> d(sizeof(PtAffine<F>) * n);
    const unsigned long long init[2] = {0, kNoBadKey};
    unsigned long long h[2];
    NZ_HIP(hipMemcpyAsync(d_res, init, sizeof init, hipMemcpyHostToDevice, cs.st));
    NZ_HIP(hipMemcpyAsync(d.p, pts, d.n, hipMemcpyHostToDevice, cs.st));
    cs.record(0);
    k_pt_test<F><<<grid_for(n, kPB, 1u << 30), kPB, 0, cs.st>>>(reinterpret_cast<const PtAffine<F>*>(d.p), n, b2,
                                                                 d_res);
    NZ_HIP(hipGetLastError());
    cs.record(1);
    NZ_HIP(hipMemcpyAsync(h, d_res, sizeof h, hipMemcpyDeviceToHost, cs.st));
    NZ_HIP(hipStreamSynchronize(cs.st));
    g_ms[kMsKernels] += cs.elapsed(0, 1);
    Tally t;
    t.n_bad = h[0];
    t.key = h[1];
    return t;
  }
  template <class F>
  void scale(const uint8_t* src, uint64_t n, const Fr& c, const Fr& tau, uint8_t* dst) {
    DevBuf<uint8_t> d(sizeof(PtAffine<F>) * n);
    Fr sec[2] = {c, tau};
    NZ_HIP(hipMemcpyAsync(d_sec, sec, sizeof sec, hipMemcpyHostToDevice, cs.st));
    NZ_HIP(hipMemcpyAsync(d.p, src, d.n, hipMemcpyHostToDevice, cs.st));
    NZ_HIP(hipStreamSynchronize(cs.st));
    wipe(sec, sizeof sec);
    cs.record(0);
    k_pt_scale<F><<<grid_for(n, kPB, 1u << 30), kPB, 0, cs.st>>>(reinterpret_cast<PtAffine<F>*>(d.p), n, d_sec);
    NZ_HIP(hipGetLastError());
    cs.record(1);
    NZ_HIP(hipMemsetAsync(d_sec, 0, 2 * sizeof(Fr), cs.st));
    NZ_HIP(hipMemcpyAsync(dst, d.p, d.n, hipMemcpyDeviceToHost, cs.st));
    NZ_HIP(hipStreamSynchronize(cs.st));  // d is freed on return
    g_ms[kMsKernels] += cs.elapsed(0, 1);
  }
  // Levels lo..hi of the section at d_src into dst (the section's level 0 is at dst).
  template <class F>
  void levels(const PtAffine<F>* d_src, uint64_t n_src, int lo, int hi, PtXyzz<F>* d_x, PtAffine<F>* d_out,
              Fr* d_tw, const Fr* d_inv_n, uint8_t* dst) {
    const uint32_t pts = (2u << hi) - (1u << lo);
    const uint32_t t0 = lo ? 1u << (lo - 1) : 0u, bf = (1u << hi) - t0;
    cs.record(0);
    if (hi) {
      k_intt_twiddles<<<grid_for(std::max(1u, 1u << (hi - 1)), kPB), kPB, 0, cs.st>>>(
          d_tw, inverse(ptau_root_of_unity(hi)), 1u << (hi - 1));
      NZ_HIP(hipGetLastError());
    }
    k_intt_load<F><<<grid_for(pts, kPB), kPB, 0, cs.st>>>(d_src, n_src, lo, pts, d_inv_n, d_x);
    NZ_HIP(hipGetLastError());
    for (int s = 0; s < hi; s++) {
      k_intt_stage<F><<<grid_for(bf, kPB), kPB, 0, cs.st>>>(d_x, lo, hi, bf, s, d_tw);
      NZ_HIP(hipGetLastError());
    }
    k_intt_store<F><<<grid_for(pts, kPB), kPB, 0, cs.st>>>(d_x, pts, d_out);
    NZ_HIP(hipGetLastError());
    cs.record(1);
    NZ_HIP(hipMemcpyAsync(dst + sizeof(PtAffine<F>) * (uint64_t)((1u << lo) - 1), d_out,
                          sizeof(PtAffine<F>) * (uint64_t)pts, hipMemcpyDeviceToHost, cs.st));
    NZ_HIP(hipStreamSynchronize(cs.st));
    g_ms[kMsKernels] += cs.elapsed(0, 1);
  }
  // levels 0..top of the n_src points at src, back to back at dst: the levels up to batch_top in
  // one run, each larger one in its own, so the work space is that of the top level
  template <class F>
  void lagrange(const uint8_t* src, uint64_t n_src, int top, uint8_t* dst) {
    using A = PtAffine<F>;
    using X = PtXyzz<F>;
    const int first = std::min(top, batch_top);
    const size_t room = std::max<size_t>(size_t(2) << first, size_t(1) << top);
    DevBuf<A> d_src((size_t)n_src), d_out(room);
    DevBuf<X> d_x(room);
    DevBuf<Fr> d_tw(std::max<size_t>(1, size_t(1) << top >> 1)), d_inv_n(kPtauMaxPower + 2);
    Fr inv_n[kPtauMaxPower + 2];
    for (int p = 0; p < kPtauMaxPower + 2; p++) inv_n[p] = ptau_inv_n(p);
    NZ_HIP(hipMemcpyAsync(d_inv_n.p, inv_n, sizeof inv_n, hipMemcpyHostToDevice, cs.st));
    NZ_HIP(hipMemcpyAsync(d_src.p, src, sizeof(A) * n_src, hipMemcpyHostToDevice, cs.st));
    levels<F>(d_src.p, n_src, 0, first, d_x.p, d_out.p, d_tw.p, d_inv_n.p, dst);
    for (int p = first + 1; p <= top; p++) levels<F>(d_src.p, n_src, p, p, d_x.p, d_out.p, d_tw.p, d_inv_n.p, dst);
  }
};

// ---------------------------------------------------------------- the operations
template <class Be, class F>
void test_section(Be& be, const PtauSections& f, int id) {
  const Tally t = be.template test<F>(f.s[id].p, f.points(id));
  if (!t.n_bad) return;
  const int st = (int)(t.key & 7u);
  throw Error(NZCB_ERR_FORMAT, "ptau: section " + std::to_string(id) + " point " + std::to_string(t.key >> 3) +
                                   (st == NZCB_KEY_ERR_RANGE ? " has a coordinate that is not below q"
                                                             : " is not on the curve") +
                                   " (" + std::to_string(t.n_bad) + " defective in the section)");
}

template <class Be>
void contribute(Be& be, const PtauSections& f, const Fr sec[3], const char* out_path, PtauOut& o) {
  test_section<Be, Fq>(be, f, 2);
  test_section<Be, Fq2>(be, f, 3);
  test_section<Be, Fq>(be, f, 4);
  test_section<Be, Fq>(be, f, 5);
  test_section<Be, Fq2>(be, f, 6);
  o.open(out_path, 12 + ptau_base_bytes(f.power, f.s[1].len, f.s[7].len));
  o.file_header(7);
  std::memcpy(o.section(1, f.s[1].len), f.s[1].p, (size_t)f.s[1].len);
  const Fr one = Fr::one();
  const Fr *tau = &sec[0], *alpha = &sec[1], *beta = &sec[2];
  be.template scale<Fq>(f.s[2].p, f.points(2), one, *tau, o.section(2, 64 * f.points(2)));
  be.template scale<Fq2>(f.s[3].p, f.points(3), one, *tau, o.section(3, 128 * f.points(3)));
  be.template scale<Fq>(f.s[4].p, f.points(4), *alpha, *tau, o.section(4, 64 * f.points(4)));
  be.template scale<Fq>(f.s[5].p, f.points(5), *beta, *tau, o.section(5, 64 * f.points(5)));
  be.template scale<Fq2>(f.s[6].p, 1, *beta, *tau, o.section(6, 128));
  std::memcpy(o.section(7, f.s[7].len), f.s[7].p, (size_t)f.s[7].len);
  o.commit();
}

template <class Be>
void prepare(Be& be, const PtauSections& f, const char* out_path, PtauOut& o) {
  const uint64_t n = uint64_t(1) << f.power;
  const uint64_t base = ptau_base_bytes(f.power, f.s[1].len, f.s[7].len);
  // a section is its levels 0..power, 2n - 1 points; section 12 adds level power + 1
  o.open(out_path, 12 + base + 4 * 12 + 64 * (4 * n - 1) + 128 * (2 * n - 1) + 2 * 64 * (2 * n - 1));
  o.file_header(11);
  for (int id = 1; id <= 7; id++) {
    const uint64_t len = id == 1 || id == 7 ? f.s[id].len : f.points(id) * PtauSections::point_bytes(id);
    std::memcpy(o.section((uint32_t)id, len), f.s[id].p, (size_t)len);
  }
  be.template lagrange<Fq>(f.s[2].p, f.points(2), (int)f.power + 1, o.section(12, 64 * (4 * n - 1)));
  be.template lagrange<Fq2>(f.s[3].p, f.points(3), (int)f.power, o.section(13, 128 * (2 * n - 1)));
  be.template lagrange<Fq>(f.s[4].p, f.points(4), (int)f.power, o.section(14, 64 * (2 * n - 1)));
  be.template lagrange<Fq>(f.s[5].p, f.points(5), (int)f.power, o.section(15, 64 * (2 * n - 1)));
  o.commit();
}

struct Secrets {
  Fr s[3];
  ~Secrets() { wipe(s, sizeof s); }
};

void contribute_on(int device, const uint8_t* ptau, size_t len, const uint8_t* secrets, const uint8_t* entropy,
                   size_t entropy_len, const char* out_path, PtauOut& o) {
  if (!ptau) throw Error(NZCB_ERR_ARG, "null argument");
  CallClock clock;
  const PtauSections f = ptau_sections_open(ptau, len);
  Secrets sec;
  make_secrets(secrets, entropy, entropy_len, sec.s);
  if (device == NZCB_PTAU_HOST) {
    HostBackend be;
    contribute(be, f, sec.s, out_path, o);
  } else {
    DeviceBackend be(device);
    contribute(be, f, sec.s, out_path, o);
  }
}

void prepare_on(int device, const uint8_t* ptau, size_t len, const char* out_path, PtauOut& o) {
  if (!ptau) throw Error(NZCB_ERR_ARG, "null argument");
  CallClock clock;
  const PtauSections f = ptau_sections_open(ptau, len);
  if (device == NZCB_PTAU_HOST) {
    HostBackend be;
    prepare(be, f, out_path, o);
  } else {
    DeviceBackend be(device);
    prepare(be, f, out_path, o);
  }
}

// creating the output truncates it: it must not be the file that is mapped as the input
void require_distinct(const char* in_path, const char* out_path) {
  struct stat a, b;
  if (stat(in_path, &a) == 0 && stat(out_path, &b) == 0 && a.st_dev == b.st_dev && a.st_ino == b.st_ino)
    throw Error(NZCB_ERR_ARG, "ptau: the output path is the input file");
}

void give(PtauOut& o, uint8_t** out, size_t* out_len) {
  *out_len = (size_t)o.len;
  *out = o.release();
}

}  // namespace

}  // namespace nzcb

using namespace nzcb;

extern "C" {

int nzcb_ptau_new(int power, uint8_t** ptau_out, size_t* ptau_len, nzcb_err* err) {
  return guarded(err, [&] {
    if (!ptau_out || !ptau_len) throw Error(NZCB_ERR_ARG, "null argument");
    PtauOut o;
    ptau_new(power, o, nullptr);
    give(o, ptau_out, ptau_len);
  });
}

int nzcb_ptau_new_file(int power, const char* out_path, nzcb_err* err) {
  return guarded(err, [&] {
    if (!out_path) throw Error(NZCB_ERR_ARG, "null argument");
    PtauOut o;
    ptau_new(power, o, out_path);
  });
}

int nzcb_ptau_contribute(const uint8_t* ptau, size_t len, const uint8_t* secrets, const uint8_t* entropy,
                         size_t entropy_len, int device, uint8_t** ptau_out, size_t* ptau_len, nzcb_err* err) {
  return guarded(err, [&] {
    if (!ptau_out || !ptau_len) throw Error(NZCB_ERR_ARG, "null argument");
    PtauOut o;
    contribute_on(device, ptau, len, secrets, entropy, entropy_len, nullptr, o);
    give(o, ptau_out, ptau_len);
  });
}

int nzcb_ptau_contribute_file(const char* in_path, const char* out_path, const uint8_t* secrets,
                              const uint8_t* entropy, size_t entropy_len, int device, nzcb_err* err) {
  return guarded(err, [&] {
    if (!in_path || !out_path) throw Error(NZCB_ERR_ARG, "null argument");
    require_distinct(in_path, out_path);
    MappedFile mf(in_path, "the ptau", "ptau: invalid file format");
    PtauOut o;
    contribute_on(device, mf.data, mf.size, secrets, entropy, entropy_len, out_path, o);
  });
}

int nzcb_ptau_prepare_phase2(const uint8_t* ptau, size_t len, int device, uint8_t** ptau_out, size_t* ptau_len,
                             nzcb_err* err) {
  return guarded(err, [&] {
    if (!ptau_out || !ptau_len) throw Error(NZCB_ERR_ARG, "null argument");
    PtauOut o;
    prepare_on(device, ptau, len, nullptr, o);
    give(o, ptau_out, ptau_len);
  });
}

int nzcb_ptau_prepare_phase2_file(const char* in_path, const char* out_path, int device, nzcb_err* err) {
  return guarded(err, [&] {
    if (!in_path || !out_path) throw Error(NZCB_ERR_ARG, "null argument");
    require_distinct(in_path, out_path);
    MappedFile mf(in_path, "the ptau", "ptau: invalid file format");
    PtauOut o;
    prepare_on(device, mf.data, mf.size, out_path, o);
  });
}

int nzcb_debug_ptau_batch_top(int level) {
  const int prev = g_batch_top;
  g_batch_top = level < 0 ? kDefaultBatchTop : std::min(level, kPtauMaxPower + 1);
  return prev;
}

int nzcb_debug_ptau_timings(double* ms, int cap) {
  int k = 0;
  for (; ms && k < cap && k < kMsCount; k++) ms[k] = g_ms[k];
  return k;
}

}  // extern "C"
