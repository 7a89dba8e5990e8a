// Batch PLONK verification: one pairing check for N proofs, the G1 scalar multiplications
// on the GPU (include/nzcb.h nzcb_verify_batch).
//
// nzcb_verify costs 20 G1 scalar multiplications and one 2-pairing check per proof. With
// random 128-bit weights rho_i, N proofs that each satisfy e(-L_i, X_2) e(R_i, [1]_2) = 1
// (L_i, R_i: verify.h plonk_terms) satisfy
//   e(-sum rho_i L_i, X_2) * e(sum rho_i R_i, [1]_2) = 1,
// and a batch with an invalid item passes that with probability of order 2^-128. The 20 N
// multiplications (every scalar times rho_i first, in Fr, on the host) are independent: one
// lane each (k_g1_term_mul), then one lane per group adds its terms and converts to affine
// (k_g1_group_sum); two groups per item give L'_i = rho_i L_i and R'_i = rho_i R_i. The host
// adds those and runs the pairing check; when it fails, it bisects over index ranges with
// sums of the same per-item points (no further scalar multiplication).
//
// A call owns its stream and its device buffer and needs no prover context; it may run
// while a context proves on the same device.
#include <sys/random.h>

#include <cerrno>
#include <chrono>
#include <cstring>
#include <vector>

#include "devcall.h"
#include "keccak.h"
#include "msm.h"
#include "transcript.h"
#include "verify.h"

namespace nzcb {

namespace {

constexpr unsigned kTermBlock = 64;      // one wavefront per workgroup: 20 N lanes spread over the CUs
constexpr size_t kMaxTerms = size_t(1) << 24;

// terms[i] = scalars[i] * points[i]; grid covers n (no stride loop: n <= kMaxTerms)
__global__ __launch_bounds__(kTermBlock) void k_g1_term_mul(const uint32_t* __restrict__ points,
                                                             const uint32_t* __restrict__ scalars,
                                                             G1xyzz* __restrict__ terms, uint32_t n) {
  const uint32_t i = blockIdx.x * kTermBlock + threadIdx.x;
  if (i >= n) return;
  terms[i] = g1_term_mul(points + size_t(16) * i, scalars + size_t(8) * i);
}

// out[g] = affine sum of terms[group_end[g - 1], group_end[g])
__global__ __launch_bounds__(kTermBlock) void k_g1_group_sum(const G1xyzz* __restrict__ terms,
                                                              const uint32_t* __restrict__ group_end,
                                                              uint32_t* __restrict__ out, uint32_t groups) {
  const uint32_t g = blockIdx.x * kTermBlock + threadIdx.x;
  if (g >= groups) return;
  const uint32_t lo = g ? group_end[g - 1] : 0u;
  g1_group_sum(terms, lo, group_end[g], out + size_t(16) * g);
}

// phases of the calling thread's last batch (nzcb_debug_verify_batch_timings)
thread_local double g_times[6] = {0, 0, 0, 0, 0, 0};

size_t check_groups(const uint32_t* group_end, size_t groups) {
  uint32_t prev = 0;
  for (size_t g = 0; g < groups; g++) {
    if (group_end[g] < prev) throw Error(NZCB_ERR_ARG, "group ends must not decrease");
    prev = group_end[g];
  }
  if (prev > kMaxTerms || groups > kMaxTerms) throw Error(NZCB_ERR_ARG, "too many terms (limit 2^24)");
  return prev;
}

void g1_lincomb_host(const uint8_t* points, const uint8_t* scalars, const uint32_t* group_end, size_t groups,
                     uint8_t* out) {
  const size_t n = check_groups(group_end, groups);
  std::vector<G1xyzz> terms(n);
  for (size_t i = 0; i < n; i++) {
    uint32_t pt[16], sc[8];
    std::memcpy(pt, points + 64 * i, 64);
    std::memcpy(sc, scalars + 32 * i, 32);
    terms[i] = g1_term_mul(pt, sc);
  }
  for (size_t g = 0; g < groups; g++) {
    uint32_t o[16];
    g1_group_sum(terms.data(), g ? group_end[g - 1] : 0u, group_end[g], o);
    std::memcpy(out + 64 * g, o, 64);
  }
}

void g1_lincomb_device(int device, const uint8_t* points, const uint8_t* scalars, const uint32_t* group_end,
                       size_t groups, uint8_t* out) {
  const size_t n = check_groups(group_end, groups);
  g_times[2] = g_times[3] = 0;
  if (!groups) return;
  CallScope cs(device, nullptr, 3);
  BlockLayout lay;
  const size_t o_pts = lay.take(64 * n), o_sc = lay.take(32 * n), o_ge = lay.take(4 * groups),
               o_terms = lay.take(sizeof(G1xyzz) * n), o_out = lay.take(64 * groups);
  char* d = cs.alloc<char>(lay.total);
  if (n) {
    NZ_HIP(hipMemcpyAsync(d + o_pts, points, 64 * n, hipMemcpyHostToDevice, cs.st));
    NZ_HIP(hipMemcpyAsync(d + o_sc, scalars, 32 * n, hipMemcpyHostToDevice, cs.st));
  }
  NZ_HIP(hipMemcpyAsync(d + o_ge, group_end, 4 * groups, hipMemcpyHostToDevice, cs.st));
  cs.record(0);
  if (n)
    k_g1_term_mul<<<grid_for(n, kTermBlock, 1u << 20), kTermBlock, 0, cs.st>>>(
        reinterpret_cast<const uint32_t*>(d + o_pts), reinterpret_cast<const uint32_t*>(d + o_sc),
        reinterpret_cast<G1xyzz*>(d + o_terms), (uint32_t)n);
  cs.record(1);
  k_g1_group_sum<<<grid_for(groups, kTermBlock, 1u << 20), kTermBlock, 0, cs.st>>>(
      reinterpret_cast<const G1xyzz*>(d + o_terms), reinterpret_cast<const uint32_t*>(d + o_ge),
      reinterpret_cast<uint32_t*>(d + o_out), (uint32_t)groups);
  cs.record(2);
  NZ_HIP(hipGetLastError());
  NZ_HIP(hipMemcpyAsync(out, d + o_out, 64 * groups, hipMemcpyDeviceToHost, cs.st));
  NZ_HIP(hipStreamSynchronize(cs.st));
  g_times[2] = cs.elapsed(0, 1);
  g_times[3] = cs.elapsed(1, 2);
}

void g1_lincomb(int device, const uint8_t* points, const uint8_t* scalars, const uint32_t* group_end, size_t groups,
                uint8_t* out) {
  if (device == NZCB_VERIFY_HOST)
    g1_lincomb_host(points, scalars, group_end, groups, out);
  else
    g1_lincomb_device(device, points, scalars, group_end, groups, out);
}

void os_random(uint8_t* b, size_t len) {
  size_t got = 0;
  while (got < len) {
    const ssize_t k = getrandom(b + got, len - got, 0);
    if (k < 0) {
      if (errno == EINTR || errno == EAGAIN) continue;
      throw Error(NZCB_ERR_INTERNAL, std::string("getrandom failed: ") + std::strerror(errno) +
                                         " (no entropy for the batch weights)");
    }
    got += (size_t)k;
  }
}

// rho_i: 128 bits, never zero, Montgomery form
Fr batch_weight(const uint8_t* seed, uint32_t i) {
  uint8_t le[32] = {0};
  if (seed) {
    uint8_t in[36], h[32];
    std::memcpy(in, seed, 32);
    std::memcpy(in + 32, &i, 4);
    keccak256(in, sizeof(in), h);
    for (int k = 0; k < 16; k++) le[k] = h[31 - k];  // the digest as a big-endian integer, low 128 bits
  } else {
    os_random(le, 16);
  }
  bool zero = true;
  for (int k = 0; k < 16; k++) zero = zero && !le[k];
  if (zero) le[0] = 1;
  return fr_from_le_normal(le);
}

double ms_since(const std::chrono::steady_clock::time_point& t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

struct Bisect {
  const Vk& vk;
  const std::vector<int>& idx;       // the items that passed step (a)
  const std::vector<G1Affine>& lr;   // L'_k, R'_k of idx[k]
  int* valid;
  int checks = 0;

  bool check(size_t lo, size_t hi) {
    G1xyzz l = G1xyzz::inf(), r = G1xyzz::inf();
    for (size_t k = lo; k < hi; k++) {
      if (!lr[2 * k].is_inf()) l = xyzz_add_affine(l, lr[2 * k].x, lr[2 * k].y);
      if (!lr[2 * k + 1].is_inf()) r = xyzz_add_affine(r, lr[2 * k + 1].x, lr[2 * k + 1].y);
    }
    checks++;
    return pairing_check({{g1_neg(xyzz_to_affine(l)), vk.x2}, {xyzz_to_affine(r), g2_generator()}});
  }
  void mark(size_t lo, size_t hi, int v) {
    for (size_t k = lo; k < hi; k++) valid[idx[k]] = v;
  }
  // known_bad: the range's own check has failed, or follows from its sibling's passing
  void solve(size_t lo, size_t hi, bool known_bad) {
    if (lo >= hi) return;
    if (!known_bad && check(lo, hi)) return mark(lo, hi, 1);
    if (hi - lo == 1) return mark(lo, hi, 0);
    const size_t mid = lo + (hi - lo) / 2;
    if (check(lo, mid)) {
      mark(lo, mid, 1);
      solve(mid, hi, true);
    } else {
      solve(lo, mid, true);
      solve(mid, hi, false);
    }
  }
};

void verify_batch(const uint8_t* vkb, const uint8_t* proofs, const uint8_t* pubs, size_t pub_stride, int n_public,
                  int count, bool transcript_public, int device, const uint8_t* seed, int* valid_out,
                  uint8_t* points_out, int* pairing_checks) {
  if (count < 0 || n_public < 0 || !vkb || (count && (!proofs || !valid_out)) ||
      (count && n_public && (!pubs || pub_stride < 32 * (size_t)n_public)))
    throw Error(NZCB_ERR_ARG, "bad argument");
  if ((size_t)count > kMaxTerms / (kVerifyLTerms + kVerifyRTerms)) throw Error(NZCB_ERR_ARG, "batch too large");
  bool ok = true;
  const Vk vk = vk_read(vkb, &ok);
  if (!ok) throw Error(NZCB_ERR_FORMAT, "invalid verification key");
  for (auto& t : g_times) t = 0;
  if (pairing_checks) *pairing_checks = 0;
  if (points_out) std::memset(points_out, 0, 128 * (size_t)count);
  // steps (a), (b) and the weights
  auto t0 = std::chrono::steady_clock::now();
  constexpr int kT = kVerifyLTerms + kVerifyRTerms;
  std::vector<int> idx;
  std::vector<uint8_t> pts, scs;
  std::vector<uint32_t> ends;
  ProofParsed pp;
  VerifyTerms tm;
  for (int i = 0; i < count; i++) {
    valid_out[i] = 0;
    if (!plonk_parse(vk, proofs + (size_t)NZCB_PROOF_BYTES * i, pubs ? pubs + pub_stride * i : nullptr, n_public, &pp))
      continue;
    plonk_terms(vk, pp, transcript_public, &tm);
    const Fr rho = batch_weight(seed, (uint32_t)i);
    const size_t k = idx.size();
    idx.push_back(i);
    pts.resize(64 * kT * (k + 1));
    scs.resize(32 * kT * (k + 1));
    uint8_t* p = pts.data() + 64 * kT * k;
    uint8_t* s = scs.data() + 32 * kT * k;
    for (int j = 0; j < kVerifyLTerms; j++, p += 64, s += 32) {
      g1_to_le(tm.lp[j], p);
      fr_to_le_normal(tm.ls[j] * rho, s);
    }
    for (int j = 0; j < kVerifyRTerms; j++, p += 64, s += 32) {
      g1_to_le(tm.rp[j], p);
      fr_to_le_normal(tm.rs[j] * rho, s);
    }
    ends.push_back((uint32_t)(kT * k + kVerifyLTerms));
    ends.push_back((uint32_t)(kT * (k + 1)));
  }
  g_times[0] = ms_since(t0);
  if (idx.empty()) return;
  // L'_i, R'_i
  t0 = std::chrono::steady_clock::now();
  std::vector<uint8_t> out(128 * idx.size());
  g1_lincomb(device, pts.data(), scs.data(), ends.data(), ends.size(), out.data());
  g_times[1] = ms_since(t0);
  std::vector<G1Affine> lr(2 * idx.size());
  for (size_t k = 0; k < lr.size(); k++) {
    lr[k] = g1_from_le(out.data() + 64 * k, &ok);
    if (!ok) throw Error(NZCB_ERR_INTERNAL, "group sums are not canonical");
  }
  if (points_out)
    for (size_t k = 0; k < idx.size(); k++) std::memcpy(points_out + 128 * (size_t)idx[k], out.data() + 128 * k, 128);
  // one pairing check; bisection when it fails
  t0 = std::chrono::steady_clock::now();
  Bisect bs{vk, idx, lr, valid_out};
  bs.solve(0, idx.size(), false);
  g_times[4] = ms_since(t0);
  g_times[5] = bs.checks;
  if (pairing_checks) *pairing_checks = bs.checks;
}

}  // namespace

}  // namespace nzcb

using namespace nzcb;

extern "C" {

int nzcb_engine_g1_lincomb(int device, const uint8_t* points, const uint8_t* scalars, const uint32_t* group_end,
                           size_t groups, uint8_t* out, nzcb_err* err) {
  return guarded(err, [&] {
    if (groups && (!group_end || !out)) throw Error(NZCB_ERR_ARG, "null argument");
    if (groups && group_end[groups - 1] && (!points || !scalars)) throw Error(NZCB_ERR_ARG, "null argument");
    g1_lincomb(device, points, scalars, group_end, groups, out);
  });
}

int nzcb_engine_verify_batch(const uint8_t* vk, const uint8_t* proofs, const uint8_t* pubs, size_t pub_stride,
                             int n_public, int count, int transcript_public, int device, const uint8_t* seed,
                             int* valid_out, uint8_t* points_out, int* pairing_checks, nzcb_err* err) {
  return guarded(err, [&] {
    verify_batch(vk, proofs, pubs, pub_stride, n_public, count, transcript_public != 0, device, seed, valid_out,
                 points_out, pairing_checks);
  });
}

int nzcb_debug_verify_batch_timings(double* ms, int cap) {
  int k = 0;
  for (; ms && k < cap && k < 6; k++) ms[k] = g_times[k];
  return k;
}

int nzcb_verify_batch(const uint8_t* vk, const uint8_t* proofs, const uint8_t* pubs, size_t pub_stride, int n_public,
                      int count, int transcript_public, int device, const uint8_t* seed, int* valid_out,
                      nzcb_err* err) {
  return nzcb_engine_verify_batch(vk, proofs, pubs, pub_stride, n_public, count, transcript_public, device, seed,
                                  valid_out, nullptr, nullptr, err);
}

}  // extern "C"
