// Powers of tau: new, contribute and prepare phase 2 (include/nzcb.h nzcb_ptau_new,
// nzcb_ptau_contribute, nzcb_ptau_prepare_phase2): what the kernels of ptau_ops.hip and the
// host path (NZCB_PTAU_HOST) share, and the reader and writer of the file's sections.
//
// NZ_HD functions compile for the device and for the host from this one text: Fq2, a point in
// XYZZ coordinates over either field (G1 over Fq, G2 over Fq2, the formulas of ec.h with the
// same complete special cases), the 254-bit scalar multiplication, the point tests and the
// scalar a lane derives for its index. The header needs no HIP runtime: a host-only program may
// include it (tests/native/ptau_ops_host.cpp).
#pragma once
#include <sys/random.h>

#include <algorithm>
#include <cerrno>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "capi_guard.h"
#include "ec.h"
#include "field.h"
#include "key_check.h"

namespace nzcb {

// ---------------------------------------------------------------- Fq2 = Fq[u] / (u^2 + 1)
struct Fq2 {
  Fq c0, c1;
  NZ_HD static Fq2 zero() { return {Fq::zero(), Fq::zero()}; }
  NZ_HD static Fq2 one() { return {Fq::one(), Fq::zero()}; }
  NZ_HD bool is_zero() const { return c0.is_zero() && c1.is_zero(); }
  NZ_HD bool operator==(const Fq2& o) const { return c0 == o.c0 && c1 == o.c1; }
};
NZ_HD Fq2 operator+(const Fq2& a, const Fq2& b) { return {a.c0 + b.c0, a.c1 + b.c1}; }
NZ_HD Fq2 operator-(const Fq2& a, const Fq2& b) { return {a.c0 - b.c0, a.c1 - b.c1}; }
NZ_HD Fq2 neg(const Fq2& a) { return {neg(a.c0), neg(a.c1)}; }
NZ_HD Fq2 dbl(const Fq2& a) { return {dbl(a.c0), dbl(a.c1)}; }
// three base-field products (Karatsuba)
NZ_HD Fq2 operator*(const Fq2& a, const Fq2& b) {
  const Fq t0 = a.c0 * b.c0, t1 = a.c1 * b.c1;
  const Fq m = (a.c0 + a.c1) * (b.c0 + b.c1);
  return {t0 - t1, m - t0 - t1};
}
// two: (a0 + a1)(a0 - a1) + 2 a0 a1 u
NZ_HD Fq2 sqr(const Fq2& a) {
  const Fq p = a.c0 * a.c1;
  return {(a.c0 + a.c1) * (a.c0 - a.c1), dbl(p)};
}
// conj(a) / (a0^2 + a1^2); the inverse of zero is zero
NZ_HD Fq2 inverse(const Fq2& a) {
  const Fq d = inverse(sqr(a.c0) + sqr(a.c1));
  return {a.c0 * d, neg(a.c1) * d};
}

// ---------------------------------------------------------------- points over F = Fq or Fq2
// affine, the file's layout: G1 x || y (64 B), G2 x.c0 || x.c1 || y.c0 || y.c1 (128 B), LE
// Montgomery; all zero bytes is the point at infinity
template <class F>
struct PtAffine {
  F x, y;
  NZ_HD bool is_inf() const { return x.is_zero() && y.is_zero(); }
};
// x = X / ZZ, y = Y / ZZZ; ZZ = 0 is the point at infinity (ec.h G1xyzz)
template <class F>
struct PtXyzz {
  F X, Y, ZZ, ZZZ;
  NZ_HD static PtXyzz inf() { return {F::one(), F::one(), F::zero(), F::zero()}; }
  NZ_HD bool is_inf() const { return ZZ.is_zero(); }
};
using G1Pt = PtAffine<Fq>;
using G2Pt = PtAffine<Fq2>;
static_assert(sizeof(G1Pt) == 64 && sizeof(G2Pt) == 128, "the file's point layouts");

template <class F>
NZ_HD PtXyzz<F> pt_from_affine(const PtAffine<F>& p) {
  if (p.is_inf()) return PtXyzz<F>::inf();
  return {p.x, p.y, F::one(), F::one()};
}
// dbl-2008-s-1 (a = 0)
template <class F>
NZ_HD PtXyzz<F> pt_dbl(const PtXyzz<F>& p) {
  if (p.is_inf() || p.Y.is_zero()) return PtXyzz<F>::inf();
  const F U = dbl(p.Y);
  const F V = sqr(U);
  const F W = U * V;
  const F S = p.X * V;
  const F X2 = sqr(p.X);
  const F M = X2 + dbl(X2);
  PtXyzz<F> r;
  r.X = sqr(M) - dbl(S);
  r.Y = M * (S - r.X) - W * p.Y;
  r.ZZ = V * p.ZZ;
  r.ZZZ = W * p.ZZZ;
  return r;
}
// madd-2008-s: p + (qx, qy), the affine point not infinity
template <class F>
NZ_HD PtXyzz<F> pt_add_affine(const PtXyzz<F>& p, const F& qx, const F& qy) {
  if (p.is_inf()) return {qx, qy, F::one(), F::one()};
  const F P = qx * p.ZZ - p.X;
  const F R = qy * p.ZZZ - p.Y;
  if (P.is_zero()) {
    if (R.is_zero()) return pt_dbl(PtXyzz<F>{qx, qy, F::one(), F::one()});
    return PtXyzz<F>::inf();
  }
  const F PP = sqr(P);
  const F PPP = P * PP;
  const F Q = p.X * PP;
  PtXyzz<F> r;
  r.X = sqr(R) - PPP - dbl(Q);
  r.Y = R * (Q - r.X) - p.Y * PPP;
  r.ZZ = p.ZZ * PP;
  r.ZZZ = p.ZZZ * PPP;
  return r;
}
// add-2008-s
template <class F>
NZ_HD PtXyzz<F> pt_add(const PtXyzz<F>& p, const PtXyzz<F>& q) {
  if (p.is_inf()) return q;
  if (q.is_inf()) return p;
  const F U1 = p.X * q.ZZ;
  const F S1 = p.Y * q.ZZZ;
  const F P = q.X * p.ZZ - U1;
  const F R = q.Y * p.ZZZ - S1;
  if (P.is_zero()) {
    if (R.is_zero()) return pt_dbl(p);
    return PtXyzz<F>::inf();
  }
  const F PP = sqr(P);
  const F PPP = P * PP;
  const F Q = U1 * PP;
  PtXyzz<F> r;
  r.X = sqr(R) - PPP - dbl(Q);
  r.Y = R * (Q - r.X) - S1 * PPP;
  r.ZZ = p.ZZ * q.ZZ * PP;
  r.ZZZ = p.ZZZ * q.ZZZ * PPP;
  return r;
}
template <class F>
NZ_HD PtXyzz<F> pt_neg(const PtXyzz<F>& p) {
  return {p.X, neg(p.Y), p.ZZ, p.ZZZ};
}
// k p for a normal-form scalar below 2^254 (double-and-add, MSB first)
template <class F>
NZ_HD PtXyzz<F> pt_mul(const PtXyzz<F>& p, const Fr& k) {
  PtXyzz<F> r = PtXyzz<F>::inf();
  for (int b = 253; b >= 0; b--) {
    r = pt_dbl(r);
    if ((k.v[b >> 5] >> (b & 31)) & 1u) r = pt_add(r, p);
  }
  return r;
}
// the same with the affine point as the mixed addend
template <class F>
NZ_HD PtXyzz<F> pt_mul_affine(const PtAffine<F>& p, const Fr& k) {
  PtXyzz<F> r = PtXyzz<F>::inf();
  if (p.is_inf()) return r;
  for (int b = 253; b >= 0; b--) {
    r = pt_dbl(r);
    if ((k.v[b >> 5] >> (b & 31)) & 1u) r = pt_add_affine(r, p.x, p.y);
  }
  return r;
}
// one inversion: ZZ^3 = ZZZ^2, so (ZZ / ZZZ)^2 = 1 / ZZ
template <class F>
NZ_HD PtAffine<F> pt_to_affine(const PtXyzz<F>& p) {
  if (p.is_inf()) return {F::zero(), F::zero()};
  const F izzz = inverse(p.ZZZ);
  const F izz = sqr(p.ZZ * izzz);
  return {p.X * izz, p.Y * izzz};
}

// ---------------------------------------------------------------- point tests
// G2: w = x.c0 || x.c1 || y.c0 || y.c1 as 32 LE words. b2 = 3 / (9 + u), the twist's constant.
// NZCB_KEY_OK, NZCB_KEY_ERR_RANGE (a stored word >= q) or NZCB_KEY_ERR_CURVE ((0, 0) or
// y^2 != x^3 + b2). Membership of the subgroup of order r is NOT tested.
NZ_HD int g2_point_status(const uint32_t* w, const Fq2& b2) {
  Fq c[4];
  bool in_range = true, zero = true;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    uint32_t br = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      c[k].v[i] = w[8 * k + i];
      (void)subb(w[8 * k + i], FqParams::P[i], br);
    }
    in_range = in_range && br;
    zero = zero && c[k].is_zero();
  }
  if (!in_range) return NZCB_KEY_ERR_RANGE;
  if (zero) return NZCB_KEY_ERR_CURVE;
  const Fq2 x{c[0], c[1]}, y{c[2], c[3]};
  return sqr(y) == sqr(x) * x + b2 ? NZCB_KEY_OK : NZCB_KEY_ERR_CURVE;
}
template <class F>
NZ_HD int pt_status(const PtAffine<F>* p, const Fq2& b2);
template <>
NZ_HD int pt_status<Fq>(const PtAffine<Fq>* p, const Fq2&) {
  return srs_point_status(reinterpret_cast<const uint32_t*>(p));
}
template <>
NZ_HD int pt_status<Fq2>(const PtAffine<Fq2>* p, const Fq2& b2) {
  return g2_point_status(reinterpret_cast<const uint32_t*>(p), b2);
}

// the scalar of point i of a contribution: c tau^i, normal form (c, tau Montgomery)
NZ_HD Fr ptau_scalar(const Fr& c, const Fr& tau, uint64_t i) { return from_mont(c * pow_u64(tau, i)); }

// ---------------------------------------------------------------- host constants
inline Fq fq_of_words(const uint32_t l[8]) {
  Fq x;
  for (int i = 0; i < 8; i++) x.v[i] = l[i];
  return to_mont(x);
}
inline Fq fq_small(uint32_t k) {
  Fq x = Fq::zero();
  x.v[0] = k;
  return to_mont(x);
}
inline Fq2 g2_twist_b() {
  const Fq2 d = inverse(Fq2{fq_small(9), Fq::one()});
  const Fq three = fq_small(3);
  return {d.c0 * three, d.c1 * three};
}
inline G1Pt g1_gen_point() { return {Fq::one(), dbl(Fq::one())}; }
inline G2Pt g2_gen_point() {
  static const uint32_t X0[8] = {0xd992f6edu, 0x46debd5cu, 0xf75edaddu, 0x674322d4u,
                                 0x5e5c4479u, 0x426a0066u, 0x121f1e76u, 0x1800deefu};
  static const uint32_t X1[8] = {0xaef312c2u, 0x97e485b7u, 0x35a9e712u, 0xf1aa4933u,
                                 0x31fb5d25u, 0x7260bfb7u, 0x920d483au, 0x198e9393u};
  static const uint32_t Y0[8] = {0x66fa7daau, 0x4ce6cc01u, 0x0c43d37bu, 0xe3d1e769u,
                                 0x8dcb408fu, 0x4aab7180u, 0xdb8c6debu, 0x12c85ea5u};
  static const uint32_t Y1[8] = {0xd122975bu, 0x55acdadcu, 0x70b38ef3u, 0xbc4b3133u,
                                 0x690c3395u, 0xec9e99adu, 0x585ff075u, 0x090689d0u};
  return {{fq_of_words(X0), fq_of_words(X1)}, {fq_of_words(Y0), fq_of_words(Y1)}};
}
// w_(2^k) of ntt.h's fr_root_of_unity (Montgomery): 5^((r - 1) / 2^28) squared down
inline Fr ptau_root_of_unity(int k) {
  static const uint32_t w28[8] = {0x725b19f0u, 0x9bd61b6eu, 0x41112ed4u, 0x402d111eu,
                                  0x8ef62abcu, 0x00e0a7ebu, 0xa58a7e85u, 0x2a3c09f0u};
  Fr w;
  for (int i = 0; i < 8; i++) w.v[i] = w28[i];
  w = to_mont(w);
  for (int j = 28; j > k; j--) w = sqr(w);
  return w;
}
// 1 / 2^k, normal form
inline Fr ptau_inv_n(int k) {
  Fr n = Fr::zero();
  n.v[k >> 5] = 1u << (k & 31);
  return from_mont(inverse(to_mont(n)));
}

// ---------------------------------------------------------------- the file (host)
constexpr int kPtauMinPower = 1, kPtauMaxPower = 24;

// Sections 1-7 of a powers-of-tau file, every length checked in 64 bits against the header's
// power. NZCB_ERR_FORMAT for a missing or short section, NZCB_ERR_ARG for a power outside 1..24.
struct PtauSections {
  uint32_t power = 0;
  KeySection s[8];  // by section id; s[0] unused
  uint64_t points(int id) const {
    const uint64_t n = uint64_t(1) << power;
    return id == 2 ? 2 * n - 1 : id == 6 ? 1 : n;
  }
  static bool is_g2(int id) { return id == 3 || id == 6 || id == 13; }
  static uint64_t point_bytes(int id) { return is_g2(id) ? 128 : 64; }
};
inline PtauSections ptau_sections_open(const uint8_t* d, size_t len) {
  PtauSections f;
  for (uint32_t id = 1; id <= 7; id++) {
    f.s[id] = key_find_section(d, len, "ptau", id);
    if (!f.s[id].p) throw Error(NZCB_ERR_FORMAT, "ptau: section " + std::to_string(id) + " is missing");
  }
  const KeySection& h = f.s[1];
  uint32_t n8 = 0;
  if (h.len < 44) throw Error(NZCB_ERR_FORMAT, "ptau: header too short");
  std::memcpy(&n8, h.p, 4);
  if (n8 != 32 || std::memcmp(h.p + 4, FqParams::P, 32) != 0)
    throw Error(NZCB_ERR_FORMAT, "ptau: not a bn128 powers of tau file");
  std::memcpy(&f.power, h.p + 36, 4);
  if (f.power < (uint32_t)kPtauMinPower || f.power > (uint32_t)kPtauMaxPower)
    throw Error(NZCB_ERR_ARG, "ptau: power must be in 1..24");
  for (int id = 2; id <= 6; id++)
    if (f.s[id].len / PtauSections::point_bytes(id) < f.points(id))
      throw Error(NZCB_ERR_FORMAT, "ptau: section " + std::to_string(id) + " is shorter than the header's power");
  if (f.s[7].len < 4) throw Error(NZCB_ERR_FORMAT, "ptau: contributions section too short");
  return f;
}

// The bytes an operation writes: a malloc'ed block (the caller's, after release()) or a file
// mapped for writing, removed again unless commit() was reached.
struct PtauOut {
  uint8_t* p = nullptr;
  uint64_t len = 0, at = 0;
  int fd = -1;
  std::string path;
  bool done = false;

  PtauOut() = default;
  PtauOut(const PtauOut&) = delete;
  PtauOut& operator=(const PtauOut&) = delete;
  // path NULL: in memory
  void open(const char* out_path, uint64_t bytes) {
    len = bytes;
    if (bytes > SIZE_MAX / 2) throw Error(NZCB_ERR_ARG, "ptau: output too large for this host");
    if (!out_path) {
      p = static_cast<uint8_t*>(std::malloc((size_t)bytes));
      if (!p) throw Error(NZCB_ERR_INTERNAL, "out of host memory");
      return;
    }
    path = out_path;
    fd = ::open(out_path, O_RDWR | O_CREAT | O_TRUNC, 0644);
    if (fd < 0) throw Error(NZCB_ERR_ARG, std::string("cannot create ") + out_path);
    if (ftruncate(fd, (off_t)bytes) != 0) throw Error(NZCB_ERR_INTERNAL, std::string("cannot size ") + out_path);
    void* m = mmap(nullptr, (size_t)bytes, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
    if (m == MAP_FAILED) throw Error(NZCB_ERR_INTERNAL, "mmap of the output failed");
    p = static_cast<uint8_t*>(m);
  }
  void put(const void* src, uint64_t n) {
    if (n > len - at) throw Error(NZCB_ERR_INTERNAL, "ptau: output overrun");
    if (n) std::memcpy(p + at, src, (size_t)n);
    at += n;
  }
  void put_u32(uint32_t v) { put(&v, 4); }
  void put_u64(uint64_t v) { put(&v, 8); }
  void file_header(uint32_t n_sections) {
    put("ptau", 4);
    put_u32(1);
    put_u32(n_sections);
  }
  // the section's table entry; its payload (bytes long) begins at the returned pointer
  uint8_t* section(uint32_t id, uint64_t bytes) {
    put_u32(id);
    put_u64(bytes);
    if (bytes > len - at) throw Error(NZCB_ERR_INTERNAL, "ptau: output overrun");
    uint8_t* at_p = p + at;
    at += bytes;
    return at_p;
  }
  void commit() {
    if (at != len) throw Error(NZCB_ERR_INTERNAL, "ptau: output size mismatch");
    done = true;
  }
  uint8_t* release() {  // in memory only
    uint8_t* r = p;
    p = nullptr;
    return r;
  }
  ~PtauOut() {
    if (fd >= 0) {
      if (p) munmap(p, (size_t)len);
      close(fd);
      if (!done) unlink(path.c_str());
    } else {
      std::free(p);
    }
  }
};

inline void ptau_put_header(PtauOut& o, uint32_t power) {
  uint8_t* h = o.section(1, 44);
  const uint32_t n8 = 32;
  std::memcpy(h, &n8, 4);
  std::memcpy(h + 4, FqParams::P, 32);
  std::memcpy(h + 36, &power, 4);
  std::memcpy(h + 40, &power, 4);
}

// bytes of sections 1-7 with their table entries, after the 12-byte file header
inline uint64_t ptau_base_bytes(uint32_t power, uint64_t s1_len, uint64_t s7_len) {
  const uint64_t n = uint64_t(1) << power;
  return 7 * 12 + s1_len + 64 * (2 * n - 1) + 128 * n + 64 * n + 64 * n + 128 + s7_len;
}

// nzcb_ptau_new: every point its group's generator, no contributions
inline void ptau_new(int power, PtauOut& o, const char* out_path) {
  if (power < kPtauMinPower || power > kPtauMaxPower) throw Error(NZCB_ERR_ARG, "ptau: power must be in 1..24");
  const uint64_t n = uint64_t(1) << power;
  o.open(out_path, 12 + ptau_base_bytes((uint32_t)power, 44, 4));
  o.file_header(7);
  ptau_put_header(o, (uint32_t)power);
  const G1Pt g1 = g1_gen_point();
  const G2Pt g2 = g2_gen_point();
  auto fill = [&](uint32_t id, uint64_t count, const void* pt, uint64_t bytes) {
    uint8_t* s = o.section(id, count * bytes);
    for (uint64_t i = 0; i < count; i++) std::memcpy(s + i * bytes, pt, (size_t)bytes);
  };
  fill(2, 2 * n - 1, &g1, 64);
  fill(3, n, &g2, 128);
  fill(4, n, &g1, 64);
  fill(5, n, &g1, 64);
  fill(6, 1, &g2, 128);
  const uint32_t none = 0;
  std::memcpy(o.section(7, 4), &none, 4);
  o.commit();
}

// ---------------------------------------------------------------- what the host paths share
// (ptau_ops.hip and groth16.h)
inline void wipe(void* p, size_t n) {
  volatile uint8_t* b = static_cast<volatile uint8_t*>(p);
  for (size_t i = 0; i < n; i++) b[i] = 0;
}

struct Tally {  // defective points and the lowest one's key (key_check.h srs_bad_key)
  uint64_t n_bad = 0, key = kNoBadKey;
};

// fn(i) for i < n on up to 16 threads of the host
template <class Fn>
void parallel_for(uint64_t n, Fn fn) {
  const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
  const unsigned nt = (unsigned)std::min<uint64_t>(std::min(16u, hw), n / 4);
  if (nt <= 1) {
    for (uint64_t i = 0; i < n; i++) fn(i);
    return;
  }
  std::vector<std::thread> th;
  for (unsigned t = 0; t < nt; t++) {
    const uint64_t lo = n * t / nt, hi = n * (t + 1) / nt;
    th.emplace_back([lo, hi, &fn] {
      for (uint64_t i = lo; i < hi; i++) fn(i);
    });
  }
  for (auto& t : th) t.join();
}

inline void os_random(uint8_t* b, size_t len) {
  size_t got = 0;
  while (got < len) {
    const ssize_t k = getrandom(b + got, len - got, 0);
    if (k < 0) {
      if (errno == EINTR || errno == EAGAIN) continue;
      throw Error(NZCB_ERR_INTERNAL, std::string("getrandom failed: ") + std::strerror(errno));
    }
    got += (size_t)k;
  }
}

// `count` <= 3 secrets in Montgomery form (a powers-of-tau contribution: tau, alpha, beta; a
// Groth16 zkey contribution: the one factor of delta). given: count x 32 B LE, each in [1, r)
// (NZCB_ERR_ARG "<what>: a secret is zero or not below r" otherwise). NULL: keccak256(random ||
// entropy || k) for k < count (one byte), the digest read as a big-endian integer mod r, with 96
// fresh bytes from the OS until none of them is zero.
inline void make_secrets(const uint8_t* given, const uint8_t* entropy, size_t entropy_len, Fr* out, int count = 3,
                         const char* what = "ptau") {
  if (given) {
    for (int k = 0; k < count; k++) {
      Fr s;
      std::memcpy(s.v, given + 32 * k, 32);
      const bool ok = !s.is_zero() && !fr_noncanonical(s.v);
      out[k] = ok ? to_mont(s) : Fr::zero();
      wipe(&s, sizeof s);
      if (!ok) {
        wipe(out, (size_t)count * sizeof(Fr));
        throw Error(NZCB_ERR_ARG, std::string(what) + ": a secret is zero or not below r");
      }
    }
    return;
  }
  if (entropy_len && !entropy) throw Error(NZCB_ERR_ARG, "null argument");
  std::vector<uint8_t> msg(96 + entropy_len + 1);
  if (entropy_len) std::memcpy(msg.data() + 96, entropy, entropy_len);
  for (bool again = true; again;) {
    again = false;
    os_random(msg.data(), 96);
    for (int k = 0; k < count; k++) {
      uint8_t dg[32];
      msg.back() = (uint8_t)k;
      keccak256(msg.data(), msg.size(), dg);
      Fr s;
      for (int i = 0; i < 8; i++)
        s.v[i] = (uint32_t)dg[31 - 4 * i] | (uint32_t)dg[30 - 4 * i] << 8 | (uint32_t)dg[29 - 4 * i] << 16 |
                 (uint32_t)dg[28 - 4 * i] << 24;
      for (int i = 0; i < 6; i++) s = reduce_once(s);  // 2^256 < 6 r
      again = again || s.is_zero();
      out[k] = to_mont(s);
      wipe(&s, sizeof s);
      wipe(dg, sizeof dg);
    }
  }
  wipe(msg.data(), msg.size());
}

}  // namespace nzcb
