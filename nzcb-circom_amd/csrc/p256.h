// NIST P-256 (secp256r1) arithmetic for ECDSA verification: the fields F_p and F_n on 8 x 32-bit
// limbs and the curve y^2 = x^3 - 3x + b, as NZ_HD functions, so that the host path and the
// kernels of p256_verify.hip run the same code.
//
// Why not field.h / ec.h: both moduli here are full width (p, n > 2^255). A sum of two reduced
// values and the Montgomery product before its final subtraction (< 2m) can reach 2^256, which
// field.h's operator+ and operator* drop (they are right for BN254's 254-bit moduli only), and
// ec.h's formulas are for a = 0. Everything here keeps the ninth word: add and mul carry it into
// the conditional subtraction.
//
// Representation: Montgomery, x 2^256 mod m, product scanning with the 96-bit column accumulator
// of field.h (one v_mad_u64_u32 and a carry add per partial product on the device). For p,
// -p^-1 mod 2^32 = 1: the quotient digit of a column is the column's low word, no multiplication.
// A Solinas reduction would serve p alone; Montgomery serves p and n (which has no special form)
// with one routine, and s^-1 mod n costs about as many products as the table additions mod p
// (DESIGN.md "Pass signature").
//
// Verification handles public data only (public key, signature, digest): branches and table
// reads depend on the data, and nothing here is constant time. Do not sign with it.
#pragma once
#include "field.h"

namespace nzcb {
namespace p256 {

struct PParams {  // the field prime p = 2^256 - 2^224 + 2^192 + 2^96 - 1
  static constexpr uint32_t P[8] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0x00000000u,
                                    0x00000000u, 0x00000000u, 0x00000001u, 0xffffffffu};
  static constexpr uint32_t INV = 0x00000001u;  // -p^-1 mod 2^32
  static constexpr uint32_t ONE[8] = {0x00000001u, 0x00000000u, 0x00000000u, 0xffffffffu,
                                      0xffffffffu, 0xffffffffu, 0xfffffffeu, 0x00000000u};
  static constexpr uint32_t R2[8] = {0x00000003u, 0x00000000u, 0xffffffffu, 0xfffffffbu,
                                     0xfffffffeu, 0xffffffffu, 0xfffffffdu, 0x00000004u};
};

struct NParams {  // the group order n
  static constexpr uint32_t P[8] = {0xfc632551u, 0xf3b9cac2u, 0xa7179e84u, 0xbce6faadu,
                                    0xffffffffu, 0xffffffffu, 0x00000000u, 0xffffffffu};
  static constexpr uint32_t INV = 0xee00bc4fu;
  static constexpr uint32_t ONE[8] = {0x039cdaafu, 0x0c46353du, 0x58e8617bu, 0x43190552u,
                                      0x00000000u, 0x00000000u, 0xffffffffu, 0x00000000u};
  static constexpr uint32_t R2[8] = {0xbe79eea2u, 0x83244c95u, 0x49bd6fa6u, 0x4699799cu,
                                     0x2b6bec59u, 0x2845b239u, 0xf3d95620u, 0x66e12d94u};
};

// 256 bits, little-endian limbs; what it means (normal or Montgomery form, which modulus) is
// the caller's business, as with the raw limb arrays of the other kernels
struct alignas(16) U256 {
  uint32_t v[8];
};

NZ_HD U256 u_zero() {
  U256 r;
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = 0;
  return r;
}

template <class Par>
NZ_HD U256 modulus() {
  U256 r;
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = Par::P[i];
  return r;
}
template <class Par>
NZ_HD U256 mont_one() {
  U256 r;
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = Par::ONE[i];
  return r;
}
template <class Par>
NZ_HD U256 mont_r2() {
  U256 r;
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = Par::R2[i];
  return r;
}

NZ_HD bool u_is_zero(const U256& a) {
  uint32_t x = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) x |= a.v[i];
  return x == 0;
}

NZ_HD bool u_eq(const U256& a, const U256& b) {
  uint32_t x = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) x |= a.v[i] ^ b.v[i];
  return x == 0;
}

// a + b as 256 bits, the carry out of limb 7 returned
NZ_HD uint32_t u_add(U256& r, const U256& a, const U256& b) {
  uint32_t c = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = addc(a.v[i], b.v[i], c);
  return c;
}

// a - b as 256 bits, the borrow out of limb 7 returned (1 iff a < b)
NZ_HD uint32_t u_sub(U256& r, const U256& a, const U256& b) {
  uint32_t w = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = subb(a.v[i], b.v[i], w);
  return w;
}

NZ_HD bool u_lt(const U256& a, const U256& b) {
  U256 t;
  return u_sub(t, a, b) != 0;
}

// c ? a : b, limb by limb (a ternary over the structs can become a choice between two
// addresses, which keeps both in scratch memory)
NZ_HD U256 u_select(bool c, const U256& a, const U256& b) {
  U256 r;
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = c ? a.v[i] : b.v[i];
  return r;
}

// (top : a) < 2m  ->  [0, m): subtract m when the ninth word is set or the low words reach m
template <class Par>
NZ_HD U256 cond_sub(const U256& a, uint32_t top) {
  U256 t;
  const uint32_t borrow = u_sub(t, a, modulus<Par>());
  return u_select((top | (borrow ^ 1u)) != 0, t, a);
}

// any 256-bit value -> [0, m): both moduli exceed 2^255, so one subtraction is enough
template <class Par>
NZ_HD U256 reduce(const U256& a) {
  return cond_sub<Par>(a, 0);
}

template <class Par>
NZ_HD U256 add(const U256& a, const U256& b) {
  U256 s;
  const uint32_t c = u_add(s, a, b);
  return cond_sub<Par>(s, c);
}

template <class Par>
NZ_HD U256 sub(const U256& a, const U256& b) {
  U256 d, t;
  const uint32_t borrow = u_sub(d, a, b);
  u_add(t, d, modulus<Par>());
  return u_select(borrow != 0, t, d);
}

template <class Par>
NZ_HD U256 neg(const U256& a) {
  return sub<Par>(u_zero(), a);
}

// Montgomery product a b 2^-256 mod m for a, b < m. Before the final subtraction the value is
// below 2m, which does not fit 256 bits: the column accumulator's last carry is the ninth word.
template <class Par>
NZ_HD U256 mul(const U256& a, const U256& b) {
  uint32_t q[8];
  U256 r;
  uint64_t acc = 0;
  uint32_t hi = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
#pragma unroll
    for (int j = 0; j < i; j++) {
      mac(acc, hi, a.v[j], b.v[i - j]);
      mac_c(acc, hi, q[j], Par::P[i - j]);
    }
    mac(acc, hi, a.v[i], b.v[0]);
    q[i] = (uint32_t)acc * Par::INV;
    mac_c(acc, hi, q[i], Par::P[0]);
    acc = (acc >> 32) | ((uint64_t)hi << 32);
    hi = 0;
  }
#pragma unroll
  for (int i = 8; i < 15; i++) {
#pragma unroll
    for (int j = i - 7; j < 8; j++) {
      mac(acc, hi, a.v[j], b.v[i - j]);
      mac_c(acc, hi, q[j], Par::P[i - j]);
    }
    r.v[i - 8] = (uint32_t)acc;
    acc = (acc >> 32) | ((uint64_t)hi << 32);
    hi = 0;
  }
  r.v[7] = (uint32_t)acc;
  return cond_sub<Par>(r, (uint32_t)(acc >> 32));
}

template <class Par>
NZ_HD U256 sqr(const U256& a) {
  return mul<Par>(a, a);
}

template <class Par>
NZ_HD U256 to_mont(const U256& a) {
  return mul<Par>(a, mont_r2<Par>());
}

template <class Par>
NZ_HD U256 from_mont(const U256& a) {
  U256 one = u_zero();
  one.v[0] = 1;
  return mul<Par>(a, one);
}

// a^(m - 2) (Fermat), Montgomery in and out; 0 -> 0. The exponent is shifted out of a register
// copy bit by bit, so no register array is indexed by a loop variable (that would be scratch).
template <class Par>
NZ_HD U256 inv(const U256& a) {
  U256 e = modulus<Par>();
  e.v[0] -= 2;  // both moduli are odd and end in a word above 1
  U256 r = mont_one<Par>();
#pragma unroll 1
  for (int i = 0; i < 256; i++) {
    r = sqr<Par>(r);
    if (e.v[7] >> 31) r = mul<Par>(r, a);
#pragma unroll
    for (int k = 7; k > 0; k--) e.v[k] = (e.v[k] << 1) | (e.v[k - 1] >> 31);
    e.v[0] <<= 1;
  }
  return r;
}

// 32 big-endian bytes (JWK coordinate, r, s, SHA-256 digest) <-> limbs. On the device the
// pointer is 4-byte aligned (checked by the caller).
NZ_HD U256 load_be(const uint8_t* p) {
  U256 r;
#if defined(__HIP_DEVICE_COMPILE__)
  const uint32_t* w = reinterpret_cast<const uint32_t*>(p);
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = __builtin_bswap32(w[7 - i]);
#else
  for (int i = 0; i < 8; i++) {
    const uint8_t* q = p + 4 * (7 - i);
    r.v[i] = ((uint32_t)q[0] << 24) | ((uint32_t)q[1] << 16) | ((uint32_t)q[2] << 8) | (uint32_t)q[3];
  }
#endif
  return r;
}

NZ_HD void store_be(uint8_t* p, const U256& a) {
  for (int i = 0; i < 8; i++) {
    uint8_t* q = p + 4 * (7 - i);
    q[0] = (uint8_t)(a.v[i] >> 24);
    q[1] = (uint8_t)(a.v[i] >> 16);
    q[2] = (uint8_t)(a.v[i] >> 8);
    q[3] = (uint8_t)a.v[i];
  }
}

// ---- the curve -------------------------------------------------------------------------------

typedef PParams Fp;
typedef NParams Fn;

NZ_HD U256 curve_b() {  // normal form
  const uint32_t c[8] = {0x27d2604bu, 0x3bce3c3eu, 0xcc53b0f6u, 0x651d06b0u,
                         0x769886bcu, 0xb3ebbd55u, 0xaa3a93e7u, 0x5ac635d8u};
  U256 r;
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = c[i];
  return r;
}

// affine point, coordinates in Montgomery form; never the point at infinity
struct Affine {
  U256 x, y;
};

NZ_HD Affine generator() {
  const uint32_t gx[8] = {0xd898c296u, 0xf4a13945u, 0x2deb33a0u, 0x77037d81u,
                          0x63a440f2u, 0xf8bce6e5u, 0xe12c4247u, 0x6b17d1f2u};
  const uint32_t gy[8] = {0x37bf51f5u, 0xcbb64068u, 0x6b315eceu, 0x2bce3357u,
                          0x7c0f9e16u, 0x8ee7eb4au, 0xfe1a7f9bu, 0x4fe342e2u};
  Affine g;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    g.x.v[i] = gx[i];
    g.y.v[i] = gy[i];
  }
  g.x = to_mont<Fp>(g.x);
  g.y = to_mont<Fp>(g.y);
  return g;
}

// y^2 = x^3 - 3x + b for normal-form x, y < p
NZ_HD bool on_curve(const U256& x, const U256& y) {
  const U256 xm = to_mont<Fp>(x), ym = to_mont<Fp>(y);
  U256 rhs = mul<Fp>(sqr<Fp>(xm), xm);
  const U256 x3 = add<Fp>(add<Fp>(xm, xm), xm);
  rhs = add<Fp>(sub<Fp>(rhs, x3), to_mont<Fp>(curve_b()));
  return u_eq(sqr<Fp>(ym), rhs);
}

// Jacobian point (X / Z^2, Y / Z^3), Montgomery coordinates; Z = 0 is the point at infinity
struct Jac {
  U256 x, y, z;
};

NZ_HD Jac jac_infinity() {
  Jac r;
  r.x = mont_one<Fp>();
  r.y = mont_one<Fp>();
  r.z = u_zero();
  return r;
}

NZ_HD bool jac_is_infinity(const Jac& a) { return u_is_zero(a.z); }

// 2 a for a = -3 (dbl-2001-b: 3 (X - Z^2)(X + Z^2) is the tangent's numerator). Infinity stays
// infinity (Z3 = 2 Y Z = 0); the curve has no point of order 2, so Y = 0 does not occur.
NZ_HD Jac jac_double(const Jac& a) {
  const U256 delta = sqr<Fp>(a.z), gamma = sqr<Fp>(a.y), beta = mul<Fp>(a.x, gamma);
  const U256 t = mul<Fp>(sub<Fp>(a.x, delta), add<Fp>(a.x, delta));
  const U256 alpha = add<Fp>(add<Fp>(t, t), t);
  U256 b4 = add<Fp>(beta, beta);
  b4 = add<Fp>(b4, b4);
  Jac r;
  r.x = sub<Fp>(sqr<Fp>(alpha), add<Fp>(b4, b4));
  const U256 yz = add<Fp>(a.y, a.z);
  r.z = sub<Fp>(sub<Fp>(sqr<Fp>(yz), gamma), delta);
  U256 g8 = sqr<Fp>(gamma);
  g8 = add<Fp>(g8, g8);
  g8 = add<Fp>(g8, g8);
  g8 = add<Fp>(g8, g8);
  r.y = sub<Fp>(mul<Fp>(alpha, sub<Fp>(b4, r.x)), g8);
  return r;
}

// a += b for an affine b: right when a is infinity, when a = b (the tangent) and when a = -b.
// In place and with one result object: separate result objects per return path stayed in
// scratch memory after inlining.
NZ_HD void jac_add_affine(Jac& a, const Affine& b) {
  if (jac_is_infinity(a)) {
    a.x = b.x;
    a.y = b.y;
    a.z = mont_one<Fp>();
    return;
  }
  const U256 z2 = sqr<Fp>(a.z);
  const U256 u2 = mul<Fp>(b.x, z2), s2 = mul<Fp>(b.y, mul<Fp>(z2, a.z));
  const U256 h = sub<Fp>(u2, a.x), rr = sub<Fp>(s2, a.y);
  if (u_is_zero(h)) {
    if (u_is_zero(rr)) {
      a = jac_double(a);
    } else {
      a.z = u_zero();  // a = -b: infinity is Z = 0, whatever X and Y hold
    }
    return;
  }
  const U256 h2 = sqr<Fp>(h), h3 = mul<Fp>(h2, h), v = mul<Fp>(a.x, h2);
  const U256 x3 = sub<Fp>(sub<Fp>(sqr<Fp>(rr), h3), add<Fp>(v, v));
  a.y = sub<Fp>(mul<Fp>(rr, sub<Fp>(v, x3)), mul<Fp>(a.y, h3));
  a.x = x3;
  a.z = mul<Fp>(a.z, h);
}

// a finite Jacobian point -> affine, given 1 / Z
NZ_HD Affine jac_to_affine(const Jac& a, const U256& zinv) {
  const U256 zi2 = sqr<Fp>(zinv);
  Affine r;
  r.x = mul<Fp>(a.x, zi2);
  r.y = mul<Fp>(a.y, mul<Fp>(zi2, zinv));
  return r;
}

// ---- fixed-base window tables --------------------------------------------------------------
// For a base B and window width w: entry [j 2^w + d] = d 2^(w j) B, affine, for
// 0 <= j < ceil(256 / w) and 1 <= d < 2^w (slot d = 0 is not used). B has prime order n and
// d 2^(w j) is not a multiple of n, so no entry is the point at infinity. u B is then the sum of
// one entry per non-zero window of u: ceil(256 / w) mixed additions, no doublings.

NZ_HD int table_windows(int w) { return (256 + w - 1) / w; }

// One window's row of the table: the lane (or host loop turn) for window j doubles B w j times,
// then adds the window's base 2^w - 2 times, keeping X, Y in the row and Z, and the running
// product of the Zs, in `zs` and `prods` (2^w values each), and turns the row affine with ONE
// inversion (Montgomery's trick).
NZ_HD void table_build_row(const Affine& base, int w, int j, Affine* row, U256* zs, U256* prods) {
  Jac p;
  p.x = base.x;
  p.y = base.y;
  p.z = mont_one<Fp>();
#pragma unroll 1
  for (int i = 0; i < w * j; i++) p = jac_double(p);
  const Affine pj = jac_to_affine(p, inv<Fp>(p.z));
  const int n = 1 << w;
  Jac acc = jac_infinity();
  U256 run = mont_one<Fp>();
#pragma unroll 1
  for (int d = 1; d < n; d++) {
    jac_add_affine(acc, pj);  // d = 2 is the doubling case
    row[d].x = acc.x;
    row[d].y = acc.y;
    zs[d] = acc.z;
    prods[d] = run;  // the product of zs[1 .. d - 1]
    run = mul<Fp>(run, acc.z);
  }
  U256 ri = inv<Fp>(run);
#pragma unroll 1
  for (int d = n - 1; d >= 1; d--) {
    const U256 zinv = mul<Fp>(ri, prods[d]);
    ri = mul<Fp>(ri, zs[d]);
    Jac t;
    t.x = row[d].x;
    t.y = row[d].y;
    t.z = zs[d];
    row[d] = jac_to_affine(t, zinv);
  }
}

// acc += u B from B's table; u in normal form (any 256-bit value: the digits are u's bits)
NZ_HD Jac table_mul_add(Jac acc, const Affine* table, int w, U256 u) {
  const int windows = table_windows(w);
  const uint32_t mask = (1u << w) - 1u;
#pragma unroll 1
  for (int j = 0; j < windows; j++) {
    const uint32_t d = u.v[0] & mask;
    if (d) jac_add_affine(acc, table[((size_t)j << w) + d]);
    // the next window moves down: the limbs are shifted, never indexed by j
#pragma unroll
    for (int k = 0; k < 7; k++) u.v[k] = (u.v[k] >> w) | (u.v[k + 1] << (32 - w));
    u.v[7] >>= w;
  }
  return acc;
}

// u1 G + u2 Q
NZ_HD Jac mul2(const Affine* tg, const Affine* tq, int w, const U256& u1, const U256& u2) {
  return table_mul_add(table_mul_add(jac_infinity(), tg, w, u1), tq, w, u2);
}

// ---- ECDSA verification of one signature -----------------------------------------------------
// status values as include/nzcb.h NZCB_SIG_*
NZ_HD int verify_one(const Affine* tg, const Affine* tq, int w, const uint8_t* hash, const uint8_t* sig) {
  const U256 r = load_be(sig), s = load_be(sig + 32);
  const U256 n = modulus<Fn>();
  // 1 <= r, s <= n - 1, and an out-of-range value is not reduced into range
  if (u_is_zero(r) || u_is_zero(s) || !u_lt(r, n) || !u_lt(s, n)) return 2;
  const U256 z = reduce<Fn>(load_be(hash));
  // Montgomery form of 1 / s; a normal-form factor times it is the product in normal form
  const U256 sinv = inv<Fn>(to_mont<Fn>(s));
  const U256 u1 = mul<Fn>(z, sinv), u2 = mul<Fn>(r, sinv);
  const Jac R = mul2(tg, tq, w, u1, u2);
  if (jac_is_infinity(R)) return 1;
  // R.x mod n = r, tested as X = r Z^2 without leaving Jacobian coordinates. r < n < p. The
  // affine x is below p < 2 n, so it may also be r + n, when that is below p.
  const U256 z2 = sqr<Fp>(R.z);
  if (u_eq(R.x, mul<Fp>(to_mont<Fp>(r), z2))) return 0;
  U256 rn;
  const uint32_t carry = u_add(rn, r, n);
  if (!carry && u_lt(rn, modulus<Fp>()) && u_eq(R.x, mul<Fp>(to_mont<Fp>(rn), z2))) return 0;
  return 1;
}

}  // namespace p256
}  // namespace nzcb
