// The PLONK verifier's steps, shared by the single-proof verifier (verify.cpp) and the
// batch verifier (verify_batch.hip):
//   (a) plonk_parse : canonical Fq / Fr, points on the curve, nPublic
//   (b) plonk_terms : Fiat-Shamir challenges and the (point, scalar) terms of the two
//                     pairing inputs, L = Wxi + u Wxiw and R = xi Wxi + u xi w Wxiw + F - E
//   (c) pairing_check(-L, X_2; R, [1]_2)
// and the G1 linear-combination functions (NZ_HD: the host path of the batch verifier and
// its kernels compile the same code, so both give the same bytes).
#pragma once
#include <cstring>
#include <utility>
#include <vector>

#include "ec.h"

namespace nzcb {

struct F2 {  // Fq2 = Fq[u]/(u^2 + 1)
  Fq a, b;
};
struct P2 {  // G2 (twist), affine
  F2 x, y;
  bool inf = false;
};

// binary verification key (include/nzcb.h NZCB_VK_BYTES)
struct Vk {
  uint32_t nPublic = 0, power = 0;
  Fr k1, k2, w;
  G1Affine q[8];  // Qm, Ql, Qr, Qo, Qc, S1, S2, S3
  P2 x2;
};
Vk vk_read(const uint8_t* in, bool* ok);
P2 g2_generator();
// G2 on the host for the key check (csrc/key_check.hip): the sum of two points, and whether a
// finite point satisfies the twist's equation y^2 = x^3 + 3 / (9 + u)
P2 p2_sum(const P2& a, const P2& b);
bool p2_on_twist(const P2& p);

// prod e(P_i, Q_i) == 1
bool pairing_check(const std::vector<std::pair<G1Affine, P2>>& pairs);

G1Affine g1_neg(const G1Affine& p);
// x || y, 32-byte LE normal form each, zeros = infinity; *ok = false if a coordinate is >= p
G1Affine g1_from_le(const uint8_t* p, bool* ok);
void g1_to_le(const G1Affine& a, uint8_t* out);

struct ProofParsed {
  G1Affine pt[9];  // A, B, C, Z, T1, T2, T3, Wxi, Wxiw
  Fr ev[7];        // eval_a, eval_b, eval_c, eval_s1, eval_s2, eval_zw, eval_r
  std::vector<Fr> pubs;
};
// step (a); false = the proof is invalid whatever the pairing says
bool plonk_parse(const Vk& vk, const uint8_t* proof, const uint8_t* pub, int npub, ProofParsed* out);

constexpr int kVerifyLTerms = 2, kVerifyRTerms = 18;
struct VerifyTerms {
  G1Affine lp[kVerifyLTerms];  // (Wxi, 1), (Wxiw, u)
  Fr ls[kVerifyLTerms];
  G1Affine rp[kVerifyRTerms];  // the 17 terms of D, F, xi Wxi, u xi w Wxiw, then (G1 generator, -e)
  Fr rs[kVerifyRTerms];        // Montgomery form
};
// step (b)
void plonk_terms(const Vk& vk, const ProofParsed& p, bool transcript_public, VerifyTerms* out);

// ---------------------------------------------------------------- G1 linear combinations
// c ? a : b, limb by limb (v_cndmask on the device: no branch on a scalar's bits)
NZ_HD Fq fq_select(bool c, const Fq& a, const Fq& b) {
  Fq r;
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = c ? a.v[i] : b.v[i];
  return r;
}

// k * P, MSB-first double-and-add. pt: x || y as 16 LE words, normal form (zeros = infinity);
// sc: 8 LE words, normal form. The scalar is read one word per 32 steps and the sum is formed
// every step and kept or dropped by a select, so there is no table indexed at run time and a
// wavefront does not serialise on the bits of its 64 scalars.
NZ_HD G1xyzz g1_term_mul(const uint32_t* pt, const uint32_t* sc) {
  Fq x, y;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    x.v[i] = pt[i];
    y.v[i] = pt[8 + i];
  }
  G1xyzz acc = G1xyzz::inf();
  if (x.is_zero() && y.is_zero()) return acc;
  x = to_mont(x);
  y = to_mont(y);
  for (int l = 7; l >= 0; l--) {
    const uint32_t w = sc[l];
    for (int b = 31; b >= 0; b--) {
      acc = xyzz_dbl(acc);
      const G1xyzz s = xyzz_add_affine(acc, x, y);
      const bool bit = (w >> b) & 1u;
      acc.X = fq_select(bit, s.X, acc.X);
      acc.Y = fq_select(bit, s.Y, acc.Y);
      acc.ZZ = fq_select(bit, s.ZZ, acc.ZZ);
      acc.ZZZ = fq_select(bit, s.ZZZ, acc.ZZZ);
    }
  }
  return acc;
}

// sum of terms[lo, hi) as an affine point: 16 LE words, normal form, zeros = infinity
NZ_HD void g1_group_sum(const G1xyzz* terms, uint32_t lo, uint32_t hi, uint32_t* out) {
  G1xyzz acc = G1xyzz::inf();
  for (uint32_t j = lo; j < hi; j++) acc = xyzz_add(acc, terms[j]);
  if (acc.is_inf()) {
#pragma unroll
    for (int i = 0; i < 16; i++) out[i] = 0;
    return;
  }
  const Fq x = from_mont(acc.X * inverse(acc.ZZ));
  const Fq y = from_mont(acc.Y * inverse(acc.ZZZ));
#pragma unroll
  for (int i = 0; i < 8; i++) {
    out[i] = x.v[i];
    out[8 + i] = y.v[i];
  }
}

}  // namespace nzcb
