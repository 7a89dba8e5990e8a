// The key material check (include/nzcb.h nzcb_ptau_check, nzcb_zkey_check): what its kernels
// and its host path share, and the readers of the two files' sections.
//
// NZ_HD functions compile for the device and for the host from this one text, so the host
// path (NZCB_KEY_HOST) judges a point, derives a weight and compares a value exactly as the
// kernels of key_check.hip do. The header needs no HIP runtime: a host-only program may
// include it (tests/native/key_check_host.cpp).
#pragma once
#include <cstdint>
#include <cstring>

#include "capi_guard.h"
#include "field.h"
#include "keccak.h"

namespace nzcb {

// ---------------------------------------------------------------- one SRS point
// w: x || y as 16 LE words, Montgomery form as stored (ptau section 2, zkey section 14).
// NZCB_KEY_OK, NZCB_KEY_ERR_RANGE (a stored coordinate >= q) or NZCB_KEY_ERR_CURVE ((0, 0) or
// y^2 != x^3 + 3; Montgomery products of the stored values, which are then below q).
NZ_HD int srs_point_status(const uint32_t* w) {
  Fq x, y;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    x.v[i] = w[i];
    y.v[i] = w[8 + i];
  }
  // x >= q iff x - q does not borrow
  uint32_t bx = 0, by = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    (void)subb(x.v[i], FqParams::P[i], bx);
    (void)subb(y.v[i], FqParams::P[i], by);
  }
  if (!bx || !by) return NZCB_KEY_ERR_RANGE;
  if (x.is_zero() && y.is_zero()) return NZCB_KEY_ERR_CURVE;
  const Fq one = Fq::one();
  const Fq three = one + one + one;
  return sqr(y) == sqr(x) * x + three ? NZCB_KEY_OK : NZCB_KEY_ERR_CURVE;
}

// The key of a defective point for a minimum over points: the lowest index wins and carries
// its status along.
NZ_HD uint64_t srs_bad_key(uint64_t index, int status) { return (index << 3) | (uint64_t)status; }
constexpr uint64_t kNoBadKey = ~uint64_t(0);

// ---------------------------------------------------------------- weights
// rho_i = the low 128 bits of keccak256(seed || LE32(i)) read as a big-endian integer, zero
// becomes 1 (verify_batch.hip batch_weight's rule). seed: the 32 bytes as 4 LE words. out: 8 LE
// words, normal form, the upper half zero (the generic MSM's scalar layout). One permutation:
// the 36 bytes and the padding fit the first block.
NZ_HD uint64_t bswap64(uint64_t x) {
  x = ((x & 0x00ff00ff00ff00ffULL) << 8) | ((x >> 8) & 0x00ff00ff00ff00ffULL);
  x = ((x & 0x0000ffff0000ffffULL) << 16) | ((x >> 16) & 0x0000ffff0000ffffULL);
  return (x << 32) | (x >> 32);
}
NZ_HD void srs_weight(const uint64_t seed[4], uint32_t i, uint32_t out[8]) {
  uint64_t s[25];
#pragma unroll
  for (int k = 0; k < 25; k++) s[k] = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) s[k] = seed[k];
  s[4] = (uint64_t)i | (uint64_t(0x01) << 32);  // LE32(i), then the pad byte at offset 36
  s[16] = uint64_t(0x80) << 56;                 // the last byte of the 136-byte block
  keccak_f1600(s);
  uint64_t lo = bswap64(s[3]), hi = bswap64(s[2]);  // digest bytes 24..31 and 16..23
  if (!(lo | hi)) lo = 1;
  out[0] = (uint32_t)lo;
  out[1] = (uint32_t)(lo >> 32);
  out[2] = (uint32_t)hi;
  out[3] = (uint32_t)(hi >> 32);
  out[4] = out[5] = out[6] = out[7] = 0;
}

// ---------------------------------------------------------------- Fr values of a zkey part
// a stored value that is not below r
NZ_HD bool fr_noncanonical(const uint32_t* w) {
  uint32_t b = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) (void)subb(w[i], FrParams::P[i], b);
  return !b;
}
NZ_HD bool words8_differ(const uint32_t* a, const uint32_t* b) {
  uint32_t x = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) x |= a[i] ^ b[i];
  return x != 0;
}

// ---------------------------------------------------------------- iden3 binfile sections (host)
// magic, u32 version, u32 count, (u32 type, u64 size, data)*: the first section of type `id`
// (the readers here want one of each), or {NULL, 0}. Throws NZCB_ERR_FORMAT for a file that
// ends inside a section table entry or a section.
struct KeySection {
  const uint8_t* p = nullptr;
  uint64_t len = 0;
};
inline KeySection key_find_section(const uint8_t* d, size_t len, const char magic[4], uint32_t id) {
  if (!d || len < 12 || std::memcmp(d, magic, 4) != 0)
    throw Error(NZCB_ERR_FORMAT, std::string(magic, 4) + ": invalid file format");
  uint32_t nsec;
  std::memcpy(&nsec, d + 8, 4);
  size_t off = 12;
  KeySection found;
  for (uint32_t i = 0; i < nsec; i++) {
    if (len - off < 12) throw Error(NZCB_ERR_FORMAT, std::string(magic, 4) + ": truncated section table");
    uint32_t type;
    uint64_t size;
    std::memcpy(&type, d + off, 4);
    std::memcpy(&size, d + off + 4, 8);
    off += 12;
    if (size > len - off) throw Error(NZCB_ERR_FORMAT, std::string(magic, 4) + ": truncated section");
    if (type == id && !found.p) found = KeySection{d + off, size};
    off += size;
  }
  return found;
}

// What nzcb_ptau_check reads of a powers-of-tau file.
struct PtauView {
  uint32_t power = 0;
  const uint8_t* g1 = nullptr;  // `count` points
  uint64_t count = 0;
  const uint8_t* g2_0 = nullptr;  // tauG2[0], 128 B
  const uint8_t* g2_1 = nullptr;  // tauG2[1] = [tau]G2
};
// count = 0: every point the header promises
inline PtauView ptau_open(const uint8_t* d, size_t len, uint64_t count) {
  const KeySection h = key_find_section(d, len, "ptau", 1), s2 = key_find_section(d, len, "ptau", 2),
                   s3 = key_find_section(d, len, "ptau", 3);
  if (!h.p || !s2.p || !s3.p) throw Error(NZCB_ERR_FORMAT, "ptau: missing header, tauG1 or tauG2");
  uint32_t n8 = 0;
  if (h.len < 40) throw Error(NZCB_ERR_FORMAT, "ptau: header too short");
  std::memcpy(&n8, h.p, 4);
  if (n8 != 32 || std::memcmp(h.p + 4, FqParams::P, 32) != 0)
    throw Error(NZCB_ERR_FORMAT, "ptau: not a bn128 powers of tau file");
  PtauView v;
  std::memcpy(&v.power, h.p + 36, 4);
  if (v.power > 28) throw Error(NZCB_ERR_FORMAT, "ptau: power above 28");
  const uint64_t promised = (uint64_t(2) << v.power) - 1, held = s2.len / 64;
  if (count == 0) {
    if (held < promised) throw Error(NZCB_ERR_FORMAT, "ptau: tauG1 section shorter than the header's power");
    count = promised;
  } else if (count > held) {
    throw Error(NZCB_ERR_ARG, "ptau: count is larger than the tauG1 section");
  }
  if (s3.len < 256) throw Error(NZCB_ERR_FORMAT, "ptau: tauG2 section too small");
  v.g1 = s2.p;
  v.count = count;
  v.g2_0 = s3.p;
  v.g2_1 = s3.p + 128;
  return v;
}

}  // namespace nzcb
