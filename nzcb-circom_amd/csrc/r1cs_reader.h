// iden3 binary files and the r1cs reader (host): the sections, the r1cs header and the
// linear combinations of the constraint section. Two users parse through it: the PLONK
// setup (csrc/synth.hip circuit_from_r1cs, snarkjs `plonk setup`) and the witness check
// (csrc/r1cs_check.hip, snarkjs `wtns check`), so a file is malformed for both in the same
// words. The Groth16 setup (csrc/groth16.h) reads its constraints through it too. The header
// needs no HIP runtime.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

#include "capi_guard.h"
#include "field.h"

namespace nzcb {

struct BinSections {  // iden3 binfile: magic, u32 version, u32 count, (u32 type, u64 size, data)*
  std::vector<std::pair<const uint8_t*, uint64_t>> sec[16];  // other section types are ignored
};
inline BinSections read_binfile(const uint8_t* d, size_t len, const char* magic, const char* what) {
  BinSections b;
  char msg[96];
  if (!d || len < 12 || std::memcmp(d, magic, 4) != 0) {
    std::snprintf(msg, sizeof msg, "%s: invalid file format", what);
    throw Error(NZCB_ERR_FORMAT, msg);
  }
  uint32_t version, nsec;
  std::memcpy(&version, d + 4, 4);
  std::memcpy(&nsec, d + 8, 4);
  size_t off = 12;
  for (uint32_t i = 0; i < nsec; i++) {
    if (off + 12 > len) throw Error(NZCB_ERR_FORMAT, "truncated section table");
    uint32_t type;
    uint64_t size;
    std::memcpy(&type, d + off, 4);
    std::memcpy(&size, d + off + 4, 8);
    off += 12;
    if (size > len - off) throw Error(NZCB_ERR_FORMAT, "truncated section");
    if (type < 16) b.sec[type].push_back({d + off, size});
    off += size;
  }
  return b;
}

struct ByteReader {
  const uint8_t* p;
  uint64_t left;
  uint32_t u32() {
    if (left < 4) throw Error(NZCB_ERR_FORMAT, "r1cs: truncated");
    uint32_t v;
    std::memcpy(&v, p, 4);
    p += 4;
    left -= 4;
    return v;
  }
  uint64_t u64() {
    const uint64_t lo = u32();
    return lo | ((uint64_t)u32() << 32);
  }
  Fr fr_normal() {  // 32 B LE normal form -> Montgomery (ffjavascript Fr.fromRprLE)
    if (left < 32) throw Error(NZCB_ERR_FORMAT, "r1cs: truncated");
    Fr v;
    std::memcpy(v.v, p, 32);
    p += 32;
    left -= 32;
    if (!(reduce_once(v) == v) || v == Fr::modulus()) throw Error(NZCB_ERR_FORMAT, "r1cs: coefficient not reduced");
    return to_mont(v);
  }
};

// The header section (1) and a reader placed at the start of the constraint section (2).
struct R1csFile {
  uint32_t n_wires = 0, n_out = 0, n_pub_in = 0, n_prv_in = 0, n_cons = 0;
  uint64_t n_labels = 0;
  ByteReader constraints{nullptr, 0};
};
// curve_msg: the NZCB_ERR_CURVE text when the prime is not BN254's r (each command has snarkjs's own)
inline R1csFile r1cs_open(const uint8_t* d, size_t len, const char* curve_msg) {
  BinSections b = read_binfile(d, len, "r1cs", "r1cs");
  if (b.sec[1].empty() || b.sec[2].empty()) throw Error(NZCB_ERR_FORMAT, "r1cs: missing header or constraints");
  ByteReader h{b.sec[1][0].first, b.sec[1][0].second};
  if (h.u32() != 32) throw Error(NZCB_ERR_FORMAT, "r1cs: field size is not 32 bytes");
  if (h.left < 32 || std::memcmp(h.p, FrParams::P, 32) != 0) throw Error(NZCB_ERR_CURVE, curve_msg);
  h.p += 32;
  h.left -= 32;
  R1csFile f;
  f.n_wires = h.u32();
  f.n_out = h.u32();
  f.n_pub_in = h.u32();
  f.n_prv_in = h.u32();
  f.n_labels = h.u64();
  f.n_cons = h.u32();
  f.constraints = ByteReader{b.sec[2][0].first, b.sec[2][0].second};
  return f;
}

// One linear combination: term(signal, coefficient in Montgomery form) per entry, in file order.
template <class F>
inline void r1cs_read_lc(ByteReader& cr, uint32_t n_wires, F&& term) {
  const uint32_t nt = cr.u32();
  for (uint32_t i = 0; i < nt; i++) {
    const uint32_t s = cr.u32();
    const Fr coef = cr.fr_normal();
    if (s >= n_wires) throw Error(NZCB_ERR_FORMAT, "r1cs: signal out of range");
    term(s, coef);
  }
}

}  // namespace nzcb
