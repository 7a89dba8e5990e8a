// NZ COVID Pass URI -> COSE_Sign1 -> record, Sig_structure digest and circuit input signals
// (include/nzcb.h nzcb_nzcp_decode), as NZ_HD functions, so that the kernel (csrc/nzcp_decode.hip),
// the host path and the stand-alone bounds test (tests/native/nzcp_decode_host.cpp) run one source.
//
// The parallel steps take (lane, lanes): the kernel calls them with the lane of a 64-lane
// workgroup, the host with (0, 1). The serial steps (the prefix, the CBOR walk, SHA-256) take no
// lane. The input is untrusted. The rules every function here keeps:
//   * `uri` is read in [0, len) only, `cose` in [0, n) only, and an item of a byte string that is
//     parsed on its own (protected header, claims) within that string only: every read goes
//     through read_head / skip_item, which take the region's end and check against it first;
//   * a length taken from the input is a uint64_t and is compared against the bytes left of the
//     region BEFORE it is added to an offset or counted: offsets stay uint32_t below the region's
//     end, which is at most kMaxCose;
//   * skipping does not recurse: a counter of items still to read, and every iteration consumes
//     at least one byte, so the walk ends after at most n heads whatever the nesting.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/nzcb.h"

#ifndef NZ_HD
#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define NZ_HD __host__ __device__ __forceinline__
#else
#define NZ_HD inline
#endif
#endif

namespace nzcb {
namespace nzdec {

constexpr uint32_t kMaxUri = NZCB_PASS_MAX_URI;
// the shortest prefix is "NZCP:/1/": at most 2040 digits, floor(5 * 2040 / 8) = 1275 bytes
constexpr uint32_t kMaxCose = 1280;
// 12 bytes of context, two heads of at most 3 bytes, the empty external_aad, and the two strings,
// which lie in the COSE bytes without overlapping: at most 12 + 3 + 1 + 3 + 1275 = 1294
constexpr uint32_t kMaxTbs = 1296;
constexpr uint32_t kNone = 0xffffffffu;
constexpr uint32_t kDataBytes = 20;
constexpr uint32_t kDataBits = 8 * kDataBytes;

// ------------------------------------------------------------------ prefix and base32
// "NZCP:/" digits{1,9} "/" and at least one more byte; *start = the index of that byte
NZ_HD bool parse_prefix(const uint8_t* uri, uint32_t len, uint32_t* version, uint32_t* start) {
  const uint8_t lead[6] = {'N', 'Z', 'C', 'P', ':', '/'};
  if (len < 6) return false;
  for (uint32_t i = 0; i < 6; i++)
    if (uri[i] != lead[i]) return false;
  uint32_t i = 6, v = 0, digits = 0;
  while (i < len && uri[i] >= '0' && uri[i] <= '9') {
    if (++digits > 9) return false;
    v = v * 10 + (uri[i] - '0');  // at most 999,999,999
    i++;
  }
  if (digits < 1 || i >= len || uri[i] != '/') return false;
  i++;
  if (i >= len) return false;
  *version = v;
  *start = i;
  return true;
}

// the value of a base32 digit (RFC 4648 alphabet, upper case), 0xff for any other byte
NZ_HD uint32_t b32_value(uint8_t c) {
  if (c >= 'A' && c <= 'Z') return (uint32_t)(c - 'A');
  if (c >= '2' && c <= '7') return (uint32_t)(c - '2') + 26u;
  return 0xffu;
}

// the lowest index i in [start, len), i = start + lane (mod lanes), whose byte is no base32
// digit, or kNone; the minimum over the lanes is the BASE32 detail
NZ_HD uint32_t b32_first_bad(const uint8_t* uri, uint32_t start, uint32_t len, uint32_t lane, uint32_t lanes) {
  for (uint32_t i = start + lane; i < len; i += lanes)
    if (b32_value(uri[i]) == 0xffu) return i;
  return kNone;
}

NZ_HD uint32_t b32_bytes(uint32_t digits) { return (uint32_t)(((uint64_t)digits * 5u) / 8u); }

// cose[j] for j = lane (mod lanes) below b32_bytes(len - start): bits [8j, 8j + 8) of the digits'
// 5-bit values, which lie in at most three digits. The leftover bits of the last digits are
// dropped. All digits must be valid (b32_first_bad found none).
NZ_HD void b32_decode(const uint8_t* uri, uint32_t start, uint32_t len, uint8_t* cose, uint32_t lane, uint32_t lanes) {
  const uint32_t digits = len - start;
  const uint32_t n = b32_bytes(digits);
  for (uint32_t j = lane; j < n; j += lanes) {
    const uint32_t bit = 8u * j, c0 = bit / 5u, sh = bit % 5u;
    uint32_t acc = 0;
    for (uint32_t k = 0; k < 3; k++) {
      const uint32_t c = c0 + k;
      acc = (acc << 5) | (c < digits ? (b32_value(uri[start + c]) & 31u) : 0u);
    }
    cose[j] = (uint8_t)(acc >> (7u - sh));
  }
}

// ------------------------------------------------------------------ CBOR
struct Head {
  uint32_t major, info;
  uint64_t arg;
  uint32_t next;  // the first byte after the head: a string's body, an array's first item
};

// The head at `off` of the region that ends at `end` (off <= end <= the buffer's length). 0, or
// the failing status: the head's own bytes, a string's body or an array's / map's item count
// beyond the region is TRUNCATED, additional info 28..31 is CBOR.
NZ_HD int read_head(const uint8_t* buf, uint32_t off, uint32_t end, Head* h) {
  if (off >= end) return NZCB_PASS_ERR_TRUNCATED;
  const uint8_t ib = buf[off];
  h->major = ib >> 5;
  h->info = ib & 31u;
  h->arg = h->info;
  uint32_t next = off + 1;
  if (h->info >= 28) return NZCB_PASS_ERR_CBOR;
  if (h->info >= 24) {
    const uint32_t nb = 1u << (h->info - 24);
    if (nb > end - next) return NZCB_PASS_ERR_TRUNCATED;
    uint64_t a = 0;
    for (uint32_t k = 0; k < nb; k++) a = (a << 8) | buf[next + k];
    h->arg = a;
    next += nb;
  }
  h->next = next;
  if (h->major >= 2 && h->major <= 5 && h->arg > (uint64_t)(end - next)) return NZCB_PASS_ERR_TRUNCATED;
  return 0;
}

// One whole item starting at `off`: *next = the offset after it. On failure *detail = the offset
// of the failing head.
NZ_HD int skip_item(const uint8_t* buf, uint32_t off, uint32_t end, uint32_t* next, uint32_t* detail) {
  uint64_t todo = 1;  // items still to read; bounded by (1 + 2 * end) * end, far below 2^64
  while (todo) {
    Head h;
    const int st = read_head(buf, off, end, &h);
    if (st) {
      *detail = off;
      return st;
    }
    todo--;
    off = h.next;
    switch (h.major) {
      case 2:
      case 3: off += (uint32_t)h.arg; break;  // arg <= end - next, checked by read_head
      case 4: todo += h.arg; break;
      case 5: todo += 2 * h.arg; break;
      case 6: todo += 1; break;
      default: break;  // integers and major 7: the head is the item
    }
  }
  *next = off;
  return 0;
}

NZ_HD int32_t saturate_int(const Head& h) {  // major 0: arg, major 1: -1 - arg
  if (h.major == 0) return h.arg > 0x7fffffffull ? (int32_t)0x7fffffff : (int32_t)h.arg;
  return h.arg > 0x7fffffffull ? (int32_t)(-0x7fffffff - 1) : (int32_t)(-1 - (int64_t)h.arg);
}

NZ_HD void copy_first(uint8_t* dst, uint32_t cap, const uint8_t* src, uint64_t len) {
  for (uint32_t i = 0; i < cap; i++) dst[i] = i < len ? src[i] : 0;
}

NZ_HD int fail(nzcb_nzcp_pass* r, int status, uint32_t detail) {
  r->status = status;
  r->detail = detail;
  return status;
}

// The map at the start of cose[off, end): the protected header (claims = false) or the CWT claims
// (claims = true) into *r. `not_map` is the status when the region does not begin with a map.
NZ_HD int parse_map(const uint8_t* cose, uint32_t off, uint32_t end, bool claims, int not_map, nzcb_nzcp_pass* r) {
  Head m;
  int st = read_head(cose, off, end, &m);
  if (st) return fail(r, st, off);
  if (m.major != 5) return fail(r, not_map, off);
  off = m.next;
  for (uint64_t e = 0; e < m.arg; e++) {
    Head k;
    st = read_head(cose, off, end, &k);
    if (st) return fail(r, st, off);
    uint64_t key = ~0ull;  // an integer key >= 0, or none of those this parser knows
    uint32_t detail = 0;
    if (k.major == 0) {
      key = k.arg;
      off = k.next;
    } else {
      st = skip_item(cose, off, end, &off, &detail);
      if (st) return fail(r, st, detail);
    }
    Head v;
    st = read_head(cose, off, end, &v);
    if (st) return fail(r, st, off);
    const uint8_t* body = cose + v.next;  // of a string: [next, next + arg) is inside the region
    if (!claims && key == 1) {
      r->present &= ~(uint32_t)NZCB_PASS_HAS_ALG;
      r->alg = 0;
      if (v.major <= 1) {
        r->alg = saturate_int(v);
        r->present |= NZCB_PASS_HAS_ALG;
      }
    } else if (!claims && key == 4) {
      r->present &= ~(uint32_t)NZCB_PASS_HAS_KID;
      r->kid_len = 0;
      copy_first(r->kid, sizeof(r->kid), body, 0);
      if (v.major == 2) {
        r->kid_len = (uint32_t)v.arg;
        copy_first(r->kid, sizeof(r->kid), body, v.arg);
        r->present |= NZCB_PASS_HAS_KID;
      }
    } else if (claims && key == 1) {
      r->present &= ~(uint32_t)NZCB_PASS_HAS_ISS;
      r->iss_len = 0;
      copy_first(r->iss, sizeof(r->iss), body, 0);
      if (v.major == 3) {
        r->iss_len = (uint32_t)v.arg;
        copy_first(r->iss, sizeof(r->iss), body, v.arg);
        r->present |= NZCB_PASS_HAS_ISS;
      }
    } else if (claims && (key == 4 || key == 5)) {
      const uint32_t bit = key == 4 ? NZCB_PASS_HAS_EXP : NZCB_PASS_HAS_NBF;
      uint64_t* dst = key == 4 ? &r->exp : &r->nbf;
      r->present &= ~bit;
      *dst = 0;
      if (v.major == 0) {
        *dst = v.arg;
        r->present |= bit;
      }
    } else if (claims && key == 7) {
      r->present &= ~(uint32_t)NZCB_PASS_HAS_CTI;
      r->cti_len = 0;
      copy_first(r->cti, sizeof(r->cti), body, 0);
      if (v.major == 2) {
        r->cti_len = (uint32_t)v.arg;
        copy_first(r->cti, sizeof(r->cti), body, v.arg);
        r->present |= NZCB_PASS_HAS_CTI;
      }
    }
    st = skip_item(cose, off, end, &off, &detail);  // the value, whatever it is
    if (st) return fail(r, st, detail);
  }
  return 0;
}

// Steps 5 to 7 over cose[0, n): COSE_Sign1, protected header, claims. *r must be zeroed but for
// version. Returns r->status.
NZ_HD int parse_cose(const uint8_t* cose, uint32_t n, nzcb_nzcp_pass* r) {
  Head h;
  uint32_t off = 0, detail = 0;
  int st = read_head(cose, off, n, &h);
  if (st) return fail(r, st, off);
  if (h.major != 6 || h.arg != 18) return fail(r, NZCB_PASS_ERR_NOT_COSE, off);
  off = h.next;
  st = read_head(cose, off, n, &h);
  if (st) return fail(r, st, off);
  if (h.major != 4 || h.arg != 4) return fail(r, NZCB_PASS_ERR_NOT_COSE, off);
  off = h.next;
  // item 0: the protected header, a byte string
  st = read_head(cose, off, n, &h);
  if (st) return fail(r, st, off);
  if (h.major != 2) return fail(r, NZCB_PASS_ERR_NOT_COSE, off);
  r->protected_off = h.next;
  r->protected_len = (uint32_t)h.arg;
  off = h.next + (uint32_t)h.arg;
  // item 1: the unprotected header, not looked at
  st = skip_item(cose, off, n, &off, &detail);
  if (st) return fail(r, st, detail);
  // item 2: the payload, a byte string
  st = read_head(cose, off, n, &h);
  if (st) return fail(r, st, off);
  if (h.major != 2) return fail(r, NZCB_PASS_ERR_NOT_COSE, off);
  r->payload_off = h.next;
  r->payload_len = (uint32_t)h.arg;
  off = h.next + (uint32_t)h.arg;
  // item 3: the signature
  st = read_head(cose, off, n, &h);
  if (st) return fail(r, st, off);
  if (h.major == 2) {
    r->present |= NZCB_PASS_HAS_SIG;
    r->sig_len = (uint32_t)h.arg;
    copy_first(r->sig, sizeof(r->sig), cose + h.next, h.arg == sizeof(r->sig) ? h.arg : 0);
    off = h.next + (uint32_t)h.arg;
  } else {
    st = skip_item(cose, off, n, &off, &detail);
    if (st) return fail(r, st, detail);
  }
  r->cose_len = off;
  if (parse_map(cose, r->protected_off, r->protected_off + r->protected_len, false, NZCB_PASS_ERR_HEADER, r))
    return r->status;
  return parse_map(cose, r->payload_off, r->payload_off + r->payload_len, true, NZCB_PASS_ERR_CLAIMS, r);
}

// every field but status, detail and version back to zero (a failed pass)
NZ_HD void clear_failed(nzcb_nzcp_pass* r) {
  const int32_t status = r->status;
  const uint32_t detail = r->detail, version = r->version;
  *r = nzcb_nzcp_pass{};
  r->status = status;
  r->detail = detail;
  r->version = version;
}

// ------------------------------------------------------------------ Sig_structure
NZ_HD uint32_t bstr_head_bytes(uint32_t len) { return len < 24 ? 1u : len < 256 ? 2u : 3u; }  // len < 65536

NZ_HD uint32_t put_bstr_head(uint8_t* p, uint32_t len) {
  if (len < 24) {
    p[0] = (uint8_t)(0x40u | len);
    return 1;
  }
  if (len < 256) {
    p[0] = 0x58;
    p[1] = (uint8_t)len;
    return 2;
  }
  p[0] = 0x59;
  p[1] = (uint8_t)(len >> 8);
  p[2] = (uint8_t)len;
  return 3;
}

NZ_HD uint32_t tbs_length(uint32_t protected_len, uint32_t payload_len) {
  return 12u + bstr_head_bytes(protected_len) + protected_len + 1u + bstr_head_bytes(payload_len) + payload_len;
}

// ["Signature1", protected, h'', payload] into tbs[0, tbs_length) (at most kMaxTbs): lane 0 writes
// the heads, all lanes copy the two strings out of the COSE bytes
NZ_HD void tbs_fill(const uint8_t* cose, const nzcb_nzcp_pass* r, uint8_t* tbs, uint32_t lane, uint32_t lanes) {
  const uint32_t plen = r->protected_len, qlen = r->payload_len;
  const uint32_t p_at = 12u + bstr_head_bytes(plen);
  const uint32_t q_at = p_at + plen + 1u + bstr_head_bytes(qlen);
  if (lane == 0) {
    const uint8_t ctx[12] = {0x84, 0x6a, 'S', 'i', 'g', 'n', 'a', 't', 'u', 'r', 'e', '1'};
    for (uint32_t i = 0; i < 12; i++) tbs[i] = ctx[i];
    put_bstr_head(tbs + 12, plen);
    tbs[p_at + plen] = 0x40;
    put_bstr_head(tbs + p_at + plen + 1, qlen);
  }
  for (uint32_t i = lane; i < plen; i += lanes) tbs[p_at + i] = cose[r->protected_off + i];
  for (uint32_t i = lane; i < qlen; i += lanes) tbs[q_at + i] = cose[r->payload_off + i];
}

// ------------------------------------------------------------------ SHA-256
struct Sha256K {
  static constexpr uint32_t K[64] = {
      0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5,
      0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174,
      0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da,
      0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967,
      0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
      0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070,
      0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3,
      0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
};

NZ_HD uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }

// SHA-256 of msg[0, len), len < 2^29; reads msg below len only (the padding is made up here).
// The 16-word schedule window and the rounds are unrolled so that w[] stays in registers.
NZ_HD void sha256(const uint8_t* msg, uint32_t len, uint8_t out[32]) {
  uint32_t h[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
  const uint32_t nblocks = (len + 9 + 63) / 64;
  const uint64_t bitlen = (uint64_t)len * 8;
  for (uint32_t blk = 0; blk < nblocks; blk++) {
    uint32_t w[16];
#pragma unroll
    for (int t = 0; t < 16; t++) {
      uint32_t word = 0;
#pragma unroll
      for (int b = 0; b < 4; b++) {
        const uint32_t idx = blk * 64 + 4 * t + b;
        uint32_t byte = idx < len ? msg[idx] : (idx == len ? 0x80u : 0u);
        if (blk == nblocks - 1 && t >= 14) byte = (uint32_t)(bitlen >> (8 * (7 - (4 * (t - 14) + b)))) & 0xffu;
        word = (word << 8) | byte;
      }
      w[t] = word;
    }
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
#pragma unroll
    for (int i = 0; i < 64; i++) {
      uint32_t wi;
      if (i < 16) {
        wi = w[i];
      } else {
        const uint32_t w15 = w[(i + 1) & 15], w2 = w[(i + 14) & 15];
        const uint32_t s0 = rotr(w15, 7) ^ rotr(w15, 18) ^ (w15 >> 3);
        const uint32_t s1 = rotr(w2, 17) ^ rotr(w2, 19) ^ (w2 >> 10);
        wi = w[i & 15] + s0 + w[(i + 9) & 15] + s1;
        w[i & 15] = wi;
      }
      const uint32_t S1 = rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25);
      const uint32_t ch = (e & f) ^ (~e & g);
      const uint32_t t1 = hh + S1 + ch + Sha256K::K[i] + wi;
      const uint32_t S0 = rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22);
      const uint32_t mj = (a & b) ^ (a & c) ^ (b & c);
      const uint32_t t2 = S0 + mj;
      hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
    }
    h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
  }
#pragma unroll
  for (int i = 0; i < 8; i++)
#pragma unroll
    for (int b = 0; b < 4; b++) out[4 * i + b] = (uint8_t)(h[i] >> (24 - 8 * b));
}

// ------------------------------------------------------------------ circuit input signals
NZ_HD uint32_t input_signals(uint32_t max_tbs_bytes) { return 8u * max_tbs_bytes + 1u + kDataBits; }

// signal k of the main's inputs (all fit 32 bits): toBeSigned bit k (MSB first per byte, zero past
// the length), toBeSignedLen, then the data bits: bit j of the reversed-bytes / reversed-bits
// arrangement, MSB first, is bit (j % 8) of data[19 - j / 8]
NZ_HD uint32_t input_signal(const uint8_t* tbs, uint32_t tbs_len, const uint8_t* data20, uint32_t max_tbs_bytes,
                            uint32_t k) {
  const uint32_t nbits = 8u * max_tbs_bytes;
  if (k < nbits) return (k >> 3) < tbs_len ? (uint32_t)(tbs[k >> 3] >> (7u - (k & 7u))) & 1u : 0u;
  if (k == nbits) return tbs_len;
  const uint32_t j = k - nbits - 1u;
  return data20 ? (uint32_t)(data20[kDataBytes - 1u - (j >> 3)] >> (j & 7u)) & 1u : 0u;
}

// One pass's block of input_signals() x 32 bytes, written as 16-byte halves h = lane (mod lanes):
// half 2k holds signal k's low word, half 2k + 1 is zero. fits = false writes zeros. `out` is
// 16-byte aligned on the device (consecutive lanes, consecutive 16-byte stores).
NZ_HD void inputs_fill(const uint8_t* tbs, uint32_t tbs_len, const uint8_t* data20, uint32_t max_tbs_bytes, bool fits,
                       uint8_t* out, uint32_t lane, uint32_t lanes) {
  const uint32_t halves = 2u * input_signals(max_tbs_bytes);
  for (uint32_t q = lane; q < halves; q += lanes) {
    const uint32_t v = (fits && !(q & 1u)) ? input_signal(tbs, tbs_len, data20, max_tbs_bytes, q >> 1) : 0u;
#if defined(__HIP_DEVICE_COMPILE__)
    reinterpret_cast<uint4*>(out)[q] = make_uint4(v, 0u, 0u, 0u);
#else
    uint8_t b[16] = {(uint8_t)v, (uint8_t)(v >> 8), (uint8_t)(v >> 16), (uint8_t)(v >> 24)};
    memcpy(out + (size_t)16 * q, b, 16);
#endif
  }
}

// ------------------------------------------------------------------ one pass, serially
// The whole decode of one URI with (lane, lanes) = (0, 1): the host path, and the statement of
// the order the kernel follows. cose: kMaxCose bytes, tbs: kMaxTbs bytes of the caller's.
// inputs_out (may be NULL) takes input_signals(max_tbs_bytes) x 32 bytes, tbs_out (may be NULL)
// tbs_cap bytes.
NZ_HD void decode_one(const uint8_t* uri, uint64_t len, uint32_t max_tbs_bytes, const uint8_t* data20, uint8_t* cose,
                      uint8_t* tbs, nzcb_nzcp_pass* r, uint8_t* inputs_out, uint8_t* tbs_out, size_t tbs_cap) {
  *r = nzcb_nzcp_pass{};
  uint32_t start = 0, n = 0;
  if (len > kMaxUri) {
    fail(r, NZCB_PASS_ERR_LENGTH, (uint32_t)len);
  } else if (!parse_prefix(uri, (uint32_t)len, &r->version, &start)) {
    fail(r, NZCB_PASS_ERR_PREFIX, 0);
  } else {
    const uint32_t bad = b32_first_bad(uri, start, (uint32_t)len, 0, 1);
    if (bad != kNone) {
      fail(r, NZCB_PASS_ERR_BASE32, bad);
    } else {
      b32_decode(uri, start, (uint32_t)len, cose, 0, 1);
      n = b32_bytes((uint32_t)len - start);
      parse_cose(cose, n, r);
    }
  }
  if (r->status) {
    clear_failed(r);
  } else {
    r->tbs_len = tbs_length(r->protected_len, r->payload_len);
    tbs_fill(cose, r, tbs, 0, 1);
    sha256(tbs, r->tbs_len, r->tbs_sha256);
    r->fits = (max_tbs_bytes && r->tbs_len <= max_tbs_bytes) ? 1u : 0u;
  }
  if (inputs_out && max_tbs_bytes)
    inputs_fill(tbs, r->tbs_len, data20, max_tbs_bytes, r->fits != 0, inputs_out, 0, 1);
  if (tbs_out)
    for (size_t i = 0; i < tbs_cap; i++) tbs_out[i] = (!r->status && i < r->tbs_len) ? tbs[i] : 0;
}

}  // namespace nzdec
}  // namespace nzcb
