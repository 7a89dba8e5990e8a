// Groth16 key generation: setup and zkey contribute (include/nzcb.h nzcb_groth16_setup,
// nzcb_groth16_contribute, nzcb_groth16_vk_to_json; the first three lines of snarkjs's `phase2`
// recipe). What the kernels of groth16.hip and the host path (NZCB_GROTH16_HOST) share, the whole
// host path, and the reader and writer of the Groth16 zkey.
//
// THE LAYOUT WRITTEN HERE IS THE SPECIFICATION. snarkjs is not available to compare with: the
// file layout is restated from its published format and PARITY WITH snarkjs 0.4.12 IS UNPINNED
// (DESIGN.md). No circuit hash and no contribution records are written, so `snarkjs zkey verify`
// does not accept a key made here.
//
// The key. m constraints, nVars wires, nPublic = nOutputs + nPubInputs, cirPower =
// floor(log2(m + nPublic)) + 1, n = 2^cirPower. L12, L13, L14, L15: level cirPower of the
// prepared file's sections 12-15 ([L_c(tau)]G1, [L_c(tau)]G2, [alpha L_c(tau)]G1,
// [beta L_c(tau)]G1); T: level cirPower + 1 of section 12. With a, b, c the coefficients of
// constraint c' at signal s:
//   A[s]  = sum a L12[c']  (+ L12[m + s] for s <= nPublic)
//   B1[s] = sum b L12[c'],  B2[s] = sum b L13[c']
//   K[s]  = sum a L15[c'] + b L14[c'] + c L12[c']  (+ L15[m + s] for s <= nPublic)
//   IC = K[0..nPublic], C = K[nPublic + 1..], H[i] = T[2 i + 1],
//   alpha1, beta1, beta2 from sections 4, 5, 6; gamma2 = delta2 = [1]G2, delta1 = [1]G1.
//
// Every key point is a row of one sum-of-products family, out[row] = sum_t sign_t k_t P[idx_t]
// with k = min(c, r - c). A row is cut into chunks of bounded length and work, one lane per chunk; within
// a chunk the bits are walked from its longest k down with the doublings shared, so a chunk of
// unit coefficients costs its mixed additions and nothing else. Chunks are ordered by bit length
// (then by length), longest first, so the lanes of a wave run loops of about the same length.
// The chunk partials (XYZZ) of a row are folded with bounded fan-in, level by level, and each row
// is stored once in affine form: no atomics, and the bytes do not depend on the schedule.
//
// The header needs no HIP runtime: a host-only program may include it
// (tests/native/groth16_host.cpp).
#pragma once
#include <chrono>

#include "ptau_ops.h"
#include "r1cs_reader.h"

namespace nzcb {

// ---------------------------------------------------------------- terms, chunks, folds
// k: the low 30 bits are the coefficient itself, or with kG16Big its index in the table of long
// ones (normal form); kG16Neg: the term is subtracted
struct G16Term {
  uint32_t idx, k;
};
constexpr uint32_t kG16Neg = 1u << 31, kG16Big = 1u << 30, kG16Low = kG16Big - 1;
// terms [t0, t0 + len) of one row; bits: the longest k's bit length; slot: where the partial goes
struct G16Chunk {
  uint32_t t0, slot;
  uint16_t len, bits;
};
struct G16Fold {  // out = the sum of partials [begin, begin + count), count >= 1
  uint32_t begin, count;
};
constexpr uint32_t kG16NoSlot = ~0u;
constexpr uint32_t kG16DefaultChunk = 32, kG16DefaultFanIn = 8, kG16MaxKnob = 1024;

NZ_HD bool g16_bit(uint32_t k, const Fr* big, int b) {
  if (k & kG16Big) return (big[k & kG16Low].v[b >> 5] >> (b & 31)) & 1u;
  return b < 30 && ((k >> b) & 1u);
}

// the bit length of a term's k (never zero)
NZ_HD int g16_k_bits(uint32_t k, const Fr* big) {
  if (!(k & kG16Big)) return 32 - __builtin_clz((k & kG16Low) | 1u);
  const Fr& v = big[k & kG16Low];
  for (int i = 7; i > 0; i--)
    if (v.v[i]) return 32 * i + 32 - __builtin_clz(v.v[i]);
  return 32 - __builtin_clz(v.v[0] | 1u);
}

// One chunk: bits from the top down, one doubling per bit for the whole chunk, a mixed addition
// for each term whose bit is set. The plan has put the chunk's terms in the order of their bit
// lengths, longest first, so at bit b only the first `live` of them are looked at: a lane with two
// long coefficients among thirty units visits two terms per bit until bit 0, and the lanes of a
// wave, which step through their terms together, do not each pay for the others' long ones at
// every position. (0, 0) among the points is the point at infinity and is skipped.
template <class F>
NZ_HD PtXyzz<F> g16_chunk_sum(const PtAffine<F>* pts, const G16Term* terms, const Fr* big, const G16Chunk& c) {
  PtXyzz<F> acc = PtXyzz<F>::inf();
  uint32_t live = 0;
  for (int b = (int)c.bits - 1; b >= 0; b--) {
    if (b != (int)c.bits - 1) acc = pt_dbl(acc);
    while (live < c.len && g16_k_bits(terms[c.t0 + live].k, big) > b) live++;
    for (uint32_t t = c.t0; t < c.t0 + live; t++) {
      const G16Term tm = terms[t];
      if (!g16_bit(tm.k, big, b)) continue;
      const PtAffine<F> p = pts[tm.idx];
      if (p.is_inf()) continue;
      acc = pt_add_affine(acc, p.x, (tm.k & kG16Neg) ? neg(p.y) : p.y);
    }
  }
  return acc;
}

template <class F>
NZ_HD PtXyzz<F> g16_fold_sum(const PtXyzz<F>* in, const G16Fold& f) {
  PtXyzz<F> acc = in[f.begin];
  for (uint32_t j = 1; j < f.count; j++) acc = pt_add(acc, in[f.begin + j]);
  return acc;
}

// range and curve as pt_status; all zero bytes pass where the section may hold infinity
template <class F>
NZ_HD int g16_pt_status(const PtAffine<F>* p, const Fq2& b2, bool zero_ok) {
  const int st = pt_status<F>(p, b2);
  return st == NZCB_KEY_ERR_CURVE && zero_ok && p->is_inf() ? NZCB_KEY_OK : st;
}

// ---------------------------------------------------------------- rows (host)
// The transposed lists of one point family in CSR form.
struct G16Rows {
  uint64_t n_rows = 0, n_points = 0;
  std::vector<uint32_t> row_off;  // n_rows + 1
  std::vector<G16Term> terms;     // zero coefficients are not among them
  std::vector<Fr> big;
};

inline bool fr_less(const Fr& a, const Fr& b) {  // normal form
  uint32_t br = 0;
  for (int i = 0; i < 8; i++) (void)subb(a.v[i], b.v[i], br);
  return br != 0;
}

struct G16RowsBuilder {
  struct Raw {
    uint32_t row, idx, k;
  };
  uint64_t n_rows, n_points;
  std::vector<Raw> raw;
  std::vector<Fr> big;
  G16RowsBuilder(uint64_t rows, uint64_t points) : n_rows(rows), n_points(points) {
    if (rows >= kG16NoSlot || points > kG16NoSlot) throw Error(NZCB_ERR_ARG, "groth16: too many rows or points");
  }
  // coefficient in Montgomery form; recoded as k = min(c, r - c) and a sign
  void add(uint64_t row, uint64_t idx, const Fr& coef) {
    if (row >= n_rows || idx >= n_points) throw Error(NZCB_ERR_ARG, "groth16: a term is out of range");
    const Fr c = from_mont(coef);
    if (c.is_zero()) return;
    const Fr nc = Fr::modulus() - c;
    const bool negative = fr_less(nc, c);
    const Fr k = negative ? nc : c;
    uint32_t code = k.v[0];
    bool small = !(k.v[0] >> 30);
    for (int i = 1; i < 8; i++) small = small && !k.v[i];
    if (!small) {
      if (big.size() >= kG16Low) throw Error(NZCB_ERR_ARG, "groth16: too many long coefficients");
      code = kG16Big | (uint32_t)big.size();
      big.push_back(k);
    }
    if (raw.size() >= kG16NoSlot - 1) throw Error(NZCB_ERR_ARG, "groth16: too many terms");
    raw.push_back({(uint32_t)row, (uint32_t)idx, code | (negative ? kG16Neg : 0u)});
  }
  // by row (a counting sort)
  G16Rows finish() {
    G16Rows r;
    r.n_rows = n_rows;
    r.n_points = n_points;
    r.row_off.assign((size_t)n_rows + 1, 0);
    for (const Raw& t : raw) r.row_off[t.row + 1]++;
    for (uint64_t i = 0; i < n_rows; i++) r.row_off[i + 1] += r.row_off[i];
    r.terms.resize(raw.size());
    std::vector<uint32_t> at(r.row_off.begin(), r.row_off.end() - 1);
    for (const Raw& t : raw) r.terms[at[t.row]++] = G16Term{t.idx, t.k};
    r.big = std::move(big);
    raw.clear();
    raw.shrink_to_fit();
    return r;
  }
};

// The schedule of one family: the chunks in launch order, the fold levels and where each row's
// one partial ends up. Planning first puts the terms of each row in the order of their bit lengths,
// longest k first (a sum does not depend on the order of its terms): the long coefficients of a
// row then share chunks, the chunks of its unit coefficients cost no doubling, and within a
// chunk the order is the one g16_chunk_sum wants.
struct G16Plan {
  std::vector<G16Chunk> chunks;
  std::vector<std::vector<G16Fold>> levels;
  std::vector<uint32_t> final_slot;  // per row; kG16NoSlot: an empty row, the point at infinity
};
inline G16Plan g16_plan(G16Rows& r, uint32_t chunk, uint32_t fan_in) {
  if (chunk < 1 || chunk > kG16MaxKnob || fan_in < 2 || fan_in > kG16MaxKnob)
    throw Error(NZCB_ERR_ARG, "groth16: chunk length in 1..1024 and fan-in in 2..1024");
  G16Plan p;
  std::vector<uint32_t> off((size_t)r.n_rows), cnt((size_t)r.n_rows);
  std::vector<G16Chunk> cs;
  std::vector<uint32_t> hist((size_t)255 * (chunk + 1) + 1, 0);
  auto key = [&](const G16Chunk& c) { return (size_t)(254 - c.bits) * (chunk + 1) + (chunk - c.len); };
  uint32_t max_cnt = 0;
  for (uint64_t row = 0; row < r.n_rows; row++) {
    off[row] = (uint32_t)cs.size();
    if (r.row_off[row + 1] - r.row_off[row] > 1)
      std::stable_sort(r.terms.begin() + r.row_off[row], r.terms.begin() + r.row_off[row + 1],
                       [&](const G16Term& x, const G16Term& y) {
                         return g16_k_bits(x.k, r.big.data()) > g16_k_bits(y.k, r.big.data());
                       });
    for (uint32_t t0 = r.row_off[row], len; t0 < r.row_off[row + 1]; t0 += len) {
      // at most `chunk` terms and, past the first, at most 4 * chunk expected additions (half a
      // term's bits): a 254-bit coefficient gets a lane of its own, whose 254 doublings and ~127
      // additions are then the longest a lane runs
      uint32_t work = 0;
      for (len = 0; len < chunk && t0 + len < r.row_off[row + 1]; len++) {
        const uint32_t adds = std::max(1, g16_k_bits(r.terms[t0 + len].k, r.big.data()) / 2);
        if (len && work + adds > 4 * chunk) break;
        work += adds;
      }
      G16Chunk c;
      c.t0 = t0;
      c.slot = (uint32_t)cs.size();
      c.len = (uint16_t)len;
      c.bits = (uint16_t)g16_k_bits(r.terms[t0].k, r.big.data());
      hist[key(c) + 1]++;
      cs.push_back(c);
    }
    cnt[row] = (uint32_t)cs.size() - off[row];
    max_cnt = std::max(max_cnt, cnt[row]);
  }
  // counting sort: longest bit length first, then longest chunk first
  for (size_t i = 1; i < hist.size(); i++) hist[i] += hist[i - 1];
  p.chunks.resize(cs.size());
  for (const G16Chunk& c : cs) p.chunks[hist[key(c)]++] = c;
  while (max_cnt > 1) {
    std::vector<G16Fold> lv;
    max_cnt = 0;
    for (uint64_t row = 0; row < r.n_rows; row++) {
      const uint32_t begin = off[row], have = cnt[row];
      off[row] = (uint32_t)lv.size();
      for (uint32_t g = 0; g < have; g += fan_in) lv.push_back({begin + g, std::min(fan_in, have - g)});
      cnt[row] = (uint32_t)lv.size() - off[row];
      max_cnt = std::max(max_cnt, cnt[row]);
    }
    p.levels.push_back(std::move(lv));
  }
  p.final_slot.resize((size_t)r.n_rows);
  for (uint64_t row = 0; row < r.n_rows; row++) p.final_slot[row] = cnt[row] ? off[row] : kG16NoSlot;
  return p;
}

// The G1 rows of r over points already on `device` (groth16.hip k_g16_chunks, k_g16_fold,
// k_g16_store on a stream of the call's own), affine LEM into host memory at `out`; zero bytes for
// an empty row. The prover's signal basis is built with it (sigbasis.hip).
void g16_rows_g1_device(int device, const G1Pt* d_pts, const G16Rows& r, const G16Plan& plan, uint8_t* out);

// ---------------------------------------------------------------- schedule knob and timings
struct G16Schedule {
  uint32_t chunk = kG16DefaultChunk, fan_in = kG16DefaultFanIn;
};
inline G16Schedule& g16_schedule() {
  static G16Schedule s;
  return s;
}
// of the calling thread's last setup or contribute (nzcb_debug_groth16_timings)
enum {
  kG16MsKernels,  // every kernel below
  kG16MsCall,
  kG16MsRowsG1,
  kG16MsRowsG2,
  kG16MsTests,
  kG16MsScale,
  kG16MsPlan,  // host: reading the r1cs, the transposed lists and the schedule (wall)
  kG16TermsA,
  kG16TermsB1,
  kG16TermsB2,
  kG16TermsK,
  kG16ChunksG1,
  kG16ChunksG2,
  kG16StatCount
};
inline double* g16_stats() {
  thread_local double s[kG16StatCount] = {0};
  return s;
}
using G16Clock = std::chrono::steady_clock;
inline double g16_ms_since(G16Clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(G16Clock::now() - t0).count();
}
struct G16CallClock {
  G16Clock::time_point t0 = G16Clock::now();
  G16CallClock() {
    for (int i = 0; i < kG16StatCount; i++) g16_stats()[i] = 0;
  }
  ~G16CallClock() { g16_stats()[kG16MsCall] = g16_ms_since(t0); }
};

// `count` points of a file, possibly unaligned
struct G16Span {
  const uint8_t* p;
  uint64_t count;
};

// ---------------------------------------------------------------- the host backend
struct G16HostBackend {
  Fq2 b2 = g2_twist_b();

  template <class F>
  Tally test(const uint8_t* pts, uint64_t n, bool zero_ok) {
    Tally t;
    for (uint64_t i = 0; i < n; i++) {
      PtAffine<F> p;
      std::memcpy((void*)&p, pts + sizeof p * i, sizeof p);
      const int st = g16_pt_status<F>(&p, b2, zero_ok);
      if (st == NZCB_KEY_OK) continue;
      t.n_bad++;
      t.key = std::min(t.key, srs_bad_key(i, st));
    }
    return t;
  }
  // out[row] = the row's sum over the spans laid end to end, affine
  template <class F>
  void rows(const std::vector<G16Span>& spans, const G16Rows& r, const G16Plan& plan, uint8_t* out) {
    std::vector<PtAffine<F>> pts((size_t)r.n_points);
    size_t at = 0;
    for (const G16Span& s : spans) {
      if (s.count) std::memcpy((void*)(pts.data() + at), s.p, sizeof(PtAffine<F>) * (size_t)s.count);
      at += (size_t)s.count;
    }
    std::vector<PtXyzz<F>> a(plan.chunks.size()), b;
    parallel_for(plan.chunks.size(), [&](uint64_t i) {
      const G16Chunk& c = plan.chunks[i];
      a[c.slot] = g16_chunk_sum<F>(pts.data(), r.terms.data(), r.big.data(), c);
    });
    for (const auto& lv : plan.levels) {
      b.resize(lv.size());
      parallel_for(lv.size(), [&](uint64_t i) { b[i] = g16_fold_sum<F>(a.data(), lv[i]); });
      a.swap(b);
    }
    parallel_for(r.n_rows, [&](uint64_t row) {
      const uint32_t s = plan.final_slot[row];
      const PtAffine<F> v = s == kG16NoSlot ? PtAffine<F>{F::zero(), F::zero()} : pt_to_affine(a[s]);
      std::memcpy(out + sizeof v * row, &v, sizeof v);
    });
  }
  // dst[i] = k src[i], k in normal form
  template <class F>
  void scale(const uint8_t* src, uint64_t n, const Fr& k, uint8_t* dst) {
    parallel_for(n, [&](uint64_t i) {
      PtAffine<F> p;
      std::memcpy((void*)&p, src + sizeof p * i, sizeof p);
      p = pt_to_affine(pt_mul_affine(p, k));
      std::memcpy(dst + sizeof p * i, &p, sizeof p);
    });
  }
};

// ---------------------------------------------------------------- the zkey (host)
// section 2: n8q, q, n8r, r, nVars, nPublic, n, alpha1, beta1, beta2, gamma2, delta1, delta2
constexpr uint64_t kG16HeaderBytes = 4 + 32 + 4 + 32 + 12 + 64 + 64 + 128 + 128 + 64 + 128;
constexpr uint64_t kG16OffAlpha1 = 84, kG16OffBeta2 = 212, kG16OffGamma2 = 340, kG16OffDelta1 = 468,
                   kG16OffDelta2 = 532;

struct G16Zkey {
  KeySection s[11];  // by section id; s[0] unused
  uint32_t n_vars = 0, n_public = 0, n = 0;
};
inline G16Zkey g16_zkey_open(const uint8_t* d, size_t len) {
  G16Zkey z;
  z.s[1] = key_find_section(d, len, "zkey", 1);
  uint32_t protocol = 0;
  if (!z.s[1].p || z.s[1].len < 4) throw Error(NZCB_ERR_FORMAT, "zkey: section 1 is missing");
  std::memcpy(&protocol, z.s[1].p, 4);
  if (protocol != 1) throw Error(NZCB_ERR_FORMAT, "zkey file is not groth16");
  for (uint32_t id = 2; id <= 10; id++) {
    z.s[id] = key_find_section(d, len, "zkey", id);
    if (!z.s[id].p) throw Error(NZCB_ERR_FORMAT, "zkey: section " + std::to_string(id) + " is missing");
  }
  const KeySection& h = z.s[2];
  uint32_t n8 = 0, n8r = 0;
  if (h.len < kG16HeaderBytes) throw Error(NZCB_ERR_FORMAT, "zkey: header too short");
  std::memcpy(&n8, h.p, 4);
  std::memcpy(&n8r, h.p + 36, 4);
  if (n8 != 32 || n8r != 32 || std::memcmp(h.p + 4, FqParams::P, 32) != 0 ||
      std::memcmp(h.p + 40, FrParams::P, 32) != 0)
    throw Error(NZCB_ERR_FORMAT, "zkey: not a bn128 key");
  std::memcpy(&z.n_vars, h.p + 72, 4);
  std::memcpy(&z.n_public, h.p + 76, 4);
  std::memcpy(&z.n, h.p + 80, 4);
  if (z.n_public >= z.n_vars) throw Error(NZCB_ERR_FORMAT, "zkey: fewer wires than public signals");
  const uint64_t want[11] = {0, 4, kG16HeaderBytes, 64 * ((uint64_t)z.n_public + 1), 4, 64 * (uint64_t)z.n_vars,
                             64 * (uint64_t)z.n_vars, 128 * (uint64_t)z.n_vars,
                             64 * ((uint64_t)z.n_vars - z.n_public - 1), 64 * (uint64_t)z.n, 0};
  for (int id = 3; id <= 9; id++)
    if (z.s[id].len < want[id])
      throw Error(NZCB_ERR_FORMAT, "zkey: section " + std::to_string(id) + " is shorter than the header says");
  return z;
}

inline void g16_put_header(uint8_t* h, uint32_t n_vars, uint32_t n_public, uint32_t n, const uint8_t* alpha1,
                           const uint8_t* beta1, const uint8_t* beta2, const G1Pt& delta1, const G2Pt& gamma2,
                           const G2Pt& delta2) {
  const uint32_t n8 = 32;
  std::memcpy(h, &n8, 4);
  std::memcpy(h + 4, FqParams::P, 32);
  std::memcpy(h + 36, &n8, 4);
  std::memcpy(h + 40, FrParams::P, 32);
  std::memcpy(h + 72, &n_vars, 4);
  std::memcpy(h + 76, &n_public, 4);
  std::memcpy(h + 80, &n, 4);
  std::memcpy(h + kG16OffAlpha1, alpha1, 64);
  std::memcpy(h + kG16OffAlpha1 + 64, beta1, 64);
  std::memcpy(h + kG16OffBeta2, beta2, 128);
  std::memcpy(h + kG16OffGamma2, &gamma2, 128);
  std::memcpy(h + kG16OffDelta1, &delta1, 64);
  std::memcpy(h + kG16OffDelta2, &delta2, 128);
}

inline void g16_file_header(PtauOut& o) {
  o.put("zkey", 4);
  o.put_u32(1);
  o.put_u32(10);
}

inline std::string g16_bad_point(const char* file, const std::string& where, uint64_t index, const Tally& t) {
  const int st = (int)(t.key & 7u);
  return std::string(file) + ": " + where + " point " + std::to_string(index) +
         (st == NZCB_KEY_ERR_RANGE ? " has a coordinate that is not below q" : " is not on the curve") + " (" +
         std::to_string(t.n_bad) + " defective there)";
}

// ---------------------------------------------------------------- setup
struct G16Lagrange {  // sections 12-15 of a prepared file
  KeySection s[16];
};
inline G16Lagrange g16_lagrange_open(const uint8_t* d, size_t len, const PtauSections& f) {
  G16Lagrange l;
  const uint64_t n = uint64_t(1) << f.power;
  for (uint32_t id = 12; id <= 15; id++) {
    l.s[id] = key_find_section(d, len, "ptau", id);
    if (!l.s[id].p)
      throw Error(NZCB_ERR_FORMAT,
                  "ptau: not prepared for phase 2 (section " + std::to_string(id) + " is missing)");
    const uint64_t pts = id == 12 ? 4 * n - 1 : 2 * n - 1;
    if (l.s[id].len / PtauSections::point_bytes((int)id) < pts)
      throw Error(NZCB_ERR_FORMAT, "ptau: section " + std::to_string(id) + " is shorter than the header's power");
  }
  return l;
}

template <class Be>
void g16_setup(Be& be, const uint8_t* r1cs, size_t r1cs_len, const uint8_t* ptau, size_t ptau_len,
               const char* out_path, PtauOut& o) {
  if (!r1cs || !ptau) throw Error(NZCB_ERR_ARG, "null argument");
  double* stat = g16_stats();
  R1csFile rf = r1cs_open(r1cs, r1cs_len, "r1cs curve does not match powers of tau ceremony curve");
  const PtauSections f = ptau_sections_open(ptau, ptau_len);
  const G16Lagrange lag = g16_lagrange_open(ptau, ptau_len, f);
  const uint64_t m = rf.n_cons, n_vars = rf.n_wires, n_public = (uint64_t)rf.n_out + rf.n_pub_in;
  if (n_public >= n_vars) throw Error(NZCB_ERR_FORMAT, "r1cs: fewer wires than public signals");
  if (n_vars >= (1u << 30)) throw Error(NZCB_ERR_ARG, "groth16: more than 2^30 wires");
  int cir_power = 1;
  while (cir_power < 40 && ((m + n_public) >> cir_power)) cir_power++;
  if ((uint32_t)cir_power > f.power)
    throw Error(NZCB_ERR_ARG, "circuit too big for this power of tau ceremony. " + std::to_string(m) + "*2 > 2**" +
                                  std::to_string(f.power));
  const uint64_t n = uint64_t(1) << cir_power;
  const uint64_t lvl = n - 1, lvl_t = 2 * n - 1;  // where the levels begin in their sections
  const uint8_t* L12 = lag.s[12].p + 64 * lvl;
  const uint8_t* T = lag.s[12].p + 64 * lvl_t;
  const uint8_t* L13 = lag.s[13].p + 128 * lvl;
  const uint8_t* L14 = lag.s[14].p + 64 * lvl;
  const uint8_t* L15 = lag.s[15].p + 64 * lvl;

  // the transposed lists and section 4
  const auto t_plan = G16Clock::now();
  G16RowsBuilder b1(3 * n_vars, 3 * n), b2(n_vars, n);
  std::vector<uint8_t> coefs;
  uint32_t n_coefs = 0;
  auto put_coef = [&](uint32_t matrix, uint32_t constraint, uint32_t signal, const Fr& mont) {
    const Fr twice = to_mont(mont);
    uint8_t e[44];
    std::memcpy(e, &matrix, 4);
    std::memcpy(e + 4, &constraint, 4);
    std::memcpy(e + 8, &signal, 4);
    std::memcpy(e + 12, twice.v, 32);
    coefs.insert(coefs.end(), e, e + 44);
    if (++n_coefs == 0) throw Error(NZCB_ERR_ARG, "groth16: too many coefficients");
  };
  uint64_t n_a = 0, n_b = 0, n_c = 0;
  for (uint32_t c = 0; c < rf.n_cons; c++) {
    r1cs_read_lc(rf.constraints, rf.n_wires, [&](uint32_t s, const Fr& v) {
      put_coef(0, c, s, v);
      b1.add(s, c, v);
      b1.add(2 * n_vars + s, 2 * n + c, v);
      n_a++;
    });
    r1cs_read_lc(rf.constraints, rf.n_wires, [&](uint32_t s, const Fr& v) {
      put_coef(1, c, s, v);
      b1.add(n_vars + s, c, v);
      b1.add(2 * n_vars + s, n + c, v);
      b2.add(s, c, v);
      n_b++;
    });
    r1cs_read_lc(rf.constraints, rf.n_wires, [&](uint32_t s, const Fr& v) {
      b1.add(2 * n_vars + s, c, v);
      n_c++;
    });
  }
  for (uint64_t s = 0; s <= n_public; s++) {
    put_coef(0, (uint32_t)(m + s), (uint32_t)s, Fr::one());
    b1.add(s, m + s, Fr::one());
    b1.add(2 * n_vars + s, 2 * n + m + s, Fr::one());
  }
  G16Rows r1 = b1.finish(), r2 = b2.finish();
  const G16Schedule sch = g16_schedule();
  const G16Plan p1 = g16_plan(r1, sch.chunk, sch.fan_in), p2 = g16_plan(r2, sch.chunk, sch.fan_in);
  stat[kG16MsPlan] = g16_ms_since(t_plan);
  stat[kG16TermsA] = (double)(n_a + n_public + 1);
  stat[kG16TermsB1] = stat[kG16TermsB2] = (double)n_b;
  stat[kG16TermsK] = (double)(n_a + n_b + n_c + n_public + 1);
  stat[kG16ChunksG1] = (double)p1.chunks.size();
  stat[kG16ChunksG2] = (double)p2.chunks.size();

  // every point read, before any arithmetic
  auto test = [&](auto field, uint32_t id, const uint8_t* p, uint64_t count, uint64_t first, bool zero_ok) {
    using F = decltype(field);
    const Tally t = be.template test<F>(p, count, zero_ok);
    if (t.n_bad) throw Error(NZCB_ERR_FORMAT, g16_bad_point("ptau", "section " + std::to_string(id), first + (t.key >> 3), t));
  };
  test(Fq{}, 4, f.s[4].p, 1, 0, false);
  test(Fq{}, 5, f.s[5].p, 1, 0, false);
  test(Fq2{}, 6, f.s[6].p, 1, 0, false);
  test(Fq{}, 12, L12, n, lvl, true);
  test(Fq{}, 12, T, 2 * n, lvl_t, true);
  test(Fq2{}, 13, L13, n, lvl, true);
  test(Fq{}, 14, L14, n, lvl, true);
  test(Fq{}, 15, L15, n, lvl, true);

  const uint64_t n_c_pts = n_vars - n_public - 1;
  o.open(out_path, 12 + 10 * 12 + 4 + kG16HeaderBytes + 64 * (n_public + 1) + 4 + coefs.size() + 64 * n_vars +
                       64 * n_vars + 128 * n_vars + 64 * n_c_pts + 64 * n + 68);
  g16_file_header(o);
  const uint32_t groth16 = 1;
  std::memcpy(o.section(1, 4), &groth16, 4);
  g16_put_header(o.section(2, kG16HeaderBytes), (uint32_t)n_vars, (uint32_t)n_public, (uint32_t)n, f.s[4].p, f.s[5].p,
                 f.s[6].p, g1_gen_point(), g2_gen_point(), g2_gen_point());
  uint8_t* ic = o.section(3, 64 * (n_public + 1));
  uint8_t* s4 = o.section(4, 4 + coefs.size());
  std::memcpy(s4, &n_coefs, 4);
  if (!coefs.empty()) std::memcpy(s4 + 4, coefs.data(), coefs.size());
  uint8_t* sa = o.section(5, 64 * n_vars);
  uint8_t* sb1 = o.section(6, 64 * n_vars);
  uint8_t* sb2 = o.section(7, 128 * n_vars);
  uint8_t* sc = o.section(8, 64 * n_c_pts);
  uint8_t* sh = o.section(9, 64 * n);
  std::memset(o.section(10, 68), 0, 68);

  {
    std::vector<uint8_t> g1((size_t)(64 * 3 * n_vars));
    be.template rows<Fq>({{L12, n}, {L14, n}, {L15, n}}, r1, p1, g1.data());
    std::memcpy(sa, g1.data(), (size_t)(64 * n_vars));
    std::memcpy(sb1, g1.data() + 64 * n_vars, (size_t)(64 * n_vars));
    std::memcpy(ic, g1.data() + 128 * n_vars, (size_t)(64 * (n_public + 1)));
    if (n_c_pts) std::memcpy(sc, g1.data() + 128 * n_vars + 64 * (n_public + 1), (size_t)(64 * n_c_pts));
  }
  be.template rows<Fq2>({{L13, n}}, r2, p2, sb2);
  for (uint64_t i = 0; i < n; i++) std::memcpy(sh + 64 * i, T + 64 * (2 * i + 1), 64);
  o.commit();
}

// ---------------------------------------------------------------- contribute
// d: the secret in Montgomery form. C and H by 1/d, delta1 and delta2 by d; the rest is copied.
template <class Be>
void g16_contribute(Be& be, const uint8_t* zkey, size_t len, const Fr& d, const char* out_path, PtauOut& o) {
  if (!zkey) throw Error(NZCB_ERR_ARG, "null argument");
  const G16Zkey z = g16_zkey_open(zkey, len);
  const uint64_t n_c_pts = (uint64_t)z.n_vars - z.n_public - 1;
  auto test = [&](auto field, const std::string& where, const uint8_t* p, uint64_t count, bool zero_ok) {
    using F = decltype(field);
    const Tally t = be.template test<F>(p, count, zero_ok);
    if (t.n_bad) throw Error(NZCB_ERR_FORMAT, g16_bad_point("zkey", where, t.key >> 3, t));
  };
  test(Fq{}, "section 2 delta1,", z.s[2].p + kG16OffDelta1, 1, false);
  test(Fq2{}, "section 2 delta2,", z.s[2].p + kG16OffDelta2, 1, false);
  test(Fq{}, "section 8", z.s[8].p, n_c_pts, true);
  test(Fq{}, "section 9", z.s[9].p, z.n, true);

  uint64_t total = 12 + 10 * 12 + kG16HeaderBytes + 64 * n_c_pts + 64 * (uint64_t)z.n;
  for (int id : {1, 3, 4, 5, 6, 7, 10}) total += z.s[id].len;
  o.open(out_path, total);
  g16_file_header(o);
  auto copy = [&](int id) {
    uint8_t* dst = o.section((uint32_t)id, z.s[id].len);
    if (z.s[id].len) std::memcpy(dst, z.s[id].p, (size_t)z.s[id].len);
  };
  Fr dn = from_mont(d), di = from_mont(inverse(d));
  struct Wipe {
    Fr *a, *b;
    ~Wipe() {
      wipe(a, sizeof(Fr));
      wipe(b, sizeof(Fr));
    }
  } wiper{&dn, &di};
  copy(1);
  uint8_t* h = o.section(2, kG16HeaderBytes);
  std::memcpy(h, z.s[2].p, (size_t)kG16HeaderBytes);
  be.template scale<Fq>(z.s[2].p + kG16OffDelta1, 1, dn, h + kG16OffDelta1);
  be.template scale<Fq2>(z.s[2].p + kG16OffDelta2, 1, dn, h + kG16OffDelta2);
  for (int id = 3; id <= 7; id++) copy(id);
  be.template scale<Fq>(z.s[8].p, n_c_pts, di, o.section(8, 64 * n_c_pts));
  be.template scale<Fq>(z.s[9].p, z.n, di, o.section(9, 64 * (uint64_t)z.n));
  copy(10);
  o.commit();
}

// ---------------------------------------------------------------- the verification key as JSON
// a 256-bit LE normal-form value in decimal
inline std::string g16_dec(const uint32_t v[8]) {
  uint32_t w[8];
  std::memcpy(w, v, 32);
  std::string s;
  for (;;) {
    uint64_t rem = 0;
    bool any = false;
    for (int i = 7; i >= 0; i--) {
      const uint64_t cur = (rem << 32) | w[i];
      w[i] = (uint32_t)(cur / 1000000000u);
      rem = cur % 1000000000u;
      any = any || w[i];
    }
    char buf[16];
    std::snprintf(buf, sizeof buf, any ? "%09u" : "%u", (unsigned)rem);
    s.insert(0, buf);
    if (!any) return s;
  }
}
inline std::string g16_json_fq(const uint8_t* lem) {
  Fq x;
  std::memcpy(x.v, lem, 32);
  return "\"" + g16_dec(from_mont(x).v) + "\"";
}
inline std::string g16_json_g1(const uint8_t* p) {
  bool zero = true;
  for (int i = 0; i < 64; i++) zero = zero && !p[i];
  if (zero) return "[\"0\",\"1\",\"0\"]";
  return "[" + g16_json_fq(p) + "," + g16_json_fq(p + 32) + ",\"1\"]";
}
inline std::string g16_json_g2(const uint8_t* p) {
  bool zero = true;
  for (int i = 0; i < 128; i++) zero = zero && !p[i];
  if (zero) return "[[\"0\",\"0\"],[\"1\",\"0\"],[\"0\",\"0\"]]";
  return "[[" + g16_json_fq(p) + "," + g16_json_fq(p + 32) + "],[" + g16_json_fq(p + 64) + "," +
         g16_json_fq(p + 96) + "],[\"1\",\"0\"]]";
}
// protocol, curve, nPublic, vk_alpha_1, vk_beta_2, vk_gamma_2, vk_delta_2, IC. snarkjs's
// vk_alphabeta_12 is left out: its Fq12 layout cannot be pinned here, and neither snarkjs's
// verifier nor its Solidity template reads it.
inline std::string g16_vk_json(const uint8_t* zkey, size_t len) {
  if (!zkey) throw Error(NZCB_ERR_ARG, "null argument");
  const G16Zkey z = g16_zkey_open(zkey, len);
  const uint8_t* h = z.s[2].p;
  std::string s = "{\"protocol\":\"groth16\",\"curve\":\"bn128\",\"nPublic\":" + std::to_string(z.n_public);
  s += ",\"vk_alpha_1\":" + g16_json_g1(h + kG16OffAlpha1);
  s += ",\"vk_beta_2\":" + g16_json_g2(h + kG16OffBeta2);
  s += ",\"vk_gamma_2\":" + g16_json_g2(h + kG16OffGamma2);
  s += ",\"vk_delta_2\":" + g16_json_g2(h + kG16OffDelta2);
  s += ",\"IC\":[";
  for (uint32_t i = 0; i <= z.n_public; i++) s += (i ? "," : "") + g16_json_g1(z.s[3].p + 64 * (uint64_t)i);
  return s + "]}";
}

// ---------------------------------------------------------------- the kernel entry's lists
// CSR arrays as a caller gives them (nzcb_engine_groth16_rows): row_off n_rows + 1 ascending
// offsets from 0, idx below n_points, coefficients 32 B LE normal form below r.
inline G16Rows g16_rows_from_csr(uint64_t n_points, const uint64_t* row_off, uint64_t n_rows, const uint32_t* idx,
                                 const uint8_t* coefs) {
  if (!row_off || row_off[0] != 0) throw Error(NZCB_ERR_ARG, "groth16: row offsets begin at 0");
  G16RowsBuilder b(n_rows, n_points);
  for (uint64_t row = 0; row < n_rows; row++) {
    if (row_off[row + 1] < row_off[row]) throw Error(NZCB_ERR_ARG, "groth16: row offsets descend");
    for (uint64_t t = row_off[row]; t < row_off[row + 1]; t++) {
      Fr c;
      std::memcpy(c.v, coefs + 32 * t, 32);
      if (fr_noncanonical(c.v)) throw Error(NZCB_ERR_ARG, "groth16: a coefficient is not below r");
      b.add(row, idx[t], to_mont(c));
    }
  }
  return b.finish();
}

}  // namespace nzcb
