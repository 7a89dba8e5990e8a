// Groth16 setup and zkey contribute on the GPU (include/nzcb.h nzcb_groth16_setup,
// nzcb_groth16_contribute; snarkjs's `groth16 setup` and `zkey contribute`). groth16.h holds the
// key's definition, the file layout (which is the specification: parity with snarkjs 0.4.12 is
// unpinned), the schedule and the host path; this file holds the device backend of the same
// drivers and the C-ABI.
//
// Kernels, each a template over the coordinate field (Fq for G1, Fq2 for G2):
//   k_g16_test    one lane per point read: range and curve, count and lowest index;
//   k_g16_chunks  one lane per chunk of a row (bounded length and work), in the plan's order
//                 (longest bit length first), the XYZZ partial stored at the chunk's slot;
//   k_g16_fold    one lane per group of up to fan-in partials of one row, run once per level;
//   k_g16_store   one lane per row: the one partial left, affine (zero bytes for an empty row);
//   k_g16_scale   one lane per point of a contribution: the same scalar in every lane.
// Blocks are one wave. A G2 accumulator with one mixed addend is about 100 live words before the
// temporaries of an addition, so a lane wants most of the register file and a CU holds few
// waves either way; with one wave per block a wave of long coefficients keeps nothing but
// itself waiting, and the waves after it (shorter loops, by the plan's order) fill the other SIMDs.
// Only the levels a setup reads are uploaded, never whole sections. A call owns its stream and
// buffers (devcall.h CallScope) and needs no prover context.
#include "devcall.h"
#include "groth16.h"

namespace nzcb {

namespace {

constexpr unsigned kGB = 64;

template <class F>
__global__ __launch_bounds__(kGB) void k_g16_test(const PtAffine<F>* __restrict__ pts, uint64_t n, Fq2 b2,
                                                  int zero_ok, unsigned long long* res) {
  const uint64_t i = (uint64_t)blockIdx.x * kGB + threadIdx.x;
  if (i >= n) return;
  const PtAffine<F> p = pts[i];
  const int st = g16_pt_status<F>(&p, b2, zero_ok != 0);
  if (st != NZCB_KEY_OK) {
    atomicAdd(&res[0], 1ull);
    atomicMin(&res[1], (unsigned long long)srs_bad_key(i, st));
  }
}

template <class F>
__global__ __launch_bounds__(kGB) void k_g16_chunks(const PtAffine<F>* __restrict__ pts,
                                                    const G16Term* __restrict__ terms, const Fr* __restrict__ big,
                                                    const G16Chunk* __restrict__ chunks, uint32_t n_chunks,
                                                    PtXyzz<F>* __restrict__ part) {
  const uint32_t i = blockIdx.x * kGB + threadIdx.x;
  if (i >= n_chunks) return;
  const G16Chunk c = chunks[i];
  part[c.slot] = g16_chunk_sum<F>(pts, terms, big, c);
}

template <class F>
__global__ __launch_bounds__(kGB) void k_g16_fold(const PtXyzz<F>* __restrict__ in, const G16Fold* __restrict__ folds,
                                                  uint32_t n_out, PtXyzz<F>* __restrict__ out) {
  const uint32_t i = blockIdx.x * kGB + threadIdx.x;
  if (i >= n_out) return;
  out[i] = g16_fold_sum<F>(in, folds[i]);
}

template <class F>
__global__ __launch_bounds__(kGB) void k_g16_store(const PtXyzz<F>* __restrict__ part,
                                                   const uint32_t* __restrict__ final_slot, uint32_t n_rows,
                                                   PtAffine<F>* __restrict__ out) {
  const uint32_t row = blockIdx.x * kGB + threadIdx.x;
  if (row >= n_rows) return;
  const uint32_t s = final_slot[row];
  out[row] = s == kG16NoSlot ? PtAffine<F>{F::zero(), F::zero()} : pt_to_affine(part[s]);
}

// pts[i] = k pts[i]; k normal form, in device memory the call wipes
template <class F>
__global__ __launch_bounds__(kGB) void k_g16_scale(PtAffine<F>* __restrict__ pts, uint64_t n,
                                                   const Fr* __restrict__ k) {
  const uint64_t i = (uint64_t)blockIdx.x * kGB + threadIdx.x;
  if (i >= n) return;
  const PtAffine<F> p = pts[i];
  pts[i] = pt_to_affine(pt_mul_affine(p, *k));
}

struct G16DeviceBackend {
  CallScope cs;  // first: the buffers below are freed on its device
  Fq2 b2 = g2_twist_b();
  unsigned long long* d_res;
  Fr* d_k;  // the scalar of a contribution

  explicit G16DeviceBackend(int device) : cs(device, nullptr, 2) {
    d_res = cs.alloc<unsigned long long>(16);
    d_k = cs.alloc<Fr>(sizeof(Fr));
  }
  ~G16DeviceBackend() {
    (void)hipMemsetAsync(d_k, 0, sizeof(Fr), cs.st);
    (void)hipStreamSynchronize(cs.st);
  }
  void took(int which) {
    const double ms = cs.elapsed(0, 1);
    g16_stats()[which] += ms;
    g16_stats()[kG16MsKernels] += ms;
  }
  template <class F>
  Tally test(const uint8_t* pts, uint64_t n, bool zero_ok) {
    Tally t;
    if (!n) return t;
    DevBuf<uint8_t> d(sizeof(PtAffine<F>) * n);
    const unsigned long long init[2] = {0, kNoBadKey};
    unsigned long long h[2];
    NZ_HIP(hipMemcpyAsync(d_res, init, sizeof init, hipMemcpyHostToDevice, cs.st));
    NZ_HIP(hipMemcpyAsync(d.p, pts, d.n, hipMemcpyHostToDevice, cs.st));
    cs.record(0);
    k_g16_test<F><<<grid_for(n, kGB, 1u << 30), kGB, 0, cs.st>>>(reinterpret_cast<const PtAffine<F>*>(d.p), n, b2,
                                                                  zero_ok ? 1 : 0, d_res);
    NZ_HIP(hipGetLastError());
    cs.record(1);
    NZ_HIP(hipMemcpyAsync(h, d_res, sizeof h, hipMemcpyDeviceToHost, cs.st));
    NZ_HIP(hipStreamSynchronize(cs.st));
    took(kG16MsTests);
    t.n_bad = h[0];
    t.key = h[1];
    return t;
  }
  // the rows of r over points already on the device, affine, into host memory at `out`
  template <class F>
  void rows_on(const PtAffine<F>* d_pts, const G16Rows& r, const G16Plan& plan, uint8_t* out) {
    using X = PtXyzz<F>;
    if (!r.n_rows) return;
    const size_t n_chunks = plan.chunks.size();
    size_t second = 1;
    for (const auto& lv : plan.levels) second = std::max(second, lv.size());
    DevBuf<G16Term> d_terms(std::max<size_t>(1, r.terms.size()));
    DevBuf<Fr> d_big(std::max<size_t>(1, r.big.size()));
    DevBuf<G16Chunk> d_chunks(std::max<size_t>(1, n_chunks));
    DevBuf<G16Fold> d_folds(second);
    DevBuf<uint32_t> d_final((size_t)r.n_rows);
    DevBuf<X> d_a(std::max<size_t>(1, n_chunks)), d_b(second);
    DevBuf<PtAffine<F>> d_out((size_t)r.n_rows);
    auto up = [&](void* dst, const void* src, size_t bytes) {
      if (bytes) NZ_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, cs.st));
    };
    up(d_terms.p, r.terms.data(), r.terms.size() * sizeof(G16Term));
    up(d_big.p, r.big.data(), r.big.size() * sizeof(Fr));
    up(d_chunks.p, plan.chunks.data(), n_chunks * sizeof(G16Chunk));
    up(d_final.p, plan.final_slot.data(), plan.final_slot.size() * sizeof(uint32_t));
    cs.record(0);
    if (n_chunks) {
      k_g16_chunks<F><<<grid_for(n_chunks, kGB, 1u << 30), kGB, 0, cs.st>>>(d_pts, d_terms.p, d_big.p, d_chunks.p,
                                                                             (uint32_t)n_chunks, d_a.p);
      NZ_HIP(hipGetLastError());
    }
    X *in = d_a.p, *nxt = d_b.p;
    for (const auto& lv : plan.levels) {
      // the stream orders this copy after the level before it, which read the same array
      up(d_folds.p, lv.data(), lv.size() * sizeof(G16Fold));
      k_g16_fold<F><<<grid_for(lv.size(), kGB, 1u << 30), kGB, 0, cs.st>>>(in, d_folds.p, (uint32_t)lv.size(), nxt);
      NZ_HIP(hipGetLastError());
      // the host vector must outlive the copy
      NZ_HIP(hipStreamSynchronize(cs.st));
      std::swap(in, nxt);
    }
    k_g16_store<F><<<grid_for(r.n_rows, kGB, 1u << 30), kGB, 0, cs.st>>>(in, d_final.p, (uint32_t)r.n_rows, d_out.p);
    NZ_HIP(hipGetLastError());
    cs.record(1);
    NZ_HIP(hipMemcpyAsync(out, d_out.p, sizeof(PtAffine<F>) * (size_t)r.n_rows, hipMemcpyDeviceToHost, cs.st));
    NZ_HIP(hipStreamSynchronize(cs.st));
    took(std::is_same<F, Fq>::value ? kG16MsRowsG1 : kG16MsRowsG2);
  }
  template <class F>
  void rows(const std::vector<G16Span>& spans, const G16Rows& r, const G16Plan& plan, uint8_t* out) {
    DevBuf<PtAffine<F>> d_pts(std::max<size_t>(1, (size_t)r.n_points));
    size_t at = 0;
    for (const G16Span& s : spans) {
      if (s.count)
        NZ_HIP(hipMemcpyAsync(d_pts.p + at, s.p, sizeof(PtAffine<F>) * (size_t)s.count, hipMemcpyHostToDevice, cs.st));
      at += (size_t)s.count;
    }
    if (at != r.n_points) throw Error(NZCB_ERR_INTERNAL, "groth16: point count mismatch");
    rows_on<F>(d_pts.p, r, plan, out);
  }
  template <class F>
  void scale(const uint8_t* src, uint64_t n, const Fr& k, uint8_t* dst) {
    if (!n) return;
    DevBuf<uint8_t> d(sizeof(PtAffine<F>) * n);
    NZ_HIP(hipMemcpyAsync(d_k, &k, sizeof k, hipMemcpyHostToDevice, cs.st));
    NZ_HIP(hipMemcpyAsync(d.p, src, d.n, hipMemcpyHostToDevice, cs.st));
    cs.record(0);
    k_g16_scale<F><<<grid_for(n, kGB, 1u << 30), kGB, 0, cs.st>>>(reinterpret_cast<PtAffine<F>*>(d.p), n, d_k);
    NZ_HIP(hipGetLastError());
    cs.record(1);
    NZ_HIP(hipMemsetAsync(d_k, 0, sizeof(Fr), cs.st));
    NZ_HIP(hipMemcpyAsync(dst, d.p, d.n, hipMemcpyDeviceToHost, cs.st));
    NZ_HIP(hipStreamSynchronize(cs.st));  // d is freed on return
    took(kG16MsScale);
  }
};

void setup_on(int device, const uint8_t* r1cs, size_t r1cs_len, const uint8_t* ptau, size_t ptau_len,
              const char* out_path, PtauOut& o) {
  G16CallClock clock;
  if (device == NZCB_GROTH16_HOST) {
    G16HostBackend be;
    g16_setup(be, r1cs, r1cs_len, ptau, ptau_len, out_path, o);
  } else {
    G16DeviceBackend be(device);
    g16_setup(be, r1cs, r1cs_len, ptau, ptau_len, out_path, o);
  }
}

struct Secret {
  Fr d;
  ~Secret() { wipe(&d, sizeof d); }
};

void contribute_on(int device, const uint8_t* zkey, size_t len, const uint8_t* secret, const uint8_t* entropy,
                   size_t entropy_len, const char* out_path, PtauOut& o) {
  if (!zkey) throw Error(NZCB_ERR_ARG, "null argument");
  G16CallClock clock;
  (void)g16_zkey_open(zkey, len);  // a file that is no Groth16 key costs no randomness
  Secret sec;
  make_secrets(secret, entropy, entropy_len, &sec.d, 1, "zkey");
  if (device == NZCB_GROTH16_HOST) {
    G16HostBackend be;
    g16_contribute(be, zkey, len, sec.d, out_path, o);
  } else {
    G16DeviceBackend be(device);
    g16_contribute(be, zkey, len, sec.d, out_path, o);
  }
}

void require_distinct(const char* in_path, const char* out_path, const char* what) {
  struct stat a, b;
  if (stat(in_path, &a) == 0 && stat(out_path, &b) == 0 && a.st_dev == b.st_dev && a.st_ino == b.st_ino)
    throw Error(NZCB_ERR_ARG, std::string(what) + ": the output path is an input file");
}

void give(PtauOut& o, uint8_t** out, size_t* out_len) {
  *out_len = (size_t)o.len;
  *out = o.release();
}

}  // namespace

void g16_rows_g1_device(int device, const G1Pt* d_pts, const G16Rows& r, const G16Plan& plan, uint8_t* out) {
  G16DeviceBackend be(device);
  be.rows_on<Fq>(d_pts, r, plan, out);
}

}  // namespace nzcb

using namespace nzcb;

extern "C" {

int nzcb_groth16_setup(const uint8_t* r1cs, size_t r1cs_len, const uint8_t* ptau, size_t ptau_len, int device,
                       uint8_t** zkey_out, size_t* zkey_len, nzcb_err* err) {
  return guarded(err, [&] {
    if (!zkey_out || !zkey_len) throw Error(NZCB_ERR_ARG, "null argument");
    PtauOut o;
    setup_on(device, r1cs, r1cs_len, ptau, ptau_len, nullptr, o);
    give(o, zkey_out, zkey_len);
  });
}

int nzcb_groth16_setup_file(const char* r1cs_path, const char* ptau_path, const char* zkey_path, int device,
                            nzcb_err* err) {
  return guarded(err, [&] {
    if (!r1cs_path || !ptau_path || !zkey_path) throw Error(NZCB_ERR_ARG, "null argument");
    require_distinct(r1cs_path, zkey_path, "groth16");
    require_distinct(ptau_path, zkey_path, "groth16");
    MappedFile rf(r1cs_path, "the r1cs", "r1cs: invalid file format");
    MappedFile pf(ptau_path, "the ptau", "ptau: invalid file format");
    PtauOut o;
    setup_on(device, rf.data, rf.size, pf.data, pf.size, zkey_path, o);
  });
}

int nzcb_groth16_contribute(const uint8_t* zkey, size_t len, const uint8_t* secret, const uint8_t* entropy,
                            size_t entropy_len, int device, uint8_t** zkey_out, size_t* zkey_len, nzcb_err* err) {
  return guarded(err, [&] {
    if (!zkey_out || !zkey_len) throw Error(NZCB_ERR_ARG, "null argument");
    PtauOut o;
    contribute_on(device, zkey, len, secret, entropy, entropy_len, nullptr, o);
    give(o, zkey_out, zkey_len);
  });
}

int nzcb_groth16_contribute_file(const char* in_path, const char* out_path, const uint8_t* secret,
                                 const uint8_t* entropy, size_t entropy_len, int device, nzcb_err* err) {
  return guarded(err, [&] {
    if (!in_path || !out_path) throw Error(NZCB_ERR_ARG, "null argument");
    require_distinct(in_path, out_path, "zkey");
    MappedFile mf(in_path, "the zkey", "zkey: invalid file format");
    PtauOut o;
    contribute_on(device, mf.data, mf.size, secret, entropy, entropy_len, out_path, o);
  });
}

int nzcb_groth16_vk_to_json(const uint8_t* zkey, size_t len, char* out, size_t cap) {
  nzcb_err err;
  std::string s;
  const int rc = guarded(&err, [&] { s = g16_vk_json(zkey, len); });
  if (rc != 0) {
    if (out && cap) std::snprintf(out, cap, "%s", err.msg);
    return rc;
  }
  if (!out || cap < s.size() + 1) return -(int)(s.size() + 1);
  std::memcpy(out, s.c_str(), s.size() + 1);
  return 0;
}

int nzcb_groth16_vk_to_json_file(const char* zkey_path, char* out, size_t cap) {
  nzcb_err err;
  std::string s;
  const int rc = guarded(&err, [&] {
    if (!zkey_path) throw Error(NZCB_ERR_ARG, "null argument");
    MappedFile mf(zkey_path, "the zkey", "zkey: invalid file format");
    s = g16_vk_json(mf.data, mf.size);
  });
  if (rc != 0) {
    if (out && cap) std::snprintf(out, cap, "%s", err.msg);
    return rc;
  }
  if (!out || cap < s.size() + 1) return -(int)(s.size() + 1);
  std::memcpy(out, s.c_str(), s.size() + 1);
  return 0;
}

int nzcb_engine_groth16_rows(int device, int g2, const void* points, uint64_t n_points, const uint64_t* row_off,
                             uint64_t n_rows, const uint32_t* idx, const uint8_t* coefs, uint8_t* out,
                             nzcb_err* err) {
  return guarded(err, [&] {
    if (!row_off || !out || (n_points && !points)) throw Error(NZCB_ERR_ARG, "null argument");
    if (row_off[n_rows] && (!idx || !coefs)) throw Error(NZCB_ERR_ARG, "null argument");
    G16CallClock clock;
    G16Rows r = g16_rows_from_csr(n_points, row_off, n_rows, idx, coefs);
    const G16Schedule sch = g16_schedule();
    const G16Plan plan = g16_plan(r, sch.chunk, sch.fan_in);
    if (device == NZCB_GROTH16_HOST) {
      G16HostBackend be;
      const std::vector<G16Span> spans = {{static_cast<const uint8_t*>(points), n_points}};
      if (g2)
        be.rows<Fq2>(spans, r, plan, out);
      else
        be.rows<Fq>(spans, r, plan, out);
    } else {
      G16DeviceBackend be(device);
      if (g2)
        be.rows_on<Fq2>(static_cast<const G2Pt*>(points), r, plan, out);
      else
        be.rows_on<Fq>(static_cast<const G1Pt*>(points), r, plan, out);
    }
  });
}

int nzcb_debug_groth16_schedule(int chunk, int fan_in, int* prev_chunk, int* prev_fan_in) {
  G16Schedule& s = g16_schedule();
  if (prev_chunk) *prev_chunk = (int)s.chunk;
  if (prev_fan_in) *prev_fan_in = (int)s.fan_in;
  if (chunk > (int)kG16MaxKnob || fan_in > (int)kG16MaxKnob || fan_in == 1) return NZCB_ERR_ARG;
  s.chunk = chunk <= 0 ? kG16DefaultChunk : (uint32_t)chunk;
  s.fan_in = fan_in <= 0 ? kG16DefaultFanIn : (uint32_t)fan_in;
  return 0;
}

int nzcb_debug_groth16_timings(double* out, int cap) {
  int k = 0;
  for (; out && k < cap && k < kG16StatCount; k++) out[k] = g16_stats()[k];
  return k;
}

}  // extern "C"
