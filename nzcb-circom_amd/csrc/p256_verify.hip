// Batch ECDSA P-256 / SHA-256 verification (COSE ES256, the signature of an NZ COVID Pass) on the
// GPU: include/nzcb.h nzcb_p256_*. The arithmetic is csrc/p256.h, the same functions on both paths.
//
// A key object holds fixed-base window tables for G and for the public key Q (p256.h "fixed-base
// window tables": entry [j 2^w + d] = d 2^(w j) B, affine, Montgomery coordinates), built by
// k_p256_table with one lane per window row: the row's base by w j doublings, its 2^w - 1
// multiples by additions, and one inversion for the whole row. With them u1 G + u2 Q is
// 2 ceil(256 / w) mixed additions and no doubling. k_p256_verify takes one signature per lane:
// range check, z mod n, 1 / s by Fermat in F_n, u1 = z / s, u2 = r / s, the table sum, and
// X = r Z^2 (or (r + n) Z^2) in Jacobian coordinates. Workgroups are one wavefront, so a small
// batch spreads over the CUs. Digests and signatures are read where they lie: tightly packed
// buffers or the tbs_sha256 field of the nzcb_nzcp_record array nzcb_nzcp_witness_dev wrote.
//
// The arithmetic is exact, so the statuses do not depend on the batch, the order, the window
// width or the path (device = NZCB_P256_HOST: the same functions in host loops).
// A call owns its stream (unless the caller passes one) and its buffers and needs no prover
// context; it may run while a context proves on the same device.
#include <chrono>
#include <cstring>
#include <vector>

#include "devcall.h"
#include "p256.h"

namespace nzcb {
namespace {

using namespace p256;

// 8: 32 additions per base, 2 x 512 KiB of tables; 4: 64 additions, 2 x 64 KiB. Measured on
// MI355X (profiles/p256_verify.txt, DESIGN.md "Pass signature"): the verify kernel takes 1.39 ms
// at window 8 and 2.26 ms at window 4 for 512 signatures, and 8 is the faster at every batch
// size from 1 to 65536; its table build (9.2 ms against 4.0 ms) is paid once per key object.
// 4 stays reachable through nzcb_engine_p256_key_create for the tool's comparison.
constexpr int kDefaultWindow = 8;
constexpr unsigned kBlock = 64;  // one wavefront per workgroup
constexpr size_t kMaxProbe = size_t(1) << 24;

inline bool window_ok(int w) { return w == 4 || w == 8; }
inline size_t table_entries(int w) { return (size_t)table_windows(w) << w; }

// lane t builds row t % windows of G's (t < windows) or Q's table
__global__ __launch_bounds__(kBlock) void k_p256_table(Affine q, int w, Affine* __restrict__ tg,
                                                       Affine* __restrict__ tq, U256* __restrict__ zs,
                                                       U256* __restrict__ prods) {
  const int windows = table_windows(w);
  const int t = blockIdx.x * kBlock + threadIdx.x;
  if (t >= 2 * windows) return;
  const int j = t < windows ? t : t - windows;
  const Affine base = t < windows ? generator() : q;
  Affine* row = (t < windows ? tg : tq) + ((size_t)j << w);
  table_build_row(base, w, j, row, zs + ((size_t)t << w), prods + ((size_t)t << w));
}

// status[i] for signature i; grid covers count
__global__ __launch_bounds__(kBlock) void k_p256_verify(const Affine* __restrict__ tg, const Affine* __restrict__ tq,
                                                        int w, const uint8_t* __restrict__ hashes, size_t hash_stride,
                                                        const uint8_t* __restrict__ sigs, size_t sig_stride,
                                                        uint32_t count, int32_t* __restrict__ status) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= count) return;
  status[i] = verify_one(tg, tq, w, hashes + hash_stride * i, sigs + sig_stride * i);
}

// 64 bytes x || y of u1 G + u2 Q, big-endian normal form, zeros for the point at infinity
NZ_HD void mul2_affine(const Affine* tg, const Affine* tq, int w, const uint8_t* u1, const uint8_t* u2,
                       uint8_t* out) {
  const Jac r = mul2(tg, tq, w, load_be(u1), load_be(u2));
  U256 x = u_zero(), y = u_zero();
  if (!jac_is_infinity(r)) {
    const Affine a = jac_to_affine(r, inv<Fp>(r.z));
    x = from_mont<Fp>(a.x);
    y = from_mont<Fp>(a.y);
  }
  store_be(out, x);
  store_be(out + 32, y);
}

__global__ __launch_bounds__(kBlock) void k_p256_mul2(const Affine* __restrict__ tg, const Affine* __restrict__ tq,
                                                      int w, const uint8_t* __restrict__ u1,
                                                      const uint8_t* __restrict__ u2, uint32_t count,
                                                      uint8_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= count) return;
  mul2_affine(tg, tq, w, u1 + size_t(32) * i, u2 + size_t(32) * i, out + size_t(64) * i);
}

// the field probe: normal-form operands below the modulus, big-endian, normal-form result
template <class Par>
NZ_HD U256 field_op(int op, const U256& a, const U256& b) {
  switch (op) {
    case NZCB_P256_OP_ADD: return add<Par>(a, b);
    case NZCB_P256_OP_SUB: return sub<Par>(a, b);
    case NZCB_P256_OP_MUL: return mul<Par>(to_mont<Par>(a), b);  // Montgomery x normal = normal
    case NZCB_P256_OP_SQR: return from_mont<Par>(sqr<Par>(to_mont<Par>(a)));
    default: return from_mont<Par>(inv<Par>(to_mont<Par>(a)));
  }
}

NZ_HD void field_probe(int op, int field_n, const uint8_t* a, const uint8_t* b, uint8_t* out) {
  const U256 x = load_be(a), y = load_be(b);
  store_be(out, field_n ? field_op<Fn>(op, x, y) : field_op<Fp>(op, x, y));
}

__global__ __launch_bounds__(kBlock) void k_p256_field(int op, int field_n, const uint8_t* __restrict__ a,
                                                       const uint8_t* __restrict__ b, uint32_t count,
                                                       uint8_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= count) return;
  field_probe(op, field_n, a + size_t(32) * i, b + size_t(32) * i, out + size_t(32) * i);
}

// of the calling thread: the last key's table build (kernel ms; wall ms on the host path), the
// last verification's kernel ms and its wall ms
thread_local double g_times[3] = {0, 0, 0};

double wall_ms(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace
}  // namespace nzcb

using namespace nzcb;

struct nzcb_p256_key {
  int w = kDefaultWindow;
  std::vector<Affine> host;  // host path (dev.p is NULL): G's table, then Q's
  DeviceBlock dev;           // device path: the same, one allocation
  const Affine* tg = nullptr;
  const Affine* tq = nullptr;
};

namespace nzcb {
namespace {

void build(nzcb_p256_key& k, const uint8_t* pub_xy, int device, int w) {
  if (!window_ok(w)) throw Error(NZCB_ERR_ARG, "window width must be 4 or 8");
  const U256 x = load_be(pub_xy), y = load_be(pub_xy + 32);
  const U256 p = modulus<Fp>();
  if (!u_lt(x, p) || !u_lt(y, p) || (u_is_zero(x) && u_is_zero(y)) || !on_curve(x, y))
    throw Error(NZCB_ERR_ARG, "public key is not a point on P-256");
  Affine q;
  q.x = to_mont<Fp>(x);
  q.y = to_mont<Fp>(y);
  k.w = w;
  const int windows = table_windows(w);
  const size_t entries = table_entries(w);
  g_times[0] = 0;
  if (device == NZCB_P256_HOST) {
    const auto t0 = std::chrono::steady_clock::now();
    k.host.assign(2 * entries, Affine{u_zero(), u_zero()});
    std::vector<U256> zs(size_t(1) << w), prods(size_t(1) << w);
    for (int t = 0; t < 2 * windows; t++) {
      const int j = t < windows ? t : t - windows;
      Affine* row = k.host.data() + (t < windows ? 0 : entries) + ((size_t)j << w);
      table_build_row(t < windows ? generator() : q, w, j, row, zs.data(), prods.data());
    }
    k.tg = k.host.data();
    k.tq = k.host.data() + entries;
    g_times[0] = wall_ms(t0);
    return;
  }
  CallScope cs(device, nullptr, 2);
  k.dev.alloc(2 * entries * sizeof(Affine));
  Affine* tab = k.dev.at<Affine>(0);
  NZ_HIP(hipMemsetAsync(tab, 0, 2 * entries * sizeof(Affine), cs.st));  // the unused d = 0 slots
  const size_t tmp = (size_t(2) * windows) << w;
  U256* zs = cs.alloc<U256>(tmp * sizeof(U256));
  U256* prods = cs.alloc<U256>(tmp * sizeof(U256));
  cs.record(0);
  k_p256_table<<<grid_for(2 * windows, kBlock), kBlock, 0, cs.st>>>(q, w, tab, tab + entries, zs, prods);
  cs.record(1);
  NZ_HIP(hipGetLastError());
  NZ_HIP(hipStreamSynchronize(cs.st));
  g_times[0] = cs.elapsed(0, 1);
  k.tg = tab;
  k.tq = tab + entries;
}

nzcb_p256_key* create(const uint8_t* pub_xy, int device, int w, nzcb_err* err) {
  return guarded_new<nzcb_p256_key>(err, [&] {
    if (!pub_xy) throw Error(NZCB_ERR_ARG, "null argument");
    auto k = std::make_unique<nzcb_p256_key>();
    build(*k, pub_xy, device, w ? w : kDefaultWindow);
    return k;
  });
}

void verify(nzcb_p256_key* k, const uint8_t* hashes, size_t hash_stride, const uint8_t* sigs, size_t sig_stride,
            int count, bool on_device, int32_t* status_out, void* stream) {
  if (!k || count < 0) throw Error(NZCB_ERR_ARG, "bad argument");
  g_times[1] = g_times[2] = 0;
  if (!count) return;
  if (!hashes || !sigs || !status_out) throw Error(NZCB_ERR_ARG, "null argument");
  if (hash_stride < 32) throw Error(NZCB_ERR_ARG, "hash stride is shorter than a hash");
  if (sig_stride < 64) throw Error(NZCB_ERR_ARG, "signature stride is shorter than a signature");
  const auto t0 = std::chrono::steady_clock::now();
  if (!k->dev.p) {
    if (on_device) throw Error(NZCB_ERR_ARG, "a host key object cannot read device buffers");
    for (int i = 0; i < count; i++)
      status_out[i] = verify_one(k->tg, k->tq, k->w, hashes + hash_stride * (size_t)i, sigs + sig_stride * (size_t)i);
    g_times[2] = wall_ms(t0);
    return;
  }
  if (on_device && ((reinterpret_cast<uintptr_t>(hashes) | reinterpret_cast<uintptr_t>(sigs) | hash_stride |
                     sig_stride) & 3))
    throw Error(NZCB_ERR_ARG, "device hashes, signatures and their strides must be multiples of 4");
  CallScope cs(k->dev.device, stream, 2);
  const size_t n = (size_t)count;
  int32_t* d_status = cs.alloc<int32_t>(4 * n);
  if (!on_device) {
    // packed on the host, one copy each
    std::vector<uint8_t> hp, sp;
    const uint8_t* hsrc = hashes;
    const uint8_t* ssrc = sigs;
    if (hash_stride != 32) {
      hp.resize(32 * n);
      for (size_t i = 0; i < n; i++) std::memcpy(&hp[32 * i], hashes + hash_stride * i, 32);
      hsrc = hp.data();
    }
    if (sig_stride != 64) {
      sp.resize(64 * n);
      for (size_t i = 0; i < n; i++) std::memcpy(&sp[64 * i], sigs + sig_stride * i, 64);
      ssrc = sp.data();
    }
    uint8_t* d_h = cs.alloc<uint8_t>(32 * n);
    uint8_t* d_s = cs.alloc<uint8_t>(64 * n);
    NZ_HIP(hipMemcpyAsync(d_h, hsrc, 32 * n, hipMemcpyHostToDevice, cs.st));
    NZ_HIP(hipMemcpyAsync(d_s, ssrc, 64 * n, hipMemcpyHostToDevice, cs.st));
    NZ_HIP(hipStreamSynchronize(cs.st));  // hp, sp leave scope
    hashes = d_h;
    sigs = d_s;
    hash_stride = 32;
    sig_stride = 64;
  }
  cs.record(0);
  k_p256_verify<<<grid_for(n, kBlock, 1u << 26), kBlock, 0, cs.st>>>(k->tg, k->tq, k->w, hashes, hash_stride, sigs,
                                                                     sig_stride, (uint32_t)n, d_status);
  cs.record(1);
  NZ_HIP(hipGetLastError());
  NZ_HIP(hipMemcpyAsync(status_out, d_status, 4 * n, hipMemcpyDeviceToHost, cs.st));
  NZ_HIP(hipStreamSynchronize(cs.st));
  g_times[1] = cs.elapsed(0, 1);
  g_times[2] = wall_ms(t0);
}

void mul2_call(nzcb_p256_key* k, const uint8_t* u1, const uint8_t* u2, size_t count, uint8_t* out) {
  if (!k || count > kMaxProbe) throw Error(NZCB_ERR_ARG, "bad argument");
  if (!count) return;
  if (!u1 || !u2 || !out) throw Error(NZCB_ERR_ARG, "null argument");
  if (!k->dev.p) {
    for (size_t i = 0; i < count; i++) mul2_affine(k->tg, k->tq, k->w, u1 + 32 * i, u2 + 32 * i, out + 64 * i);
    return;
  }
  CallScope cs(k->dev.device, nullptr, 0);
  uint8_t* d1 = cs.alloc<uint8_t>(32 * count);
  uint8_t* d2 = cs.alloc<uint8_t>(32 * count);
  uint8_t* d_out = cs.alloc<uint8_t>(64 * count);
  NZ_HIP(hipMemcpyAsync(d1, u1, 32 * count, hipMemcpyHostToDevice, cs.st));
  NZ_HIP(hipMemcpyAsync(d2, u2, 32 * count, hipMemcpyHostToDevice, cs.st));
  k_p256_mul2<<<grid_for(count, kBlock, 1u << 26), kBlock, 0, cs.st>>>(k->tg, k->tq, k->w, d1, d2, (uint32_t)count,
                                                                       d_out);
  NZ_HIP(hipGetLastError());
  NZ_HIP(hipMemcpyAsync(out, d_out, 64 * count, hipMemcpyDeviceToHost, cs.st));
  NZ_HIP(hipStreamSynchronize(cs.st));
}

void field_call(int device, int op, int field, const uint8_t* a, const uint8_t* b, size_t count, uint8_t* out) {
  if (op < NZCB_P256_OP_ADD || op > NZCB_P256_OP_INV || (field != 0 && field != 1) || count > kMaxProbe)
    throw Error(NZCB_ERR_ARG, "bad argument");
  if (!count) return;
  if (!a || !b || !out) throw Error(NZCB_ERR_ARG, "null argument");
  const U256 m = field ? modulus<Fn>() : modulus<Fp>();
  for (size_t i = 0; i < count; i++)
    if (!u_lt(load_be(a + 32 * i), m) || !u_lt(load_be(b + 32 * i), m))
      throw Error(NZCB_ERR_ARG, "field probe operands must be below the modulus");
  if (device == NZCB_P256_HOST) {
    for (size_t i = 0; i < count; i++) field_probe(op, field, a + 32 * i, b + 32 * i, out + 32 * i);
    return;
  }
  CallScope cs(device, nullptr, 0);
  uint8_t* da = cs.alloc<uint8_t>(32 * count);
  uint8_t* db = cs.alloc<uint8_t>(32 * count);
  uint8_t* d_out = cs.alloc<uint8_t>(32 * count);
  NZ_HIP(hipMemcpyAsync(da, a, 32 * count, hipMemcpyHostToDevice, cs.st));
  NZ_HIP(hipMemcpyAsync(db, b, 32 * count, hipMemcpyHostToDevice, cs.st));
  k_p256_field<<<grid_for(count, kBlock, 1u << 26), kBlock, 0, cs.st>>>(op, field, da, db, (uint32_t)count, d_out);
  NZ_HIP(hipGetLastError());
  NZ_HIP(hipMemcpyAsync(out, d_out, 32 * count, hipMemcpyDeviceToHost, cs.st));
  NZ_HIP(hipStreamSynchronize(cs.st));
}

}  // namespace
}  // namespace nzcb

extern "C" {

nzcb_p256_key* nzcb_p256_key_create(const uint8_t pub_xy[64], int device, nzcb_err* err) {
  return create(pub_xy, device, 0, err);
}

nzcb_p256_key* nzcb_engine_p256_key_create(const uint8_t pub_xy[64], int device, int window, nzcb_err* err) {
  return create(pub_xy, device, window, err);
}

int nzcb_p256_verify(nzcb_p256_key* k, const void* hashes, size_t hash_stride, const void* sigs, size_t sig_stride,
                     int count, int on_device, int32_t* status_out, void* stream, nzcb_err* err) {
  return guarded(err, [&] {
    verify(k, static_cast<const uint8_t*>(hashes), hash_stride, static_cast<const uint8_t*>(sigs), sig_stride, count,
           on_device != 0, status_out, stream);
  });
}

void nzcb_p256_key_destroy(nzcb_p256_key* k) { delete k; }

int nzcb_debug_p256_field(int device, int op, int field, const uint8_t* a, const uint8_t* b, size_t count,
                          uint8_t* out, nzcb_err* err) {
  return guarded(err, [&] { field_call(device, op, field, a, b, count, out); });
}

int nzcb_debug_p256_mul2(nzcb_p256_key* k, const uint8_t* u1, const uint8_t* u2, size_t count, uint8_t* out_xy,
                         nzcb_err* err) {
  return guarded(err, [&] { mul2_call(k, u1, u2, count, out_xy); });
}

int nzcb_debug_p256_timings(double* ms, int cap) {
  int k = 0;
  for (; ms && k < cap && k < 3; k++) ms[k] = g_times[k];
  return k;
}

}  // extern "C"
