// NZ COVID Pass URIs decoded on the GPU: include/nzcb.h nzcb_nzcp_decode(_dev). The decoding
// itself is csrc/nzcp_decode.h, the same functions on both paths; this file is the kernel that
// spreads one pass over a workgroup, and the C ABI.
//
// k_nzcp_decode: one pass per 64-lane workgroup (one wavefront). The URI, the COSE bytes and the
// ToBeSigned live in LDS (about 5 KiB with the record), so the untrusted bytes are read from HBM
// once, inside [offsets[i], offsets[i + 1]), and every later index is checked against a length
// that is in LDS or a register. The alphabet check (with a minimum over the lanes for the index
// reported), the base32 decode (each output byte is a function of three digits), the copies into
// the Sig_structure and the pass's block of input signals (16-byte stores, consecutive lanes on
// consecutive addresses: 95 KB per pass for nzcp_live, the kernel's only sizeable traffic) run
// across the lanes; the CBOR walk (a few dozen heads) and SHA-256 (at most 21 blocks) run on
// lane 0. One lane per pass would turn the input block into 64 scattered streams and the parse
// into 64 divergent ones.
#include <chrono>
#include <vector>

#include "devcall.h"
#include "nzcp_decode.h"

namespace nzcb {
namespace nzdec {
namespace {

constexpr unsigned kLanes = 64;
constexpr uint32_t kRecWords = sizeof(nzcb_nzcp_pass) / 4;
static_assert(sizeof(nzcb_nzcp_pass) % 8 == 0, "the record array is read in place with 8-byte fields");
static_assert(offsetof(nzcb_nzcp_pass, sig) % 4 == 0 && offsetof(nzcb_nzcp_pass, tbs_sha256) % 4 == 0,
              "nzcb_p256_verify reads both in place");

struct Stage {
  alignas(16) uint8_t uri[kMaxUri];
  alignas(16) uint8_t cose[kMaxCose];
  alignas(16) uint8_t tbs[kMaxTbs];
  alignas(8) nzcb_nzcp_pass rec;
  uint8_t data[kDataBytes];
};

__global__ __launch_bounds__(kLanes) void k_nzcp_decode(const uint8_t* __restrict__ uris,
                                                        const uint32_t* __restrict__ offsets, uint32_t max_tbs_bytes,
                                                        const uint8_t* __restrict__ data20,
                                                        nzcb_nzcp_pass* __restrict__ passes,
                                                        uint8_t* __restrict__ inputs, uint8_t* __restrict__ tbs_out,
                                                        size_t tbs_stride) {
  __shared__ Stage sh;
  const size_t pass = blockIdx.x;
  const uint32_t lane = threadIdx.x;
  const uint32_t o0 = offsets[pass], o1 = offsets[pass + 1];
  // the entry points reject decreasing offsets; should one arrive anyway, the pass is too long
  const uint64_t len = o1 >= o0 ? (uint64_t)(o1 - o0) : (uint64_t)1 << 32;

  // every branch below is uniform over the workgroup: its conditions are in LDS or the same in
  // every lane
  int status = 0;
  uint32_t detail = 0, version = 0, start = 0, n = 0;
  if (len <= kMaxUri)
    for (uint32_t i = lane; i < (uint32_t)len; i += kLanes) sh.uri[i] = uris[(size_t)o0 + i];
  __syncthreads();
  if (len > kMaxUri) {
    status = NZCB_PASS_ERR_LENGTH;
    detail = (uint32_t)len;
  } else if (!parse_prefix(sh.uri, (uint32_t)len, &version, &start)) {
    status = NZCB_PASS_ERR_PREFIX;
  } else {
    uint32_t bad = b32_first_bad(sh.uri, start, (uint32_t)len, lane, kLanes);
    for (int d = kLanes / 2; d; d >>= 1) {
      const uint32_t other = __shfl_xor(bad, d);
      bad = other < bad ? other : bad;
    }
    if (bad != kNone) {
      status = NZCB_PASS_ERR_BASE32;
      detail = bad;
    } else {
      b32_decode(sh.uri, start, (uint32_t)len, sh.cose, lane, kLanes);
      n = b32_bytes((uint32_t)len - start);
    }
  }
  if (data20 && lane < kDataBytes) sh.data[lane] = data20[pass * kDataBytes + lane];
  __syncthreads();
  if (lane == 0) {
    sh.rec = nzcb_nzcp_pass{};
    sh.rec.version = version;
    if (status)
      fail(&sh.rec, status, detail);
    else
      parse_cose(sh.cose, n, &sh.rec);
    if (sh.rec.status)
      clear_failed(&sh.rec);
    else
      sh.rec.tbs_len = tbs_length(sh.rec.protected_len, sh.rec.payload_len);
  }
  __syncthreads();
  const bool good = sh.rec.status == 0;
  const uint32_t tbs_len = sh.rec.tbs_len;
  const bool fits = good && max_tbs_bytes && tbs_len <= max_tbs_bytes;
  if (good) tbs_fill(sh.cose, &sh.rec, sh.tbs, lane, kLanes);
  __syncthreads();
  if (good && lane == 0) {
    sha256(sh.tbs, tbs_len, sh.rec.tbs_sha256);
    sh.rec.fits = fits ? 1u : 0u;
  }
  if (inputs && max_tbs_bytes)
    inputs_fill(sh.tbs, tbs_len, data20 ? sh.data : nullptr, max_tbs_bytes, fits,
                inputs + pass * ((size_t)input_signals(max_tbs_bytes) * 32), lane, kLanes);
  if (tbs_out)
    for (size_t i = lane; i < tbs_stride; i += kLanes)
      tbs_out[pass * tbs_stride + i] = (good && i < tbs_len) ? sh.tbs[i] : 0;
  __syncthreads();
  const uint32_t* src = reinterpret_cast<const uint32_t*>(&sh.rec);
  uint32_t* dst = reinterpret_cast<uint32_t*>(passes + pass);
  for (uint32_t i = lane; i < kRecWords; i += kLanes) dst[i] = src[i];
}

// of the calling thread's last nzcb_nzcp_decode: kernel ms (0 on the host path), wall ms
thread_local double g_times[2] = {0, 0};

uint32_t max_tbs_of(const nzcb_nzcp_params* prm) {
  if (!prm) return 0;
  if (prm->max_tbs_bytes < 1 || prm->max_tbs_bytes > 512)
    throw Error(NZCB_ERR_ARG, "nzcp: MaxToBeSignedBytes must be in [1, 512] (Sha256Var(3) holds 4096 bits)");
  return (uint32_t)prm->max_tbs_bytes;
}

void check_offsets(const uint32_t* offsets, size_t count) {
  for (size_t i = 0; i < count; i++)
    if (offsets[i + 1] < offsets[i]) throw Error(NZCB_ERR_ARG, "nzcp decode: the offsets decrease");
  if (offsets[count] > 0x80000000u) throw Error(NZCB_ERR_ARG, "nzcp decode: more than 2^31 bytes of URIs");
}

void launch(const uint8_t* d_uris, const uint32_t* d_offsets, int count, uint32_t max_tbs, const uint8_t* d_data20,
            nzcb_nzcp_pass* d_passes, uint8_t* d_inputs, uint8_t* d_tbs, size_t tbs_stride, hipStream_t st) {
  k_nzcp_decode<<<dim3((unsigned)count), dim3(kLanes), 0, st>>>(d_uris, d_offsets, max_tbs, d_data20, d_passes,
                                                                  d_inputs, d_tbs, tbs_stride);
  NZ_HIP(hipGetLastError());
}

void decode_dev(int device, const void* d_uris, const void* d_offsets, int count, const nzcb_nzcp_params* prm,
                const void* d_data20, void* d_passes, void* d_inputs, void* d_tbs, size_t tbs_stride, void* stream) {
  const uint32_t max_tbs = max_tbs_of(prm);
  if (count < 0) throw Error(NZCB_ERR_ARG, "nzcp decode: bad count");
  if (d_inputs && !max_tbs) throw Error(NZCB_ERR_ARG, "nzcp decode: inputs need the circuit's parameters");
  if (!count) return;
  if (!d_offsets || !d_passes) throw Error(NZCB_ERR_ARG, "nzcp decode: null argument");
  if ((reinterpret_cast<uintptr_t>(d_passes) & 7) || (reinterpret_cast<uintptr_t>(d_inputs) & 15) ||
      (reinterpret_cast<uintptr_t>(d_offsets) & 3))
    throw Error(NZCB_ERR_ARG, "nzcp decode: device records must be multiples of 8, inputs of 16, offsets of 4");
  DeviceScope scope(device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  std::vector<uint32_t> offsets((size_t)count + 1);
  NZ_HIP(hipMemcpyAsync(offsets.data(), d_offsets, offsets.size() * 4, hipMemcpyDeviceToHost, st));
  NZ_HIP(hipStreamSynchronize(st));
  check_offsets(offsets.data(), (size_t)count);
  if (offsets[count] && !d_uris) throw Error(NZCB_ERR_ARG, "nzcp decode: null argument");
  launch(static_cast<const uint8_t*>(d_uris), static_cast<const uint32_t*>(d_offsets), count, max_tbs,
         static_cast<const uint8_t*>(d_data20), static_cast<nzcb_nzcp_pass*>(d_passes),
         static_cast<uint8_t*>(d_inputs), static_cast<uint8_t*>(d_tbs), tbs_stride, st);
}

void decode(int device, const uint8_t* uris, const uint32_t* offsets, int count, const nzcb_nzcp_params* prm,
            const uint8_t* data20, nzcb_nzcp_pass* passes, uint8_t* inputs, uint8_t* tbs_out, size_t tbs_stride) {
  const uint32_t max_tbs = max_tbs_of(prm);
  g_times[0] = g_times[1] = 0;
  if (count < 0) throw Error(NZCB_ERR_ARG, "nzcp decode: bad count");
  if (inputs && !max_tbs) throw Error(NZCB_ERR_ARG, "nzcp decode: inputs need the circuit's parameters");
  if (!count) return;
  if (!offsets || !passes) throw Error(NZCB_ERR_ARG, "nzcp decode: null argument");
  const size_t n = (size_t)count;
  check_offsets(offsets, n);
  const size_t total = offsets[n];
  if (total && !uris) throw Error(NZCB_ERR_ARG, "nzcp decode: null argument");
  const size_t in_bytes = inputs ? (size_t)input_signals(max_tbs) * 32 : 0;
  const auto t0 = std::chrono::steady_clock::now();
  auto wall = [&] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
  if (device == NZCB_NZCP_HOST) {
    std::vector<uint8_t> cose(kMaxCose), tbs(kMaxTbs);
    for (size_t i = 0; i < n; i++)
      decode_one(uris + offsets[i], (uint64_t)(offsets[i + 1] - offsets[i]), max_tbs,
                 data20 ? data20 + kDataBytes * i : nullptr, cose.data(), tbs.data(), passes + i,
                 inputs ? inputs + in_bytes * i : nullptr, tbs_out ? tbs_out + tbs_stride * i : nullptr, tbs_stride);
    g_times[1] = wall();
    return;
  }
  CallScope cs(device, nullptr, 2);
  // the kernel takes a NULL data20, inputs or tbs_out as "not asked for"
  uint8_t* d_uris = total ? cs.alloc<uint8_t>(total) : nullptr;
  uint8_t* d_data = data20 ? cs.alloc<uint8_t>(kDataBytes * n) : nullptr;
  uint8_t* d_inputs = inputs ? cs.alloc<uint8_t>(in_bytes * n) : nullptr;
  uint8_t* d_tbs = tbs_out && tbs_stride ? cs.alloc<uint8_t>(tbs_stride * n) : nullptr;
  uint32_t* d_off = cs.alloc<uint32_t>(4 * (n + 1));
  nzcb_nzcp_pass* d_pass = cs.alloc<nzcb_nzcp_pass>(sizeof(nzcb_nzcp_pass) * n);
  if (total) NZ_HIP(hipMemcpyAsync(d_uris, uris, total, hipMemcpyHostToDevice, cs.st));
  NZ_HIP(hipMemcpyAsync(d_off, offsets, 4 * (n + 1), hipMemcpyHostToDevice, cs.st));
  if (data20) NZ_HIP(hipMemcpyAsync(d_data, data20, kDataBytes * n, hipMemcpyHostToDevice, cs.st));
  cs.record(0);
  launch(d_uris, d_off, count, max_tbs, d_data, d_pass, d_inputs, d_tbs, tbs_stride, cs.st);
  cs.record(1);
  NZ_HIP(hipMemcpyAsync(passes, d_pass, sizeof(nzcb_nzcp_pass) * n, hipMemcpyDeviceToHost, cs.st));
  if (inputs) NZ_HIP(hipMemcpyAsync(inputs, d_inputs, in_bytes * n, hipMemcpyDeviceToHost, cs.st));
  if (d_tbs) NZ_HIP(hipMemcpyAsync(tbs_out, d_tbs, tbs_stride * n, hipMemcpyDeviceToHost, cs.st));
  NZ_HIP(hipStreamSynchronize(cs.st));
  g_times[0] = cs.elapsed(0, 1);
  g_times[1] = wall();
}

}  // namespace
}  // namespace nzdec
}  // namespace nzcb

using namespace nzcb;

extern "C" {

void nzcb_nzcp_pass_layout(uint32_t out[3]) {
  out[0] = (uint32_t)sizeof(nzcb_nzcp_pass);
  out[1] = (uint32_t)offsetof(nzcb_nzcp_pass, sig);
  out[2] = (uint32_t)offsetof(nzcb_nzcp_pass, tbs_sha256);
}

int nzcb_nzcp_decode(int device, const uint8_t* uris, const uint32_t* offsets, int count, const nzcb_nzcp_params* prm,
                     const uint8_t* data20, nzcb_nzcp_pass* passes_out, uint8_t* inputs_out, uint8_t* tbs_out,
                     size_t tbs_stride, nzcb_err* err) {
  return guarded(err, [&] {
    nzdec::decode(device, uris, offsets, count, prm, data20, passes_out, inputs_out, tbs_out, tbs_stride);
  });
}

int nzcb_nzcp_decode_dev(int device, const void* dev_uris, const void* dev_offsets, int count,
                         const nzcb_nzcp_params* prm, const void* dev_data20, void* dev_passes, void* dev_inputs,
                         void* dev_tbs, size_t tbs_stride, void* stream, nzcb_err* err) {
  return guarded(err, [&] {
    nzdec::decode_dev(device, dev_uris, dev_offsets, count, prm, dev_data20, dev_passes, dev_inputs, dev_tbs,
                      tbs_stride, stream);
  });
}

int nzcb_debug_nzcp_decode_timings(double* ms, int cap) {
  int k = 0;
  for (; ms && k < cap && k < 2; k++) ms[k] = nzdec::g_times[k];
  return k;
}

}  // extern "C"
