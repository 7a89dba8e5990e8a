// Device plumbing of the self-contained entry points (batch verification, the r1cs check, the
// P-256 signatures, the pass decode): which device the calling thread is on during a call, what a
// call owns on it, and what an object keeps on it between calls.
//
// These entry points leave the calling thread on the device it came from. The older ones do not,
// on purpose: capi_engine.hip, synth.hip, nzcp.hip, wvm.hip and Prover set the device and stay on
// it, and callers may rely on that. Do not convert them to DeviceScope in passing.
#pragma once
#include <vector>

#include "common.h"

namespace nzcb {

// the calling thread's device for the duration of a call
struct DeviceScope {
  int prev = -1;
  explicit DeviceScope(int device) {
    int ndev = 0;
    NZ_HIP(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) throw Error(NZCB_ERR_ARG, "no such device");
    NZ_HIP(hipGetDevice(&prev));
    NZ_HIP(hipSetDevice(device));
  }
  ~DeviceScope() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
  DeviceScope(const DeviceScope&) = delete;
  DeviceScope& operator=(const DeviceScope&) = delete;
};

// What one call owns on its device: the stream (its own unless the caller gave one), events and
// temporary buffers. The DeviceScope is the first member, so everything is released on the
// call's device before the thread returns to its own.
struct CallScope {
  DeviceScope dev;
  hipStream_t st;
  bool own = false;
  std::vector<hipEvent_t> ev;
  std::vector<DevBuf<uint8_t>> bufs;

  CallScope(int device, void* stream, int n_events) : dev(device), st(static_cast<hipStream_t>(stream)) {
    try {
      if (!st) {
        NZ_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        own = true;
      }
      ev.resize((size_t)n_events, nullptr);
      for (auto& e : ev) NZ_HIP(hipEventCreate(&e));
    } catch (...) {
      release();
      throw;
    }
  }
  ~CallScope() { release(); }
  CallScope(const CallScope&) = delete;
  CallScope& operator=(const CallScope&) = delete;

  // one hipMalloc, freed with the call; never NULL
  template <class T>
  T* alloc(size_t bytes) {
    bufs.emplace_back(bytes ? bytes : 4);
    return reinterpret_cast<T*>(bufs.back().p);
  }
  void record(int i) { NZ_HIP(hipEventRecord(ev[(size_t)i], st)); }
  // milliseconds between two recorded events, once the stream has passed both
  float elapsed(int i, int j) {
    float ms = 0;
    NZ_HIP(hipEventElapsedTime(&ms, ev[(size_t)i], ev[(size_t)j]));
    return ms;
  }

 private:
  void release() {
    if (st) (void)hipStreamSynchronize(st);
    bufs.clear();
    for (auto& e : ev)
      if (e) (void)hipEventDestroy(e);
    ev.clear();
    if (own && st) (void)hipStreamDestroy(st);
    st = nullptr;
  }
};

// 256-byte-aligned offsets of several arrays laid into one allocation of `total` bytes
struct BlockLayout {
  size_t total = 0;
  size_t take(size_t bytes) {
    const size_t at = total;
    total += (bytes + 255) & ~size_t(255);
    return at;
  }
};

// One allocation that an object keeps between calls. It remembers its device and is freed under
// it, from whichever device the destroying thread is on.
struct DeviceBlock {
  char* p = nullptr;  // NULL: a host object
  int device = -1;
  DeviceBlock() = default;
  DeviceBlock(const DeviceBlock&) = delete;
  DeviceBlock& operator=(const DeviceBlock&) = delete;
  // on the calling thread's current device (inside a DeviceScope or CallScope)
  void alloc(size_t bytes) {
    NZ_HIP(hipGetDevice(&device));
    NZ_HIP(hipMalloc(&p, bytes));
  }
  template <class T>
  T* at(size_t offset) const {
    return reinterpret_cast<T*>(p + offset);
  }
  ~DeviceBlock() {
    int prev = 0;
    if (p && hipGetDevice(&prev) == hipSuccess && hipSetDevice(device) == hipSuccess) {
      (void)hipFree(p);
      (void)hipSetDevice(prev);
    }
  }
};

}  // namespace nzcb
