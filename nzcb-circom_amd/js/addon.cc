// N-API addon: the Node.js side of the drop-in boundary.
//
// The reference's host is Node.js: its proofs come from snarkjs.plonk.prove /
// plonk.fullProve [EXT] (snarkjs 0.4.12, /root/reference/package.json:18). This
// addon binds the C-ABI in include/nzcb.h one-to-one; index.js wraps it in the
// snarkjs-compatible Promise API. Every prove / fullProveDevice call runs on a thread of
// its own and takes a free lane of the context (nzcb_prove_logged), so concurrent promises
// on one context are proved at the same time, up to the context's lanes (setLanes); the
// result and the optional logger come back to the main thread through thread-safe
// functions, and the event loop is never blocked.
#define NAPI_VERSION 6
#include <node_api.h>

#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/nzcb.h"

#define CHECK(call)                                                    \
  do {                                                                 \
    if ((call) != napi_ok) {                                           \
      napi_throw_error(env, nullptr, "nzcb addon: N-API call failed"); \
      return nullptr;                                                  \
    }                                                                  \
  } while (0)

namespace {

struct Ctx {
  nzcb_ctx* ctx = nullptr;
};

void ctx_finalize(napi_env, void* data, void*) {
  Ctx* c = static_cast<Ctx*>(data);
  if (c->ctx) nzcb_ctx_destroy(c->ctx);
  delete c;
}

napi_value make_error(napi_env env, int code, const char* msg) {
  napi_value m, err, c;
  napi_create_string_utf8(env, msg, NAPI_AUTO_LENGTH, &m);
  napi_create_error(env, nullptr, m, &err);
  napi_create_int32(env, code, &c);
  napi_set_named_property(env, err, "code", c);
  return err;
}

// createContext(zkey: Buffer, device: number) -> external
napi_value CreateContext(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  CHECK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  void* data = nullptr;
  size_t len = 0;
  CHECK(napi_get_buffer_info(env, argv[0], &data, &len));
  int32_t device = 0;
  if (argc > 1) napi_get_value_int32(env, argv[1], &device);
  nzcb_err err{};
  nzcb_ctx* ctx = nzcb_ctx_create(static_cast<const uint8_t*>(data), len, device, &err);
  if (!ctx) {
    napi_throw(env, make_error(env, err.code, err.msg));
    return nullptr;
  }
  Ctx* c = new Ctx();
  c->ctx = ctx;
  napi_value ext;
  CHECK(napi_create_external(env, c, ctx_finalize, nullptr, &ext));
  return ext;
}

// releaseContext(ctx): frees the context's HBM now instead of at garbage collection (a
// context whose lane setup failed is dropped this way; the external must not be used after)
napi_value ReleaseContext(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  CHECK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  Ctx* c = nullptr;
  CHECK(napi_get_value_external(env, argv[0], reinterpret_cast<void**>(&c)));
  if (c && c->ctx) {
    nzcb_ctx_destroy(c->ctx);
    c->ctx = nullptr;
  }
  return nullptr;
}

// a JS string argument as UTF-8 (false if it is not a string)
bool str_arg(napi_env env, napi_value v, std::string* out) {
  napi_valuetype t;
  if (napi_typeof(env, v, &t) != napi_ok || t != napi_string) return false;
  size_t plen = 0;
  if (napi_get_value_string_utf8(env, v, nullptr, 0, &plen) != napi_ok) return false;
  out->assign(plen + 1, '\0');
  if (napi_get_value_string_utf8(env, v, &(*out)[0], out->size(), &plen) != napi_ok) return false;
  out->resize(plen);
  return true;
}

// createContextFile(path: string, device: number) -> external (zkeys larger than a Buffer)
napi_value CreateContextFile(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  CHECK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  std::string path;
  if (argc < 1 || !str_arg(env, argv[0], &path)) {
    napi_throw_type_error(env, nullptr, "createContextFile(path: string, device?: number)");
    return nullptr;
  }
  int32_t device = 0;
  if (argc > 1) napi_get_value_int32(env, argv[1], &device);
  nzcb_err err{};
  const int devs[1] = {device};
  nzcb_ctx* ctx = nzcb_ctx_create_file(path.c_str(), devs, 1, &err);
  if (!ctx) {
    napi_throw(env, make_error(env, err.code, err.msg));
    return nullptr;
  }
  Ctx* c = new Ctx();
  c->ctx = ctx;
  napi_value ext;
  CHECK(napi_create_external(env, c, ctx_finalize, nullptr, &ext));
  return ext;
}

struct Wprog;

// one prove / fullProveDevice call: runs on its own thread, completes on the main thread
struct ProveWork {
  napi_deferred deferred = nullptr;
  napi_ref ctx_ref = nullptr, in_ref = nullptr, prog_ref = nullptr;
  napi_threadsafe_function done = nullptr;  // completion (no JS function: prove_complete)
  napi_threadsafe_function tsfn = nullptr;  // the logger, if any
  Ctx* c = nullptr;
  Wprog* prog = nullptr;                    // fullProveDevice: the witness program
  const uint8_t* in = nullptr;              // .wtns bytes (prove) or input signals (fullProveDevice)
  size_t in_len = 0;
  bool has_blinding = false;
  uint8_t blinding[NZCB_BLINDING_BYTES];
  uint8_t proof[NZCB_PROOF_BYTES];
  uint8_t pub[32 * 64];
  uint32_t npub = 0;
  int rc = 0;
  int32_t status = 0;  // fullProveDevice: the witness program's failed check, if any
  nzcb_err err{};
};

void log_trampoline(void* user, const char* msg) {
  ProveWork* w = static_cast<ProveWork*>(user);
  if (!w->tsfn) return;
  char* copy = strdup(msg);
  if (napi_call_threadsafe_function(w->tsfn, copy, napi_tsfn_blocking) != napi_ok) free(copy);
}

void call_logger(napi_env env, napi_value fn, void*, void* data) {
  char* msg = static_cast<char*>(data);
  if (env && fn) {
    napi_value s, undef;
    napi_create_string_utf8(env, msg, NAPI_AUTO_LENGTH, &s);
    napi_get_undefined(env, &undef);
    napi_call_function(env, undef, fn, 1, &s, nullptr);
  }
  free(msg);
}

void prove_complete(napi_env env, napi_value, void*, void* data) {
  ProveWork* w = static_cast<ProveWork*>(data);
  if (env) {
    if (w->rc) {
      napi_reject_deferred(env, w->deferred, make_error(env, w->rc, w->err.msg));
    } else if (w->status) {
      napi_reject_deferred(env, w->deferred, make_error(env, w->status, "Assert Failed (witness calculation)"));
    } else {
      std::string pj(8192, '\0'), uj(96 * 64 + 8, '\0');
      nzcb_proof_to_json(w->proof, &pj[0], pj.size());
      nzcb_public_to_json(w->pub, (int)w->npub, &uj[0], uj.size());
      napi_value obj, a, b;
      napi_create_object(env, &obj);
      napi_create_string_utf8(env, pj.c_str(), NAPI_AUTO_LENGTH, &a);
      napi_create_string_utf8(env, uj.c_str(), NAPI_AUTO_LENGTH, &b);
      napi_set_named_property(env, obj, "proof", a);
      napi_set_named_property(env, obj, "publicSignals", b);
      napi_resolve_deferred(env, w->deferred, obj);
    }
    napi_delete_reference(env, w->ctx_ref);
    napi_delete_reference(env, w->in_ref);
    if (w->prog_ref) napi_delete_reference(env, w->prog_ref);
  }
  if (w->tsfn) napi_release_threadsafe_function(w->tsfn, napi_tsfn_release);
  napi_release_threadsafe_function(w->done, napi_tsfn_release);
  delete w;
}

void run_fullprove_device(ProveWork* w);

void prove_thread(ProveWork* w) {
  uint32_t info[5];
  nzcb_ctx_info(w->c->ctx, info);
  w->npub = info[1];
  if (w->npub > 64) {
    w->rc = NZCB_ERR_ARG;
    std::snprintf(w->err.msg, sizeof(w->err.msg), "too many public signals for the addon buffer");
  } else if (w->prog) {
    run_fullprove_device(w);
  } else {
    w->rc = nzcb_prove_logged(w->c->ctx, w->in, w->in_len, NZCB_WITNESS_WTNS, w->has_blinding ? w->blinding : nullptr,
                              w->proof, w->pub, sizeof(w->pub), w->tsfn ? log_trampoline : nullptr, w, &w->err);
  }
  napi_call_threadsafe_function(w->done, w, napi_tsfn_blocking);
}

// the common argument handling of prove / fullProveDevice: blinding (argv[bi]), logger
// (argv[bi + 1]); creates the promise and starts the thread
napi_value start_prove(napi_env env, ProveWork* w, napi_value* argv, size_t argc, size_t bi) {
  napi_valuetype t;
  if (argc > bi && napi_typeof(env, argv[bi], &t) == napi_ok && t == napi_object) {
    void* bd = nullptr;
    size_t bl = 0;
    if (napi_get_buffer_info(env, argv[bi], &bd, &bl) == napi_ok && bl == NZCB_BLINDING_BYTES) {
      std::memcpy(w->blinding, bd, bl);
      w->has_blinding = true;
    }
  }
  napi_value name;
  if (argc > bi + 1 && napi_typeof(env, argv[bi + 1], &t) == napi_ok && t == napi_function) {
    napi_create_string_utf8(env, "nzcb-logger", NAPI_AUTO_LENGTH, &name);
    CHECK(napi_create_threadsafe_function(env, argv[bi + 1], nullptr, name, 0, 1, nullptr, nullptr, nullptr,
                                          call_logger, &w->tsfn));
  }
  napi_value promise;
  CHECK(napi_create_promise(env, &w->deferred, &promise));
  napi_create_string_utf8(env, "nzcb-prove", NAPI_AUTO_LENGTH, &name);
  CHECK(napi_create_threadsafe_function(env, nullptr, nullptr, name, 0, 1, nullptr, nullptr, nullptr, prove_complete,
                                        &w->done));
  std::thread(prove_thread, w).detach();
  return promise;
}

// prove(ctx, wtns: Buffer, blinding: Buffer|null, logger: Function|null) -> Promise<{proof, publicSignals}> (JSON strings)
napi_value Prove(napi_env env, napi_callback_info info) {
  size_t argc = 4;
  napi_value argv[4];
  CHECK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  ProveWork* w = new ProveWork();
  CHECK(napi_get_value_external(env, argv[0], reinterpret_cast<void**>(&w->c)));
  void* wd = nullptr;
  CHECK(napi_get_buffer_info(env, argv[1], &wd, &w->in_len));
  w->in = static_cast<const uint8_t*>(wd);
  CHECK(napi_create_reference(env, argv[0], 1, &w->ctx_ref));
  CHECK(napi_create_reference(env, argv[1], 1, &w->in_ref));
  return start_prove(env, w, argv, argc, 2);
}

// setLanes(ctx, lanes) -> lanes: proofs in flight on the context (nzcb_ctx_set_lanes)
napi_value SetLanes(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  CHECK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  Ctx* c = nullptr;
  CHECK(napi_get_value_external(env, argv[0], reinterpret_cast<void**>(&c)));
  int32_t lanes = 1;
  CHECK(napi_get_value_int32(env, argv[1], &lanes));
  nzcb_err err{};
  if (nzcb_ctx_set_lanes(c->ctx, lanes, &err)) {
    napi_throw(env, make_error(env, err.code, err.msg));
    return nullptr;
  }
  napi_value v;
  napi_create_int32(env, nzcb_ctx_lanes(c->ctx), &v);
  return v;
}

// ---- witness programs (nzcb_wprog_*): circom's witness calculator on the GPU ----------
struct Wprog {
  nzcb_wprog* p = nullptr;
  int device = 0;  // the program's GPU: its witness buffers live there
};

// HBM buffers reused across fullProveDevice calls (a witness of nzcp_live is 19.2 MB; a
// hipMalloc per proof would cost more than the witness program's run), keyed by (device,
// bytes): a call's buffers are on its witness program's device (the per-call
// threads never selected a device, so every buffer was on device 0)
std::mutex g_pool_mu;
std::multimap<std::pair<int, size_t>, void*> g_pool;
void* pool_get(int device, size_t bytes) {
  {
    std::lock_guard<std::mutex> lk(g_pool_mu);
    auto it = g_pool.find({device, bytes});
    if (it != g_pool.end()) {
      void* p = it->second;
      g_pool.erase(it);
      return p;
    }
  }
  return nzcb_dev_alloc_on(device, bytes);
}
void pool_put(int device, size_t bytes, void* p) {
  if (!p) return;
  std::lock_guard<std::mutex> lk(g_pool_mu);
  g_pool.emplace(std::make_pair(device, bytes), p);
}

// plonk.fullProve with a witness program, everything in HBM: the input signals go up
// (a few KB), the witness program writes the witness into a device buffer, and the proof
// reads it there (nzcb_wprog_run_dev + nzcb_prove_logged NZCB_WITNESS_DEVICE); only the
// proof and the public signals come back
void run_fullprove_device(ProveWork* w) {
  uint32_t pi[5];
  nzcb_wprog_info(w->prog->p, pi);
  const size_t nwires = pi[0], nin = (size_t)pi[2] + pi[3];
  if (w->in_len != nin * 32) {
    w->rc = NZCB_ERR_ARG;
    std::snprintf(w->err.msg, sizeof(w->err.msg), "expected %zu input signals", nin);
    return;
  }
  const int dev = w->prog->device;
  void* din = pool_get(dev, nin * 32 ? nin * 32 : 32);
  void* dw = pool_get(dev, nwires * 32);
  if (!din || !dw || nzcb_memcpy_h2d(din, w->in, w->in_len) != 0) {
    w->rc = NZCB_ERR_HIP;
    std::snprintf(w->err.msg, sizeof(w->err.msg), "device buffers for the witness failed");
  } else {
    w->rc = nzcb_wprog_run_dev(w->prog->p, din, 1, dw, nwires * 32, &w->status, nullptr, &w->err);
    if (!w->rc && !w->status)
      w->rc = nzcb_prove_logged(w->c->ctx, dw, nwires, NZCB_WITNESS_DEVICE, w->has_blinding ? w->blinding : nullptr,
                                w->proof, w->pub, sizeof(w->pub), w->tsfn ? log_trampoline : nullptr, w, &w->err);
  }
  pool_put(dev, nin * 32 ? nin * 32 : 32, din);
  pool_put(dev, nwires * 32, dw);
}

void wprog_finalize(napi_env, void* data, void*) {
  Wprog* w = static_cast<Wprog*>(data);
  if (w->p) nzcb_wprog_destroy(w->p);
  delete w;
}

// createWitnessProgram(program: Buffer, device: number) -> external
napi_value CreateWitnessProgram(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  CHECK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  void* data = nullptr;
  size_t len = 0;
  CHECK(napi_get_buffer_info(env, argv[0], &data, &len));
  int32_t device = 0;
  if (argc > 1) napi_get_value_int32(env, argv[1], &device);
  nzcb_err err{};
  nzcb_wprog* p = nzcb_wprog_create(static_cast<const uint8_t*>(data), len, device, &err);
  if (!p) {
    napi_throw(env, make_error(env, err.code, err.msg));
    return nullptr;
  }
  Wprog* w = new Wprog();
  w->p = p;
  w->device = device;
  napi_value ext;
  CHECK(napi_create_external(env, w, wprog_finalize, nullptr, &ext));
  return ext;
}

struct WitnessWork {
  napi_async_work work = nullptr;
  napi_deferred deferred = nullptr;
  napi_ref prog_ref = nullptr, in_ref = nullptr;
  Wprog* w = nullptr;
  const uint8_t* inputs = nullptr;
  size_t in_len = 0;
  std::vector<uint8_t> out;
  int32_t status = 0;
  int rc = 0;
  nzcb_err err{};
};

void witness_execute(napi_env, void* data) {
  WitnessWork* k = static_cast<WitnessWork*>(data);
  uint32_t info[5];
  nzcb_wprog_info(k->w->p, info);
  const size_t nin = (size_t)info[2] + info[3];
  if (k->in_len != nin * 32) {
    k->rc = NZCB_ERR_ARG;
    std::snprintf(k->err.msg, sizeof(k->err.msg), "expected %zu input signals", nin);
    return;
  }
  k->out.resize((size_t)info[0] * 32);
  k->rc = nzcb_wprog_run(k->w->p, k->inputs, 1, k->out.data(), &k->status, &k->err);
}

void witness_complete(napi_env env, napi_status, void* data) {
  WitnessWork* k = static_cast<WitnessWork*>(data);
  if (k->rc) {
    napi_reject_deferred(env, k->deferred, make_error(env, k->rc, k->err.msg));
  } else if (k->status) {
    napi_reject_deferred(env, k->deferred, make_error(env, k->status, "Assert Failed (witness calculation)"));
  } else {
    napi_value buf;
    void* dst = nullptr;
    if (napi_create_buffer_copy(env, k->out.size(), k->out.data(), &dst, &buf) == napi_ok)
      napi_resolve_deferred(env, k->deferred, buf);
    else
      napi_reject_deferred(env, k->deferred, make_error(env, NZCB_ERR_INTERNAL, "buffer allocation failed"));
  }
  napi_delete_reference(env, k->prog_ref);
  napi_delete_reference(env, k->in_ref);
  napi_delete_async_work(env, k->work);
  delete k;
}

// calculateWitness(prog, inputs: Buffer (n_inputs x 32 B LE)) -> Promise<Buffer (n_wires x 32 B LE)>
napi_value CalculateWitness(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  CHECK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  WitnessWork* k = new WitnessWork();
  CHECK(napi_get_value_external(env, argv[0], reinterpret_cast<void**>(&k->w)));
  void* d = nullptr;
  CHECK(napi_get_buffer_info(env, argv[1], &d, &k->in_len));
  k->inputs = static_cast<const uint8_t*>(d);
  CHECK(napi_create_reference(env, argv[0], 1, &k->prog_ref));
  CHECK(napi_create_reference(env, argv[1], 1, &k->in_ref));
  napi_value promise, rname;
  CHECK(napi_create_promise(env, &k->deferred, &promise));
  napi_create_string_utf8(env, "nzcb-witness", NAPI_AUTO_LENGTH, &rname);
  CHECK(napi_create_async_work(env, nullptr, rname, witness_execute, witness_complete, k, &k->work));
  CHECK(napi_queue_async_work(env, k->work));
  return promise;
}

// fullProveDevice(ctx, prog, inputs: Buffer (n_inputs x 32 B LE), blinding, logger)
//   -> Promise<{proof, publicSignals}>
napi_value FullProveDevice(napi_env env, napi_callback_info info) {
  size_t argc = 5;
  napi_value argv[5];
  CHECK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  ProveWork* w = new ProveWork();
  CHECK(napi_get_value_external(env, argv[0], reinterpret_cast<void**>(&w->c)));
  CHECK(napi_get_value_external(env, argv[1], reinterpret_cast<void**>(&w->prog)));
  void* d = nullptr;
  CHECK(napi_get_buffer_info(env, argv[2], &d, &w->in_len));
  w->in = static_cast<const uint8_t*>(d);
  CHECK(napi_create_reference(env, argv[0], 1, &w->ctx_ref));
  CHECK(napi_create_reference(env, argv[1], 1, &w->prog_ref));
  CHECK(napi_create_reference(env, argv[2], 1, &w->in_ref));
  return start_prove(env, w, argv, argc, 3);
}

napi_value Info(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  CHECK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  Ctx* c = nullptr;
  CHECK(napi_get_value_external(env, argv[0], reinterpret_cast<void**>(&c)));
  uint32_t v[5];
  nzcb_ctx_info(c->ctx, v);
  napi_value obj;
  napi_create_object(env, &obj);
  const char* names[5] = {"domainSize", "nPublic", "nVars", "nAdditions", "nConstraints"};
  for (int i = 0; i < 5; i++) {
    napi_value x;
    napi_create_uint32(env, v[i], &x);
    napi_set_named_property(env, obj, names[i], x);
  }
  return obj;
}

napi_value Version(napi_env env, napi_callback_info) {
  napi_value s;
  napi_create_string_utf8(env, nzcb_version(), NAPI_AUTO_LENGTH, &s);
  return s;
}

napi_value DeviceCount(napi_env env, napi_callback_info) {
  napi_value s;
  napi_create_int32(env, nzcb_device_count(), &s);
  return s;
}

// buffer argument i -> (data, len); false if not a Buffer
bool buf_arg(napi_env env, napi_value v, const uint8_t** data, size_t* len) {
  void* d = nullptr;
  if (napi_get_buffer_info(env, v, &d, len) != napi_ok) return false;
  *data = static_cast<const uint8_t*>(d);
  return true;
}

napi_value json_string(napi_env env, const std::string& s) {
  napi_value v;
  napi_create_string_utf8(env, s.c_str(), s.size(), &v);
  return v;
}

// vkFromZkey(zkey: Buffer) -> Buffer (NZCB_VK_BYTES); snarkjs `zkey export verificationkey`
napi_value VkFromZkey(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  CHECK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  const uint8_t* z;
  size_t zl;
  if (argc < 1 || !buf_arg(env, argv[0], &z, &zl)) {
    napi_throw_type_error(env, nullptr, "vkFromZkey(zkey: Buffer)");
    return nullptr;
  }
  void* out = nullptr;
  napi_value res;
  CHECK(napi_create_buffer(env, NZCB_VK_BYTES, &out, &res));
  nzcb_err err{};
  if (nzcb_vk_from_zkey(z, zl, static_cast<uint8_t*>(out), &err) != 0) {
    napi_throw(env, make_error(env, err.code, err.msg));
    return nullptr;
  }
  return res;
}

// vkFromZkeyFile(path: string) -> Buffer (NZCB_VK_BYTES): the zkey is memory-mapped by the
// library, so files past a Buffer's 2 GiB limit (nzcp_live_final.zkey) work
napi_value VkFromZkeyFile(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  CHECK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  std::string path;
  if (argc < 1 || !str_arg(env, argv[0], &path)) {
    napi_throw_type_error(env, nullptr, "vkFromZkeyFile(path: string)");
    return nullptr;
  }
  void* out = nullptr;
  napi_value res;
  CHECK(napi_create_buffer(env, NZCB_VK_BYTES, &out, &res));
  nzcb_err err{};
  if (nzcb_vk_from_zkey_file(path.c_str(), static_cast<uint8_t*>(out), &err) != 0) {
    napi_throw(env, make_error(env, err.code, err.msg));
    return nullptr;
  }
  return res;
}

// remapWitnessProgram(program: Buffer, ownSym: Buffer, targetSym: Buffer) -> Buffer
// (nzcb_wprog_remap); throws with .unmatched when target signals have no counterpart
napi_value RemapWitnessProgram(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value argv[3];
  CHECK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  const uint8_t *prog, *own, *tgt;
  size_t pl, ol, tl;
  if (argc < 3 || !buf_arg(env, argv[0], &prog, &pl) || !buf_arg(env, argv[1], &own, &ol) ||
      !buf_arg(env, argv[2], &tgt, &tl)) {
    napi_throw_type_error(env, nullptr, "remapWitnessProgram(program: Buffer, ownSym: Buffer, targetSym: Buffer)");
    return nullptr;
  }
  uint8_t* out = nullptr;
  size_t out_len = 0;
  uint32_t miss = 0;
  nzcb_err err{};
  if (nzcb_wprog_remap(prog, pl, reinterpret_cast<const char*>(own), ol, reinterpret_cast<const char*>(tgt), tl, &out,
                       &out_len, &miss, &err) != 0) {
    napi_value e = make_error(env, err.code, err.msg);
    napi_value m;
    napi_create_uint32(env, miss, &m);
    napi_set_named_property(env, e, "unmatched", m);
    napi_throw(env, e);
    return nullptr;
  }
  void* dst = nullptr;
  napi_value res;
  const napi_status stc = napi_create_buffer_copy(env, out_len, out, &dst, &res);
  nzcb_free(out);
  CHECK(stc);
  return res;
}

// vkToJson(vk: Buffer) -> string (verification_key.json)
napi_value VkToJson(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  CHECK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  const uint8_t* vk;
  size_t vl;
  if (argc < 1 || !buf_arg(env, argv[0], &vk, &vl) || vl != NZCB_VK_BYTES) {
    napi_throw_type_error(env, nullptr, "vkToJson(vk: Buffer)");
    return nullptr;
  }
  std::string s((size_t)nzcb_vk_to_json(vk, nullptr, 0), '\0');
  nzcb_vk_to_json(vk, &s[0], s.size());
  s.resize(std::strlen(s.c_str()));
  return json_string(env, s);
}

// verify(vk: Buffer, proof: Buffer, pub: Buffer, transcriptPublic: bool) -> bool (snarkjs plonk.verify)
napi_value Verify(napi_env env, napi_callback_info info) {
  size_t argc = 4;
  napi_value argv[4];
  CHECK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  const uint8_t *vk, *proof, *pub;
  size_t vl, pl, ul;
  if (argc < 3 || !buf_arg(env, argv[0], &vk, &vl) || !buf_arg(env, argv[1], &proof, &pl) ||
      !buf_arg(env, argv[2], &pub, &ul) || vl != NZCB_VK_BYTES || pl != NZCB_PROOF_BYTES || ul % 32) {
    napi_throw_type_error(env, nullptr, "verify(vk: Buffer, proof: Buffer, pub: Buffer, transcriptPublic)");
    return nullptr;
  }
  bool tp = true;
  if (argc > 3) napi_get_value_bool(env, argv[3], &tp);
  int valid = 0;
  nzcb_err err{};
  if (nzcb_verify(vk, proof, pub, (int)(ul / 32), tp ? 1 : 0, &valid, &err) != 0) {
    napi_throw(env, make_error(env, err.code, err.msg));
    return nullptr;
  }
  napi_value r;
  napi_get_boolean(env, valid != 0, &r);
  return r;
}

// one verifyBatch call: nzcb_verify_batch on a worker thread (async work), the promise
// settled on the main thread; the inputs are copied, so the caller's Buffers may change
struct VerifyBatchWork {
  napi_deferred deferred = nullptr;
  napi_async_work work = nullptr;
  std::vector<uint8_t> vk, proofs, pubs;
  int n_public = 0, count = 0, device = 0;
  bool tp = true;
  std::vector<int> valid;
  int rc = 0;
  nzcb_err err{};
};

void verify_batch_execute(napi_env, void* data) {
  VerifyBatchWork* w = static_cast<VerifyBatchWork*>(data);
  w->rc = nzcb_verify_batch(w->vk.data(), w->proofs.data(), w->pubs.data(), 32 * (size_t)w->n_public, w->n_public,
                            w->count, w->tp ? 1 : 0, w->device, nullptr, w->valid.data(), &w->err);
}

void verify_batch_complete(napi_env env, napi_status status, void* data) {
  VerifyBatchWork* w = static_cast<VerifyBatchWork*>(data);
  if (status != napi_ok || w->rc != 0) {
    napi_reject_deferred(env, w->deferred,
                         make_error(env, w->rc ? w->err.code : NZCB_ERR_INTERNAL,
                                    w->rc ? w->err.msg : "verifyBatch: the work was cancelled"));
  } else {
    napi_value arr;
    napi_create_array_with_length(env, (size_t)w->count, &arr);
    for (int i = 0; i < w->count; i++) {
      napi_value b;
      napi_get_boolean(env, w->valid[i] != 0, &b);
      napi_set_element(env, arr, (uint32_t)i, b);
    }
    napi_resolve_deferred(env, w->deferred, arr);
  }
  napi_delete_async_work(env, w->work);
  delete w;
}

// verifyBatch(vk: Buffer, proofs: Buffer (count x NZCB_PROOF_BYTES), pubs: Buffer (count x
// nPublic x 32), count: number, transcriptPublic: bool, device: number) -> Promise<boolean[]>
napi_value VerifyBatch(napi_env env, napi_callback_info info) {
  size_t argc = 6;
  napi_value argv[6];
  CHECK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  const uint8_t *vk, *proofs, *pubs;
  size_t vl, pl, ul;
  int32_t count = 0, device = 0;
  bool tp = true;
  if (argc < 4 || !buf_arg(env, argv[0], &vk, &vl) || !buf_arg(env, argv[1], &proofs, &pl) ||
      !buf_arg(env, argv[2], &pubs, &ul) || napi_get_value_int32(env, argv[3], &count) != napi_ok || count < 0 ||
      vl != NZCB_VK_BYTES || pl != (size_t)count * NZCB_PROOF_BYTES || (count ? ul % (32 * (size_t)count) : ul)) {
    napi_throw_type_error(env, nullptr,
                          "verifyBatch(vk: Buffer, proofs: Buffer, pubs: Buffer, count, transcriptPublic, device)");
    return nullptr;
  }
  if (argc > 4) napi_get_value_bool(env, argv[4], &tp);
  if (argc > 5) napi_get_value_int32(env, argv[5], &device);
  VerifyBatchWork* w = new VerifyBatchWork();
  w->vk.assign(vk, vk + vl);
  w->proofs.assign(proofs, proofs + pl);
  w->pubs.assign(pubs, pubs + ul);
  w->count = count;
  w->n_public = count ? (int)(ul / 32 / (size_t)count) : 0;
  w->device = device;
  w->tp = tp;
  w->valid.assign((size_t)count + 1, 0);
  napi_value promise, name;
  if (napi_create_promise(env, &w->deferred, &promise) != napi_ok ||
      napi_create_string_utf8(env, "nzcb.verifyBatch", NAPI_AUTO_LENGTH, &name) != napi_ok ||
      napi_create_async_work(env, nullptr, name, verify_batch_execute, verify_batch_complete, w, &w->work) !=
          napi_ok ||
      napi_queue_async_work(env, w->work) != napi_ok) {
    delete w;
    napi_throw_error(env, nullptr, "nzcb addon: N-API call failed");
    return nullptr;
  }
  return promise;
}

// one wtns.check call: the r1cs parsed and uploaded (nzcb_r1cs_create_file / nzcb_r1cs_create),
// the .wtns checked (nzcb_r1cs_check) and the object released, on a worker thread (async
// work); the promise is settled on the main thread. The inputs are copied.
struct WtnsCheckWork {
  napi_deferred deferred = nullptr;
  napi_async_work work = nullptr;
  std::string r1cs_path;
  std::vector<uint8_t> r1cs, wtns;
  bool from_file = false;
  int device = 0;
  uint32_t info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  nzcb_r1cs_result res{0, 0xffffffffu};
  std::vector<uint32_t> bad;
  int rc = 0;
  nzcb_err err{};
};

void wtns_check_execute(napi_env, void* data) {
  WtnsCheckWork* w = static_cast<WtnsCheckWork*>(data);
  nzcb_r1cs* r = w->from_file ? nzcb_r1cs_create_file(w->r1cs_path.c_str(), w->device, &w->err)
                              : nzcb_r1cs_create(w->r1cs.data(), w->r1cs.size(), w->device, &w->err);
  if (!r) {
    w->rc = w->err.code ? w->err.code : NZCB_ERR_INTERNAL;
    return;
  }
  nzcb_r1cs_info(r, w->info);
  w->rc = nzcb_r1cs_check(r, w->wtns.data(), w->wtns.size(), NZCB_WITNESS_WTNS, 1, 0, &w->res, w->bad.data(),
                          (uint32_t)w->bad.size(), nullptr, &w->err);
  nzcb_r1cs_destroy(r);
}

napi_value u32_array(napi_env env, const uint32_t* v, size_t n) {
  napi_value arr;
  napi_create_array_with_length(env, n, &arr);
  for (size_t i = 0; i < n; i++) {
    napi_value x;
    napi_create_uint32(env, v[i], &x);
    napi_set_element(env, arr, (uint32_t)i, x);
  }
  return arr;
}

void wtns_check_complete(napi_env env, napi_status status, void* data) {
  WtnsCheckWork* w = static_cast<WtnsCheckWork*>(data);
  if (status != napi_ok || w->rc != 0) {
    napi_reject_deferred(env, w->deferred,
                         make_error(env, w->rc ? w->err.code : NZCB_ERR_INTERNAL,
                                    w->rc ? w->err.msg : "wtnsCheck: the work was cancelled"));
  } else {
    napi_value out, n_bad;
    napi_create_object(env, &out);
    napi_create_uint32(env, w->res.n_bad, &n_bad);
    napi_set_named_property(env, out, "nBad", n_bad);
    size_t listed = w->res.n_bad < w->bad.size() ? w->res.n_bad : w->bad.size();
    napi_set_named_property(env, out, "bad", u32_array(env, w->bad.data(), listed));
    napi_set_named_property(env, out, "info", u32_array(env, w->info, 8));
    napi_resolve_deferred(env, w->deferred, out);
  }
  napi_delete_async_work(env, w->work);
  delete w;
}

// wtnsCheck(r1cs: string (file name) | Buffer, wtns: Buffer, device: number, badCap: number)
//   -> Promise<{nBad, bad: number[] (the lowest badCap failing constraints), info: number[8]}>
napi_value WtnsCheck(napi_env env, napi_callback_info info) {
  size_t argc = 4;
  napi_value argv[4];
  CHECK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  WtnsCheckWork* w = new WtnsCheckWork();
  const uint8_t *rb = nullptr, *wb = nullptr;
  size_t rl = 0, wl = 0;
  int32_t device = 0, cap = 8;
  bool ok = argc >= 2 && buf_arg(env, argv[1], &wb, &wl);
  if (ok && str_arg(env, argv[0], &w->r1cs_path)) {
    w->from_file = true;
  } else if (ok && buf_arg(env, argv[0], &rb, &rl)) {
    w->r1cs.assign(rb, rb + rl);
  } else {
    ok = false;
  }
  if (argc > 2) napi_get_value_int32(env, argv[2], &device);
  if (argc > 3) napi_get_value_int32(env, argv[3], &cap);
  if (!ok || cap < 0) {
    delete w;
    napi_throw_type_error(env, nullptr, "wtnsCheck(r1cs: string | Buffer, wtns: Buffer, device?, badCap?)");
    return nullptr;
  }
  w->wtns.assign(wb, wb + wl);
  w->device = device;
  w->bad.assign((size_t)cap, 0xffffffffu);
  napi_value promise, name;
  if (napi_create_promise(env, &w->deferred, &promise) != napi_ok ||
      napi_create_string_utf8(env, "nzcb.wtnsCheck", NAPI_AUTO_LENGTH, &name) != napi_ok ||
      napi_create_async_work(env, nullptr, name, wtns_check_execute, wtns_check_complete, w, &w->work) != napi_ok ||
      napi_queue_async_work(env, w->work) != napi_ok) {
    delete w;
    napi_throw_error(env, nullptr, "nzcb addon: N-API call failed");
    return nullptr;
  }
  return promise;
}

// one powersOfTau.check / zKey.check call (nzcb_ptau_check*, nzcb_zkey_check*) on a worker thread
// (async work); the promise is settled on the main thread. A file name is memory-mapped by the
// library; a Buffer is copied.
struct KeyCheckWork {
  napi_deferred deferred = nullptr;
  napi_async_work work = nullptr;
  bool zkey = false, from_file = false;
  std::string path;
  std::vector<uint8_t> data;
  int device = 0;
  uint64_t count = 0;
  nzcb_key_finding ptau{};
  int ok = 0;
  nzcb_key_finding header_srs[2] = {};
  std::vector<nzcb_key_finding> parts;
  uint32_t n_parts = 0;
  int rc = 0;
  nzcb_err err{};
};

void key_check_execute(napi_env, void* data) {
  KeyCheckWork* w = static_cast<KeyCheckWork*>(data);
  if (!w->zkey) {
    w->rc = w->from_file ? nzcb_ptau_check_file(w->path.c_str(), w->count, w->device, nullptr, &w->ptau, &w->err)
                         : nzcb_ptau_check(w->data.data(), w->data.size(), w->count, w->device, nullptr, &w->ptau,
                                           &w->err);
    return;
  }
  w->parts.assign(8 + 64, nzcb_key_finding{});
  for (int pass = 0; pass < 2; pass++) {  // again only when the key has more parts than fit
    const uint32_t cap = (uint32_t)w->parts.size();
    w->rc = w->from_file ? nzcb_zkey_check_file(w->path.c_str(), w->device, nullptr, &w->ok, w->header_srs,
                                                w->parts.data(), cap, &w->n_parts, &w->err)
                         : nzcb_zkey_check(w->data.data(), w->data.size(), w->device, nullptr, &w->ok, w->header_srs,
                                           w->parts.data(), cap, &w->n_parts, &w->err);
    if (w->rc != 0 || w->n_parts <= cap) break;
    w->parts.assign(w->n_parts, nzcb_key_finding{});
  }
}

napi_value key_finding_object(napi_env env, const nzcb_key_finding& f, bool part) {
  static const char* const names[] = {"OK", "G2", "RANGE", "CURVE", "GENERATOR", "SEQUENCE", "COSETS",
                                      "NONCANONICAL", "LAGRANGE", "EVALS", "COMMIT"};
  napi_value out, v;
  napi_create_object(env, &out);
  napi_create_string_utf8(env, f.status >= 0 && f.status <= NZCB_KEY_ERR_COMMIT ? names[f.status] : "?",
                          NAPI_AUTO_LENGTH, &v);
  napi_set_named_property(env, out, "status", v);
  napi_create_double(env, (double)f.index, &v);
  napi_set_named_property(env, out, "index", v);
  napi_create_double(env, (double)f.n_bad, &v);
  napi_set_named_property(env, out, "nBad", v);
  napi_create_double(env, (double)f.checked, &v);
  napi_set_named_property(env, out, "checked", v);
  if (part) {
    napi_get_boolean(env, f.pairing_checks != 0, &v);
    napi_set_named_property(env, out, "commitChecked", v);
  } else {
    napi_create_uint32(env, f.pairing_checks, &v);
    napi_set_named_property(env, out, "pairingChecks", v);
  }
  return out;
}

void key_check_complete(napi_env env, napi_status status, void* data) {
  KeyCheckWork* w = static_cast<KeyCheckWork*>(data);
  if (status != napi_ok || w->rc != 0) {
    napi_reject_deferred(env, w->deferred,
                         make_error(env, w->rc ? w->err.code : NZCB_ERR_INTERNAL,
                                    w->rc ? w->err.msg : "keyCheck: the work was cancelled"));
  } else if (!w->zkey) {
    napi_resolve_deferred(env, w->deferred, key_finding_object(env, w->ptau, false));
  } else {
    static const char* const part_names[8] = {"Qm", "Ql", "Qr", "Qo", "Qc", "S1", "S2", "S3"};
    napi_value out, ok, parts;
    napi_create_object(env, &out);
    napi_get_boolean(env, w->ok != 0, &ok);
    napi_set_named_property(env, out, "ok", ok);
    napi_set_named_property(env, out, "header", key_finding_object(env, w->header_srs[0], false));
    napi_set_named_property(env, out, "srs", key_finding_object(env, w->header_srs[1], false));
    napi_create_object(env, &parts);
    for (uint32_t k = 0; k < w->n_parts && k < w->parts.size(); k++) {
      const std::string name = k < 8 ? part_names[k] : "L" + std::to_string(k - 8);
      napi_set_named_property(env, parts, name.c_str(), key_finding_object(env, w->parts[k], true));
    }
    napi_set_named_property(env, out, "parts", parts);
    napi_resolve_deferred(env, w->deferred, out);
  }
  napi_delete_async_work(env, w->work);
  delete w;
}

// keyCheck(kind: 0 = ptau | 1 = zkey, file: string (file name) | Buffer, device: number, count: number)
//   -> Promise<finding> (ptau) or Promise<{ok, header, srs, parts: {Qm: finding, ..., L0: ...}}> (zkey);
//   finding = {status: 'OK' | 'G2' | ..., index, nBad, checked, pairingChecks | commitChecked}
napi_value KeyCheck(napi_env env, napi_callback_info info) {
  size_t argc = 4;
  napi_value argv[4];
  CHECK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  KeyCheckWork* w = new KeyCheckWork();
  const uint8_t* b = nullptr;
  size_t bl = 0;
  int32_t kind = -1, device = 0;
  double count = 0;
  bool ok = argc >= 2 && napi_get_value_int32(env, argv[0], &kind) == napi_ok && (kind == 0 || kind == 1);
  if (ok && str_arg(env, argv[1], &w->path)) {
    w->from_file = true;
  } else if (ok && buf_arg(env, argv[1], &b, &bl)) {
    w->data.assign(b, b + bl);
  } else {
    ok = false;
  }
  if (argc > 2) napi_get_value_int32(env, argv[2], &device);
  if (argc > 3) napi_get_value_double(env, argv[3], &count);
  if (!ok || count < 0 || count > 4294967295.0) {
    delete w;
    napi_throw_type_error(env, nullptr, "keyCheck(kind: 0 | 1, file: string | Buffer, device?, count?)");
    return nullptr;
  }
  w->zkey = kind == 1;
  w->device = device;
  w->count = (uint64_t)count;
  napi_value promise, name;
  if (napi_create_promise(env, &w->deferred, &promise) != napi_ok ||
      napi_create_string_utf8(env, "nzcb.keyCheck", NAPI_AUTO_LENGTH, &name) != napi_ok ||
      napi_create_async_work(env, nullptr, name, key_check_execute, key_check_complete, w, &w->work) != napi_ok ||
      napi_queue_async_work(env, w->work) != napi_ok) {
    delete w;
    napi_throw_error(env, nullptr, "nzcb addon: N-API call failed");
    return nullptr;
  }
  return promise;
}

// one powersOfTau.newAccumulator / contribute / preparePhase2 call (nzcb_ptau_new_file,
// nzcb_ptau_contribute_file, nzcb_ptau_prepare_phase2_file) on a worker thread (async work);
// the promise is settled on the main thread. Files are mapped and written by the library.
struct PtauOpWork {
  napi_deferred deferred = nullptr;
  napi_async_work work = nullptr;
  int kind = 0;  // 0 new, 1 contribute, 2 prepare phase 2
  int power = 0, device = 0;
  std::string in_path, out_path, entropy;
  int rc = 0;
  nzcb_err err{};
};

void ptau_op_execute(napi_env, void* data) {
  PtauOpWork* w = static_cast<PtauOpWork*>(data);
  if (w->kind == 0)
    w->rc = nzcb_ptau_new_file(w->power, w->out_path.c_str(), &w->err);
  else if (w->kind == 1)
    w->rc = nzcb_ptau_contribute_file(w->in_path.c_str(), w->out_path.c_str(), nullptr,
                                      reinterpret_cast<const uint8_t*>(w->entropy.data()), w->entropy.size(),
                                      w->device, &w->err);
  else
    w->rc = nzcb_ptau_prepare_phase2_file(w->in_path.c_str(), w->out_path.c_str(), w->device, &w->err);
}

void ptau_op_complete(napi_env env, napi_status status, void* data) {
  PtauOpWork* w = static_cast<PtauOpWork*>(data);
  if (status != napi_ok || w->rc != 0) {
    napi_reject_deferred(env, w->deferred,
                         make_error(env, w->rc ? w->err.code : NZCB_ERR_INTERNAL,
                                    w->rc ? w->err.msg : "ptauOp: the work was cancelled"));
  } else {
    napi_value undef;
    napi_get_undefined(env, &undef);
    napi_resolve_deferred(env, w->deferred, undef);
  }
  napi_delete_async_work(env, w->work);
  delete w;
}

// ptauOp(kind: 0 = new | 1 = contribute | 2 = prepare phase 2, in: string (file name; ignored for
//   new), out: string (file name), power: number (new only), entropy: string, device: number)
//   -> Promise<undefined>. The secrets of a contribution are drawn inside the library.
napi_value PtauOp(napi_env env, napi_callback_info info) {
  size_t argc = 6;
  napi_value argv[6];
  CHECK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  PtauOpWork* w = new PtauOpWork();
  int32_t kind = -1, power = 0, device = 0;
  bool ok = argc >= 3 && napi_get_value_int32(env, argv[0], &kind) == napi_ok && kind >= 0 && kind <= 2 &&
            (kind == 0 || str_arg(env, argv[1], &w->in_path)) && str_arg(env, argv[2], &w->out_path);
  if (ok && argc > 3) napi_get_value_int32(env, argv[3], &power);
  if (ok && argc > 4) (void)str_arg(env, argv[4], &w->entropy);
  if (ok && argc > 5) napi_get_value_int32(env, argv[5], &device);
  if (!ok) {
    delete w;
    napi_throw_type_error(env, nullptr, "ptauOp(kind: 0 | 1 | 2, in: string, out: string, power?, entropy?, device?)");
    return nullptr;
  }
  w->kind = kind;
  w->power = power;
  w->device = device;
  napi_value promise, name;
  if (napi_create_promise(env, &w->deferred, &promise) != napi_ok ||
      napi_create_string_utf8(env, "nzcb.ptauOp", NAPI_AUTO_LENGTH, &name) != napi_ok ||
      napi_create_async_work(env, nullptr, name, ptau_op_execute, ptau_op_complete, w, &w->work) != napi_ok ||
      napi_queue_async_work(env, w->work) != napi_ok) {
    delete w;
    napi_throw_error(env, nullptr, "nzcb addon: N-API call failed");
    return nullptr;
  }
  return promise;
}

// one zKey.newZKey / zKey.contribute call for a Groth16 key (nzcb_groth16_setup_file,
// nzcb_groth16_contribute_file) on a worker thread (async work); the promise is settled on the
// main thread. Files are mapped and written by the library.
struct Groth16OpWork {
  napi_deferred deferred = nullptr;
  napi_async_work work = nullptr;
  int kind = 0;  // 0 setup, 1 contribute
  int device = 0;
  std::string a, b, out_path, entropy;
  int rc = 0;
  nzcb_err err{};
};

void groth16_op_execute(napi_env, void* data) {
  Groth16OpWork* w = static_cast<Groth16OpWork*>(data);
  if (w->kind == 0)
    w->rc = nzcb_groth16_setup_file(w->a.c_str(), w->b.c_str(), w->out_path.c_str(), w->device, &w->err);
  else
    w->rc = nzcb_groth16_contribute_file(w->a.c_str(), w->out_path.c_str(), nullptr,
                                         reinterpret_cast<const uint8_t*>(w->entropy.data()), w->entropy.size(),
                                         w->device, &w->err);
}

void groth16_op_complete(napi_env env, napi_status status, void* data) {
  Groth16OpWork* w = static_cast<Groth16OpWork*>(data);
  if (status != napi_ok || w->rc != 0) {
    napi_reject_deferred(env, w->deferred,
                         make_error(env, w->rc ? w->err.code : NZCB_ERR_INTERNAL,
                                    w->rc ? w->err.msg : "groth16Op: the work was cancelled"));
  } else {
    napi_value undef;
    napi_get_undefined(env, &undef);
    napi_resolve_deferred(env, w->deferred, undef);
  }
  napi_delete_async_work(env, w->work);
  delete w;
}

// groth16Op(kind: 0 = setup | 1 = contribute, a: string (the r1cs, or the old zkey), b: string (the
//   ptau; ignored for contribute), out: string (the zkey written), entropy: string, device: number)
//   -> Promise<undefined>. The secret of a contribution is drawn inside the library.
napi_value Groth16Op(napi_env env, napi_callback_info info) {
  size_t argc = 6;
  napi_value argv[6];
  CHECK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  Groth16OpWork* w = new Groth16OpWork();
  int32_t kind = -1, device = 0;
  bool ok = argc >= 4 && napi_get_value_int32(env, argv[0], &kind) == napi_ok && kind >= 0 && kind <= 1 &&
            str_arg(env, argv[1], &w->a) && (kind == 1 || str_arg(env, argv[2], &w->b)) &&
            str_arg(env, argv[3], &w->out_path);
  if (ok && argc > 4) (void)str_arg(env, argv[4], &w->entropy);
  if (ok && argc > 5) napi_get_value_int32(env, argv[5], &device);
  if (!ok) {
    delete w;
    napi_throw_type_error(env, nullptr, "groth16Op(kind: 0 | 1, a: string, b: string, out: string, entropy?, device?)");
    return nullptr;
  }
  w->kind = kind;
  w->device = device;
  napi_value promise, name;
  if (napi_create_promise(env, &w->deferred, &promise) != napi_ok ||
      napi_create_string_utf8(env, "nzcb.groth16Op", NAPI_AUTO_LENGTH, &name) != napi_ok ||
      napi_create_async_work(env, nullptr, name, groth16_op_execute, groth16_op_complete, w, &w->work) != napi_ok ||
      napi_queue_async_work(env, w->work) != napi_ok) {
    delete w;
    napi_throw_error(env, nullptr, "nzcb addon: N-API call failed");
    return nullptr;
  }
  return promise;
}

// groth16Vk(zkey: string (file name, memory-mapped) | Buffer) -> string: the verification key of
// a Groth16 zkey as JSON (nzcb_groth16_vk_to_json); throws with .code for any other file.
napi_value Groth16Vk(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  CHECK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  std::string path;
  const uint8_t* z = nullptr;
  size_t zl = 0;
  const bool from_file = argc >= 1 && str_arg(env, argv[0], &path);
  if (!from_file && (argc < 1 || !buf_arg(env, argv[0], &z, &zl))) {
    napi_throw_type_error(env, nullptr, "groth16Vk(zkey: string | Buffer)");
    return nullptr;
  }
  auto call = [&](char* out, size_t cap) {
    return from_file ? nzcb_groth16_vk_to_json_file(path.c_str(), out, cap) : nzcb_groth16_vk_to_json(z, zl, out, cap);
  };
  std::string s(256, '\0');
  int rc = call(&s[0], s.size());
  if (rc < 0) {
    s.assign((size_t)-rc, '\0');
    rc = call(&s[0], s.size());
  }
  if (rc != 0) {
    napi_throw(env, make_error(env, rc, s.c_str()));
    return nullptr;
  }
  return json_string(env, std::string(s.c_str()));
}

// one p256Verify call: the key's tables built (nzcb_p256_key_create), the batch verified
// (nzcb_p256_verify) and the key released, on a worker thread (async work); the promise is
// settled on the main thread. The inputs are copied.
struct P256VerifyWork {
  napi_deferred deferred = nullptr;
  napi_async_work work = nullptr;
  uint8_t key[64];
  std::vector<uint8_t> hashes, sigs;
  std::vector<int32_t> status;
  int device = 0;
  int rc = 0;
  nzcb_err err{};
};

void p256_verify_execute(napi_env, void* data) {
  P256VerifyWork* w = static_cast<P256VerifyWork*>(data);
  nzcb_p256_key* k = nzcb_p256_key_create(w->key, w->device, &w->err);
  if (!k) {
    w->rc = w->err.code ? w->err.code : NZCB_ERR_INTERNAL;
    return;
  }
  w->rc = nzcb_p256_verify(k, w->hashes.data(), 32, w->sigs.data(), 64, (int)w->status.size(), 0, w->status.data(),
                           nullptr, &w->err);
  nzcb_p256_key_destroy(k);
}

void p256_verify_complete(napi_env env, napi_status status, void* data) {
  P256VerifyWork* w = static_cast<P256VerifyWork*>(data);
  if (status != napi_ok || w->rc != 0) {
    napi_reject_deferred(env, w->deferred,
                         make_error(env, w->rc ? w->err.code : NZCB_ERR_INTERNAL,
                                    w->rc ? w->err.msg : "p256Verify: the work was cancelled"));
  } else {
    napi_value arr;
    napi_create_array_with_length(env, w->status.size(), &arr);
    for (size_t i = 0; i < w->status.size(); i++) {
      napi_value x;
      napi_create_int32(env, w->status[i], &x);
      napi_set_element(env, arr, (uint32_t)i, x);
    }
    napi_resolve_deferred(env, w->deferred, arr);
  }
  napi_delete_async_work(env, w->work);
  delete w;
}

// p256Verify(key: Buffer (x || y, 64 bytes), hashes: Buffer (32 n), sigs: Buffer (64 n), device: number)
//   -> Promise<number[n]> (NZCB_SIG_*); device -1 is the host path
napi_value P256Verify(napi_env env, napi_callback_info info) {
  size_t argc = 4;
  napi_value argv[4];
  CHECK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  const uint8_t *kb = nullptr, *hb = nullptr, *sb = nullptr;
  size_t kl = 0, hl = 0, sl = 0;
  int32_t device = 0;
  if (argc > 3) napi_get_value_int32(env, argv[3], &device);
  if (argc < 3 || !buf_arg(env, argv[0], &kb, &kl) || !buf_arg(env, argv[1], &hb, &hl) ||
      !buf_arg(env, argv[2], &sb, &sl) || kl != 64 || hl % 32 || sl != hl * 2) {
    napi_throw_type_error(env, nullptr, "p256Verify(key: Buffer(64), hashes: Buffer(32 n), sigs: Buffer(64 n), device?)");
    return nullptr;
  }
  P256VerifyWork* w = new P256VerifyWork();
  memcpy(w->key, kb, 64);
  w->hashes.assign(hb, hb + hl);
  w->sigs.assign(sb, sb + sl);
  w->status.assign(hl / 32, NZCB_SIG_INVALID);
  w->device = device;
  napi_value promise, name;
  if (napi_create_promise(env, &w->deferred, &promise) != napi_ok ||
      napi_create_string_utf8(env, "nzcb.p256Verify", NAPI_AUTO_LENGTH, &name) != napi_ok ||
      napi_create_async_work(env, nullptr, name, p256_verify_execute, p256_verify_complete, w, &w->work) != napi_ok ||
      napi_queue_async_work(env, w->work) != napi_ok) {
    delete w;
    napi_throw_error(env, nullptr, "nzcb addon: N-API call failed");
    return nullptr;
  }
  return promise;
}

// one nzcpDecode call on a worker thread: the URIs decoded (nzcb_nzcp_decode, on the GPU or with
// device -1 on the host) and, when a key came with them, each record's digest checked against
// its signature (nzcb_p256_verify reading both out of the record array by stride). The inputs are
// copied; the promise is settled on the main thread.
struct NzcpDecodeWork {
  napi_deferred deferred = nullptr;
  napi_async_work work = nullptr;
  std::vector<uint8_t> uris, data, records, inputs;
  std::vector<uint32_t> offsets;
  std::vector<int32_t> status;
  nzcb_nzcp_params prm{};
  bool has_prm = false, has_key = false;
  uint8_t key[64];
  int device = 0;
  int rc = 0;
  nzcb_err err{};
};

void nzcp_decode_execute(napi_env, void* data) {
  NzcpDecodeWork* w = static_cast<NzcpDecodeWork*>(data);
  const int count = (int)w->offsets.size() - 1;
  uint32_t lay[3];
  nzcb_nzcp_pass_layout(lay);
  w->records.assign((size_t)lay[0] * count, 0);
  if (w->has_prm) w->inputs.assign(nzcb_nzcp_input_signals(&w->prm) * 32 * (size_t)count, 0);
  w->rc = nzcb_nzcp_decode(w->device, w->uris.data(), w->offsets.data(), count, w->has_prm ? &w->prm : nullptr,
                           w->data.empty() ? nullptr : w->data.data(),
                           reinterpret_cast<nzcb_nzcp_pass*>(w->records.data()),
                           w->has_prm ? w->inputs.data() : nullptr, nullptr, 0, &w->err);
  if (w->rc || !w->has_key || !count) return;
  nzcb_p256_key* k = nzcb_p256_key_create(w->key, w->device, &w->err);
  if (!k) {
    w->rc = w->err.code ? w->err.code : NZCB_ERR_INTERNAL;
    return;
  }
  w->status.assign(count, NZCB_SIG_INVALID);
  w->rc = nzcb_p256_verify(k, w->records.data() + lay[2], lay[0], w->records.data() + lay[1], lay[0], count, 0,
                           w->status.data(), nullptr, &w->err);
  nzcb_p256_key_destroy(k);
}

void nzcp_decode_complete(napi_env env, napi_status status, void* data) {
  NzcpDecodeWork* w = static_cast<NzcpDecodeWork*>(data);
  if (status != napi_ok || w->rc != 0) {
    napi_reject_deferred(env, w->deferred,
                         make_error(env, w->rc ? w->err.code : NZCB_ERR_INTERNAL,
                                    w->rc ? w->err.msg : "nzcpDecode: the work was cancelled"));
  } else {
    napi_value out, v;
    napi_create_object(env, &out);
    napi_create_buffer_copy(env, w->records.size(), w->records.data(), nullptr, &v);
    napi_set_named_property(env, out, "records", v);
    if (w->has_prm) {
      napi_create_buffer_copy(env, w->inputs.size(), w->inputs.data(), nullptr, &v);
      napi_set_named_property(env, out, "inputs", v);
    }
    if (w->has_key) {
      napi_create_array_with_length(env, w->status.size(), &v);
      for (size_t i = 0; i < w->status.size(); i++) {
        napi_value x;
        napi_create_int32(env, w->status[i], &x);
        napi_set_element(env, v, (uint32_t)i, x);
      }
      napi_set_named_property(env, out, "status", v);
    }
    napi_resolve_deferred(env, w->deferred, out);
  }
  napi_delete_async_work(env, w->work);
  delete w;
}

// nzcpDecode(uris: Buffer (the URIs back to back), offsets: Buffer (count + 1 u32 LE), maxTbsBytes:
//            number (0 = no circuit inputs), data: Buffer (20 count) | null, device: number,
//            key: Buffer (64) | null)
//   -> Promise<{records: Buffer (count nzcb_nzcp_pass), inputs?: Buffer, status?: number[count]}>
napi_value NzcpDecode(napi_env env, napi_callback_info info) {
  size_t argc = 6;
  napi_value argv[6];
  CHECK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  const uint8_t *ub = nullptr, *ob = nullptr, *db = nullptr, *kb = nullptr;
  size_t ul = 0, ol = 0, dl = 0, kl = 0;
  int32_t max_tbs = 0, device = 0;
  const char* usage = "nzcpDecode(uris: Buffer, offsets: Buffer(4 (n + 1)), maxTbsBytes, data: Buffer(20 n) | null, "
                      "device, key: Buffer(64) | null)";
  if (argc < 6 || !buf_arg(env, argv[0], &ub, &ul) || !buf_arg(env, argv[1], &ob, &ol) || ol < 4 || ol % 4 ||
      napi_get_value_int32(env, argv[2], &max_tbs) != napi_ok ||
      napi_get_value_int32(env, argv[4], &device) != napi_ok) {
    napi_throw_type_error(env, nullptr, usage);
    return nullptr;
  }
  const size_t count = ol / 4 - 1;
  // null stands for "none": only a Buffer may go to napi_get_buffer_info
  auto optional = [&](napi_value v, const uint8_t** p, size_t* l) {
    bool is = false;
    return napi_is_buffer(env, v, &is) == napi_ok && is && buf_arg(env, v, p, l);
  };
  const bool has_data = optional(argv[3], &db, &dl), has_key = optional(argv[5], &kb, &kl);
  if ((has_data && dl != 20 * count) || (has_key && kl != 64) || count > 0x7fffffffu) {
    napi_throw_type_error(env, nullptr, usage);
    return nullptr;
  }
  NzcpDecodeWork* w = new NzcpDecodeWork();
  w->uris.assign(ub, ub + ul);
  w->offsets.resize(count + 1);
  memcpy(w->offsets.data(), ob, ol);  // little-endian hosts only, as the rest of the addon
  if (w->offsets[count] > ul) {       // the C ABI trusts the offsets to lie within the buffer
    delete w;
    napi_throw_range_error(env, nullptr, "nzcpDecode: the offsets run past the URI bytes");
    return nullptr;
  }
  if (has_data) w->data.assign(db, db + dl);
  if (max_tbs) {
    w->has_prm = true;
    w->prm.max_tbs_bytes = max_tbs;
  }
  if (has_key) {
    w->has_key = true;
    memcpy(w->key, kb, 64);
  }
  w->device = device;
  napi_value promise, name;
  if (napi_create_promise(env, &w->deferred, &promise) != napi_ok ||
      napi_create_string_utf8(env, "nzcb.nzcpDecode", NAPI_AUTO_LENGTH, &name) != napi_ok ||
      napi_create_async_work(env, nullptr, name, nzcp_decode_execute, nzcp_decode_complete, w, &w->work) != napi_ok ||
      napi_queue_async_work(env, w->work) != napi_ok) {
    delete w;
    napi_throw_error(env, nullptr, "nzcb addon: N-API call failed");
    return nullptr;
  }
  return promise;
}

// nzcpPassLayout() -> [sizeof(nzcb_nzcp_pass), offsetof sig, offsetof tbs_sha256]
napi_value NzcpPassLayout(napi_env env, napi_callback_info) {
  uint32_t lay[3];
  nzcb_nzcp_pass_layout(lay);
  napi_value arr;
  CHECK(napi_create_array_with_length(env, 3, &arr));
  for (uint32_t i = 0; i < 3; i++) {
    napi_value x;
    CHECK(napi_create_uint32(env, lay[i], &x));
    CHECK(napi_set_element(env, arr, i, x));
  }
  return arr;
}

// r1csInfo(path: string) -> number[8] (nzcb_r1cs_info; parsed on the host, no GPU)
napi_value R1csInfo(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  CHECK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  std::string path;
  if (argc < 1 || !str_arg(env, argv[0], &path)) {
    napi_throw_type_error(env, nullptr, "r1csInfo(path: string)");
    return nullptr;
  }
  nzcb_err err{};
  nzcb_r1cs* r = nzcb_r1cs_create_file(path.c_str(), NZCB_R1CS_HOST, &err);
  if (!r) {
    napi_throw(env, make_error(env, err.code, err.msg));
    return nullptr;
  }
  uint32_t v[8];
  nzcb_r1cs_info(r, v);
  nzcb_r1cs_destroy(r);
  return u32_array(env, v, 8);
}

// calldata(proof: Buffer, pub: Buffer) -> string (snarkjs `zkey export soliditycalldata`)
napi_value Calldata(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  CHECK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  const uint8_t *proof, *pub;
  size_t pl, ul;
  if (argc < 2 || !buf_arg(env, argv[0], &proof, &pl) || !buf_arg(env, argv[1], &pub, &ul) ||
      pl != NZCB_PROOF_BYTES || ul % 32) {
    napi_throw_type_error(env, nullptr, "calldata(proof: Buffer, pub: Buffer)");
    return nullptr;
  }
  std::string s((size_t)nzcb_proof_to_calldata(proof, pub, (int)(ul / 32), nullptr, 0), '\0');
  nzcb_proof_to_calldata(proof, pub, (int)(ul / 32), &s[0], s.size());
  s.resize(std::strlen(s.c_str()));
  return json_string(env, s);
}

// vkToSolidity(vk: Buffer, name: string, transcriptPublic: bool) -> string
// (snarkjs `zkey export solidityverifier`)
napi_value VkToSolidity(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value argv[3];
  CHECK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  const uint8_t* vk;
  size_t vl;
  char name[80] = {0};
  size_t nl = 0;
  bool tp = true;
  if (argc < 3 || !buf_arg(env, argv[0], &vk, &vl) || vl != NZCB_VK_BYTES ||
      napi_get_value_string_utf8(env, argv[1], name, sizeof(name), &nl) != napi_ok ||
      napi_get_value_bool(env, argv[2], &tp) != napi_ok) {
    napi_throw_type_error(env, nullptr, "vkToSolidity(vk: Buffer, name: string, transcriptPublic: boolean)");
    return nullptr;
  }
  const int need = nzcb_vk_to_solidity(vk, name, tp ? 1 : 0, nullptr, 0);
  if (need < 0) {
    napi_throw_error(env, nullptr, "solidity verifier: bad verification key or contract name");
    return nullptr;
  }
  std::string s((size_t)need, '\0');
  nzcb_vk_to_solidity(vk, name, tp ? 1 : 0, &s[0], s.size());
  s.resize(std::strlen(s.c_str()));
  return json_string(env, s);
}

// nzcpWitness(inputs: Buffer, count: number, params: [isLive, maxTbsBytes, maxArrayLenVC,
// maxMapLenVC], device: number) -> Buffer of count nzcb_nzcp_record (include/nzcb.h).
// Synchronous: one launch of the nzcp witness kernel, well under a millisecond.
napi_value NzcpWitness(napi_env env, napi_callback_info info) {
  size_t argc = 4;
  napi_value argv[4];
  CHECK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  void* data = nullptr;
  size_t len = 0;
  CHECK(napi_get_buffer_info(env, argv[0], &data, &len));
  int32_t count = 0, device = 0;
  CHECK(napi_get_value_int32(env, argv[1], &count));
  nzcb_nzcp_params prm{};
  int32_t* fields[4] = {&prm.is_live, &prm.max_tbs_bytes, &prm.max_array_len_vc, &prm.max_map_len_vc};
  for (uint32_t i = 0; i < 4; i++) {
    napi_value v;
    CHECK(napi_get_element(env, argv[2], i, &v));
    CHECK(napi_get_value_int32(env, v, fields[i]));
  }
  if (argc > 3) napi_get_value_int32(env, argv[3], &device);
  if (count < 0 || len != nzcb_nzcp_input_signals(&prm) * 32 * (size_t)count) {
    napi_throw_error(env, nullptr, "nzcpWitness: inputs must be count x input signals x 32 bytes");
    return nullptr;
  }
  void* out_data = nullptr;
  napi_value out;
  CHECK(napi_create_buffer(env, sizeof(nzcb_nzcp_record) * (size_t)(count ? count : 1), &out_data, &out));
  nzcb_err err{};
  int rc = nzcb_nzcp_witness(device, &prm, static_cast<const uint8_t*>(data), count,
                             static_cast<nzcb_nzcp_record*>(out_data), &err);
  if (rc) {
    napi_throw(env, make_error(env, err.code, err.msg));
    return nullptr;
  }
  return out;
}

// plonkSetup(r1cs: Buffer, ptau: Buffer, device: number) -> Buffer (the zkey):
// snarkjs `plonk setup` (nzcb_plonk_setup). Synchronous: a one-off key generation.
napi_value PlonkSetup(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value argv[3];
  CHECK(napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr));
  const uint8_t *r1cs, *ptau;
  size_t rl, pl;
  int32_t device = 0;
  if (argc < 2 || !buf_arg(env, argv[0], &r1cs, &rl) || !buf_arg(env, argv[1], &ptau, &pl)) {
    napi_throw_type_error(env, nullptr, "plonkSetup(r1cs: Buffer, ptau: Buffer, device?: number)");
    return nullptr;
  }
  if (argc > 2) napi_get_value_int32(env, argv[2], &device);
  uint8_t* zk = nullptr;
  size_t zl = 0;
  nzcb_err err{};
  if (nzcb_plonk_setup(r1cs, rl, ptau, pl, device, &zk, &zl, &err)) {
    napi_throw(env, make_error(env, err.code, err.msg));
    return nullptr;
  }
  void* out_data = nullptr;
  napi_value out;
  napi_status stc = napi_create_buffer_copy(env, zl, zk, &out_data, &out);
  nzcb_free(zk);
  CHECK(stc);
  return out;
}

napi_value Init(napi_env env, napi_value exports) {
  napi_property_descriptor props[] = {
      {"createContext", nullptr, CreateContext, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"prove", nullptr, Prove, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"info", nullptr, Info, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"version", nullptr, Version, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"deviceCount", nullptr, DeviceCount, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"vkFromZkey", nullptr, VkFromZkey, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"vkFromZkeyFile", nullptr, VkFromZkeyFile, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"remapWitnessProgram", nullptr, RemapWitnessProgram, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"vkToJson", nullptr, VkToJson, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"verify", nullptr, Verify, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"verifyBatch", nullptr, VerifyBatch, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"calldata", nullptr, Calldata, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"vkToSolidity", nullptr, VkToSolidity, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"nzcpWitness", nullptr, NzcpWitness, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"plonkSetup", nullptr, PlonkSetup, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"createContextFile", nullptr, CreateContextFile, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"createWitnessProgram", nullptr, CreateWitnessProgram, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"calculateWitness", nullptr, CalculateWitness, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"fullProveDevice", nullptr, FullProveDevice, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"setLanes", nullptr, SetLanes, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"releaseContext", nullptr, ReleaseContext, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"wtnsCheck", nullptr, WtnsCheck, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"keyCheck", nullptr, KeyCheck, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"ptauOp", nullptr, PtauOp, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"groth16Op", nullptr, Groth16Op, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"groth16Vk", nullptr, Groth16Vk, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"r1csInfo", nullptr, R1csInfo, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"p256Verify", nullptr, P256Verify, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"nzcpDecode", nullptr, NzcpDecode, nullptr, nullptr, nullptr, napi_default, nullptr},
      {"nzcpPassLayout", nullptr, NzcpPassLayout, nullptr, nullptr, nullptr, napi_default, nullptr},
  };
  napi_define_properties(env, exports, sizeof(props) / sizeof(props[0]), props);
  return exports;
}

}  // namespace

NAPI_MODULE(NODE_GYP_MODULE_NAME, Init)
