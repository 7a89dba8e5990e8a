/*
 * nzcb — MI355X-native PLONK prover for the nzcb circom circuit (C-ABI).
 *
 * This is the drop-in boundary under the reference's prover call:
 *   snarkjs.plonk.prove(zkeyFileName, witnessFileName, logger)      [EXT] snarkjs 0.4.12
 *   snarkjs.plonk.fullProve(input, wasmFile, zkeyFileName, logger)  [EXT]
 * pinned at /root/reference/package.json:18 and /root/reference/yarn.lock:7279-7292,
 * whose keys are produced at /root/reference/Makefile:54-62.
 * The N-API addon in nzcb-circom_amd/js/ binds these functions one-to-one
 * (see INTEGRATION.md). Plain pointers and sizes only; the caller owns every
 * buffer; nothing is retained after a call returns.
 *
 * Byte layouts
 *   zkey / wtns : snarkjs 0.4 binary files, unchanged.
 *   proof       : NZCB_PROOF_BYTES = 9 G1 affine points (A,B,C,Z,T1,T2,T3,Wxi,Wxiw),
 *                 each x||y as 32-byte little-endian normal-form integers
 *                 (infinity = 64 zero bytes), then 7 Fr evaluations
 *                 (eval_a,eval_b,eval_c,eval_s1,eval_s2,eval_zw,eval_r), 32 B LE each.
 *   public      : nPublic x 32-byte LE Fr (= witness[1..nPublic]).
 *   blinding    : 11 x 32-byte LE Fr (b1..b11), or NULL = drawn uniformly from the
 *                 OS CSPRNG per proof, as snarkjs's Fr.random() (zero-knowledge).
 *                 Fixed bytes (352 zero bytes included) give reproducible,
 *                 bit-exact proofs for tests; zero blinding is NOT zero-knowledge.
 *
 * This header is the product ABI. Kernel-level entry points for tests,
 * microbenchmarks and tuning (nzcb_engine_*, the synthetic-circuit setup, kernel timing)
 * are in nzcb_internal.h: they are exported by the same library but are not part of the
 * drop-in boundary and may change between releases. Until round 3 they were declared here;
 * code that used them through this header compiles with -DNZCB_WITH_INTERNAL (this header
 * then includes nzcb_internal.h) or includes nzcb_internal.h itself.
 */
#ifndef NZCB_H
#define NZCB_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NZCB_PROOF_BYTES (9 * 64 + 7 * 32)
#define NZCB_BLINDING_BYTES (11 * 32)

/* Error codes; messages reproduce the snarkjs 0.4.12 exception text. */
enum {
  NZCB_OK = 0,
  NZCB_ERR_ARG = 1,
  NZCB_ERR_FORMAT = 2,
  NZCB_ERR_NOT_PLONK = 3,     /* "zkey file is not plonk" */
  NZCB_ERR_CURVE = 4,         /* "Curve of the witness does not match the curve of the proving key" */
  NZCB_ERR_WITNESS_LEN = 5,   /* "Invalid witness length. Circuit: ..., witness: ..., ..." */
  NZCB_ERR_COPY = 6,          /* "Copy constraints does not match" */
  NZCB_ERR_T_DIV = 7,         /* "T Polynomial is not divisible" */
  NZCB_ERR_TZ = 8,            /* "Tz Polynomial is not well calculated" */
  NZCB_ERR_DIVPOL = 9,        /* "Polinomial does not divide" */
  NZCB_ERR_HIP = 10,
  NZCB_ERR_INTERNAL = 11
};

/* Every entry point that takes an nzcb_err* (NULL is allowed) and returns an int or a handle sets
 * err->code on every return, 0 on success, and writes err->msg only on failure. */
typedef struct nzcb_err {
  int code;
  char msg[256];
} nzcb_err;

typedef struct nzcb_ctx nzcb_ctx;
typedef void (*nzcb_log_fn)(void* user, const char* msg);

/* Library identity / devices. */
const char* nzcb_version(void);
int nzcb_device_count(void);

/* ---- Prover (replaces snarkjs plonk_prove) ---------- */

/* Parse a snarkjs 0.4 PLONK zkey and upload it to `device` (HBM-resident,
 * context-owned). Replaces the zkey read in snarkjs plonk_prove.js [EXT]. */
nzcb_ctx* nzcb_ctx_create(const uint8_t* zkey, size_t zkey_len, int device, nzcb_err* err);
/* SURVEY.md §8b's form: one context over a device set. Every device holds its own
 * HBM-resident copy of the proving key; nzcb_prove_batch spreads its items over the
 * lanes of all devices (nzcb_ctx_set_lanes sets lanes per device); single proofs run on
 * devices[0]. nzcb_ctx_create(z, len, d, err) is this with devices = {d}. */
nzcb_ctx* nzcb_ctx_create_devices(const uint8_t* zkey, size_t zkey_len, const int* devices, int ndev, nzcb_err* err);
/* The same from a zkey file (memory-mapped, nothing retained after the call): zkeys of
 * nzcp_live size (~3.9 GB) exceed what a Node.js Buffer holds. devices NULL = device 0. */
nzcb_ctx* nzcb_ctx_create_file(const char* zkey_path, const int* devices, int ndev, nzcb_err* err);
int nzcb_ctx_devices(const nzcb_ctx* ctx);
void nzcb_ctx_destroy(nzcb_ctx* ctx);

/* Optional progress logger (snarkjs `logger.debug` lines). */
void nzcb_ctx_set_logger(nzcb_ctx* ctx, nzcb_log_fn fn, void* user);

/* Include the public inputs in the beta transcript (1, default)
 * or hash A||B||C only (0). */
void nzcb_ctx_set_transcript_public(nzcb_ctx* ctx, int on);

/* Context facts: domain size, nPublic, nVars, nAdditions, nConstraints. */
int nzcb_ctx_info(const nzcb_ctx* ctx, uint32_t out[5]);

/* One proof. wtns = snarkjs .wtns bytes. proof_out: NZCB_PROOF_BYTES.
 * pub_out: pub_cap >= 32 * nPublic bytes. Returns NZCB_OK or an error code. */
int nzcb_prove(nzcb_ctx* ctx, const uint8_t* wtns, size_t wtns_len, const uint8_t* blinding, uint8_t* proof_out,
               uint8_t* pub_out, size_t pub_cap, nzcb_err* err);

/* Same with the witness given as nWitness x 32-byte LE field elements (no file header). */
int nzcb_prove_witness(nzcb_ctx* ctx, const uint8_t* witness, size_t n_witness, const uint8_t* blinding,
                       uint8_t* proof_out, uint8_t* pub_out, size_t pub_cap, nzcb_err* err);

/* Same with the witness already resident in HBM: dev_witness is a device pointer
 * (nzcb_dev_alloc) holding nWitness x 32-byte LE normal-form values. */
int nzcb_prove_device(nzcb_ctx* ctx, const void* dev_witness, size_t n_witness, const uint8_t* blinding,
                      uint8_t* proof_out, uint8_t* pub_out, size_t pub_cap, nzcb_err* err);

/* One proof with its own logger (NULL: the context's, nzcb_ctx_set_logger), the witness in
 * any of the three forms above: NZCB_WITNESS_WTNS (.wtns bytes, n = byte length),
 * NZCB_WITNESS_HOST (n x 32-byte LE values in host memory), NZCB_WITNESS_DEVICE (the same
 * in HBM). Concurrent calls on one context (several host threads; the N-API addon's
 * in-flight promises) each take a free lane and run at the same time; a call waits while
 * every lane is proving. nzcb_prove, nzcb_prove_witness and nzcb_prove_device are this
 * with the context's logger. */
#define NZCB_WITNESS_WTNS 0
#define NZCB_WITNESS_HOST 1
#define NZCB_WITNESS_DEVICE 2
int nzcb_prove_logged(nzcb_ctx* ctx, const void* witness, size_t n, int kind, const uint8_t* blinding,
                      uint8_t* proof_out, uint8_t* pub_out, size_t pub_cap, nzcb_log_fn log, void* log_user,
                      nzcb_err* err);

/* Proof lanes (default 1): each extra lane is a per-proof working set + streams on
 * the context's device (~6.5 GB at n = 2^21) sharing the HBM-resident proving key,
 * so nzcb_prove_batch keeps `lanes` proofs in flight and one proof's latency-bound
 * phases (Fiat-Shamir host steps, bucket reductions) overlap another's compute. A change
 * of the count waits for the proofs in flight (it rebuilds the lane pool); setting the
 * count the context already has returns at once. */
int nzcb_ctx_set_lanes(nzcb_ctx* ctx, int lanes, nzcb_err* err);
int nzcb_ctx_lanes(const nzcb_ctx* ctx);

/* Single-proof mode across GPUs: every commitment MSM of lane 0
 * is split by point range over devices[0..ndev) (devices[0] = the context's device); each
 * other device holds the shifted-base tables of its PTau range and of its range of the n + 2
 * Lagrange-basis points (A, B, C's commitments, when the context commits them in that basis),
 * receives its scalar slice by a peer copy over xGMI and returns one partial, which the host
 * adds. ndev = 1 restores the single-device schedule. Results are bit-identical either way. */
int nzcb_ctx_set_msm_devices(nzcb_ctx* ctx, const int* devices, int ndev, nzcb_err* err);

/* The same split across processes, one rank per GPU (each rank's
 * slice of the scalars by RCCL scatter, one 64-byte partial per rank back by gather; the
 * collectives live in the host runtime, e.g. torch.distributed, see nzcb/msmsplit.py). The
 * context (rank 0) computes PTau points [0, own_points) of every commitment of lane 0 and,
 * when own_lagrange > 0, Lagrange-basis points [0, own_lagrange) of A, B and C's commitments
 * (own_lagrange = 0 keeps those three whole on this rank), and calls
 *   send(user, slot, dev_scalars, count): the commitment's `count` scalars (32-byte
 *       Montgomery Fr, HBM of the context's device) are ready; the other ranks take the
 *       points [own, count) of it; called when the commitment starts. `slot` carries
 *       NZCB_MSM_LAGRANGE when the commitment is over the Lagrange basis (the n + 2 points
 *       [L_k(tau)] for k < n, [tau^n] - [1], [tau^(n+1)] - [tau]; a serving rank's table of
 *       its range comes from nzcb_msm_table_create_lagrange) rather than PTau
 *   gather(user, slot, own_partial, partials_out): returns world x 64 bytes, every rank's
 *       partial sum (affine x || y, 32-byte LE normal form, infinity = zeros) in rank
 *       order (own_partial at index 0); called when the commitment is needed, with the
 *       same slot value as its send
 * Up to 3 commitments (slot & 0xff = 0..2) are in flight at once. A callback returning
 * non-zero fails the proof. world = 1 or NULL callbacks restore the local schedule. */
#define NZCB_MSM_LAGRANGE 0x100
typedef int (*nzcb_msm_send_fn)(void* user, int slot, const void* dev_scalars, size_t count);
typedef int (*nzcb_msm_gather_fn)(void* user, int slot, const uint8_t* own_partial, uint8_t* partials_out);
int nzcb_ctx_set_msm_split(nzcb_ctx* ctx, int world, size_t own_points, size_t own_lagrange,
                           nzcb_msm_send_fn send, nzcb_msm_gather_fn gather, void* user, nzcb_err* err);

/* `count` independent proofs over the context's lanes (SURVEY.md §8b nzcb_prove_batch,
 * §8e batch mode). witnesses[i]: nWitness x 32-byte LE normal-form values, host memory,
 * or device pointers when witness_on_device. blindings: count x NZCB_BLINDING_BYTES or
 * NULL (random per proof, see `blinding` above). proofs_out: count x NZCB_PROOF_BYTES. pubs_out: count x pub_stride
 * (pub_stride >= 32 * nPublic). Returns the error of the lowest failing index. */
int nzcb_prove_batch(nzcb_ctx* ctx, const void* const* witnesses, size_t n_witness, int count, int witness_on_device,
                     const uint8_t* blindings, uint8_t* proofs_out, uint8_t* pubs_out, size_t pub_stride,
                     nzcb_err* err);
/* As nzcb_prove_batch, but a failed proof does not stop the batch: every
 * item is proved, status_out[i] (count ints) receives 0 or proof i's error code, and a
 * failed item's proof and public bytes are zeroed. Returns (and reports in err) the
 * error of the lowest failing index, 0 when all succeed. */
int nzcb_prove_batch_status(nzcb_ctx* ctx, const void* const* witnesses, size_t n_witness, int count,
                            int witness_on_device, const uint8_t* blindings, uint8_t* proofs_out, uint8_t* pubs_out,
                            size_t pub_stride, int* status_out, nzcb_err* err);

/* Milliseconds of the last proof's phases. Host wall clock: [0] total [1] witness
 * upload+additions+ABC [2] round1 [3] round2 [4] round3 [5] round4 [6] round5, [7] host time
 * inside the MSM calls (enqueue + waiting for their results), [8] host time enqueueing the
 * transforms. GPU time (HIP events around each commitment MSM / each transform on its
 * stream, only while nzcb_ctx_kernel_stats is on, else -1): [9] MSMs [10] transforms.
 * Returns the number of values written (cap <= 11). */
int nzcb_ctx_last_timings(const nzcb_ctx* ctx, double* ms, int cap);

/* snarkjs-format JSON ({proof}, [publicSignals]) from the binary outputs. */
int nzcb_proof_to_json(const uint8_t* proof, char* out, size_t cap);
int nzcb_public_to_json(const uint8_t* pub, int n_public, char* out, size_t cap);

/* ---- Verification key, verifier, Solidity calldata ----
 * Host-only (no GPU needed). Binary verification key, NZCB_VK_BYTES:
 *   u32 nPublic | u32 power | k1, k2 (Fr, 32 B LE) | Qm Ql Qr Qo Qc S1 S2 S3 (G1 x||y,
 *   32 B LE each, infinity = zeros) | X_2 (x.c0 x.c1 y.c0 y.c1, 32 B LE) | w (Fr, 32 B LE)
 * Replaces snarkjs `zkey export verificationkey` (/root/reference/Makefile:56,61). */
#define NZCB_VK_BYTES (8 + 2 * 32 + 8 * 64 + 4 * 32 + 32)
int nzcb_vk_from_zkey(const uint8_t* zkey, size_t zkey_len, uint8_t* vk_out, nzcb_err* err);
/* The same from a zkey file, memory-mapped (zkeys past 2 GiB, e.g. nzcp_live's ~3.9 GB, which
 * `snarkjs zkey export verificationkey|solidityverifier nzcp_live_final.zkey` reads,
 * /root/reference/Makefile:61-62). */
int nzcb_vk_from_zkey_file(const char* zkey_path, uint8_t* vk_out, nzcb_err* err);
/* verification_key.json text (snarkjs layout); returns 0, or the needed size if cap is short. */
int nzcb_vk_to_json(const uint8_t* vk, char* out, size_t cap);
/* snarkjs plonk.verify: *valid = 1 if the proof (NZCB_PROOF_BYTES) is valid for the public
 * signals (n_public x 32 B LE), else 0. transcript_public as nzcb_ctx_set_transcript_public. */
int nzcb_verify(const uint8_t* vk, const uint8_t* proof, const uint8_t* pub, int n_public, int transcript_public,
                int* valid, nzcb_err* err);
/* nzcb_verify for `count` proofs of one key at once: one pairing check for the whole batch
 * instead of one per proof, and the 20 G1 scalar multiplications of every proof on GPU
 * `device` (own stream and buffers per call, no nzcb_ctx needed; may run while a context
 * proves on the same device). device = NZCB_VERIFY_HOST runs the same algorithm with the
 * scalar multiplications on the host, so the library still verifies without a GPU.
 *   proofs : count x NZCB_PROOF_BYTES;  pubs : item i at pubs + i * pub_stride
 *   (pub_stride >= 32 * n_public);  valid_out : count ints.
 * Returns 0 when the batch was examined, whatever the verdicts (count = 0 is fine).
 * valid_out[i] is what nzcb_verify says of item i, up to the soundness error of the random
 * weights: the items are combined under independent 128-bit weights rho_i, so a batch holding
 * an invalid item passes a combined check with probability of order 2^-128; a failing check is
 * bisected (at most 1 + 2 k ceil(log2 N) pairing checks for k invalid among N well-formed items).
 * seed = NULL draws the weights from the OS CSPRNG, like the blinding. A 32-byte seed makes
 * rho_i the low 128 bits of keccak256(seed || LE32(i)) (the digest read as a big-endian
 * integer; zero becomes 1): FOR REPRODUCIBLE TESTS ONLY, since whoever knows the weights
 * before choosing the proofs can make invalid items cancel. */
#define NZCB_VERIFY_HOST (-1)
int nzcb_verify_batch(const uint8_t* vk, const uint8_t* proofs /* count x NZCB_PROOF_BYTES */,
                      const uint8_t* pubs, size_t pub_stride, int n_public, int count,
                      int transcript_public, int device /* >= 0, or NZCB_VERIFY_HOST */,
                      const uint8_t* seed /* 32 B or NULL */, int* valid_out /* count */, nzcb_err* err);
/* snarkjs `zkey export soliditycalldata` for PLONK (/root/reference/Makefile:57,62 verifier):
 * "0x<proof hex>,[\"0x<pub>\",...]"; returns 0, or the needed size if cap is short. */
int nzcb_proof_to_calldata(const uint8_t* proof, const uint8_t* pub, int n_public, char* out, size_t cap);
/* snarkjs `zkey export solidityverifier` (/root/reference/Makefile:57,62; the contract
 * /root/reference/deploy-script.js:4-7 deploys): a Solidity PLONK verifier for this key,
 * verifyProof(bytes proof, uint256[] pubSignals) taking the soliditycalldata arguments
 * above. contract_name: NULL = "PlonkVerifier" (snarkjs's name; the reference's deploy
 * script asks for "Verifier"). transcript_public as nzcb_verify. Returns 0, the needed
 * size if cap is short, or -1 for a bad key or name. Parity unpinned (csrc/solidity.cpp). */
int nzcb_vk_to_solidity(const uint8_t* vk, const char* contract_name, int transcript_public, char* out, size_t cap);

/* ---- nzcp witness -----------------------------------
 * The semantic signals and public outputs of NZCPPubIdentity
 * (/root/reference/circuits/nzcptpl.circom:444-655, cbortpl.circom, quinSelector.circom)
 * for a batch of passes, one GPU workgroup per pass. Replaces, for the signals the
 * proof's public inputs depend on, circom_runtime's
 *   WitnessCalculator.calculateWitness(input, sanityCheck)   [EXT] circom_runtime 0.1.17
 * as called by snarkjs plonk.fullProve (wtns_calculate) and by the reference tests
 * (test/nzcp.js:42 `cir.calculateWitness(input, true)`).
 * Inputs per pass: the main's input signals in declaration order, each a 32-byte LE
 * field element (values >= r are reduced): toBeSigned[8*max_tbs_bytes] (bits, MSB
 * first per byte, test/helpers/utils.js:2-10), toBeSignedLen, data[160]
 * (nzcb_nzcp_input_signals() elements). Status codes mirror the circuit's failing
 * constraint or assert (the first one in template order); oracle/nzcp_circuit.py
 * is the CPU restatement with the same codes. */
enum {
  NZCB_NZCP_OK = 0,
  NZCB_NZCP_ERR_BIT = 1,        /* toBeSigned[i] * (toBeSigned[i] - 1) === 0 (detail = i) */
  NZCB_NZCP_ERR_LEN = 2,        /* toBeSignedLen < MaxToBeSignedBytes + 1 */
  NZCB_NZCP_ERR_RANGE = 3,      /* a LessThan / Num2Bits operand outside its bit range */
  NZCB_NZCP_ERR_SELECT = 4,     /* QuinSelector index >= choices (detail = index) */
  NZCB_NZCP_ERR_NOT_MAP = 5,    /* ReadMapLength: CBOR type is not a map */
  NZCB_NZCP_ERR_UINT23 = 6,     /* DecodeUint23: map length > 23 */
  NZCB_NZCP_ERR_NOT_STRING = 7, /* ReadStringLength: CBOR type is not a string */
  NZCB_NZCP_ERR_UNPINNED = 8    /* negative toBeSignedLen: Sha256Var behaviour not on disk */
};

/* NZCPPubIdentity(IsLive, MaxToBeSignedBytes, MaxCborArrayLenVC, MaxCborMapLenVC, ...):
 * nzcp_live = {1, 351, 0, 4}, nzcp_example = {0, 314, 0, 4} (circuits/nzcp_*.circom). */
typedef struct nzcb_nzcp_params {
  int32_t is_live;          /* CWT claims map at byte 30 (live) or 27 (example) */
  int32_t max_tbs_bytes;    /* 1..512 */
  int32_t max_array_len_vc; /* 0..8 */
  int32_t max_map_len_vc;   /* 0..32 */
} nzcb_nzcp_params;

/* One pass's result. On status != OK every other field except detail is zero. */
typedef struct nzcb_nzcp_record {
  int32_t status;
  int32_t detail;
  uint32_t exp;             /* CWT claim 4 */
  int32_t vc_pos;           /* FindCWTClaims.vcPos */
  int32_t given_len, family_len, dob_len, nullifier_len;
  uint8_t tbs_sha256[32];   /* SHA-256(ToBeSigned) */
  uint8_t nullifier_sha512[64];
  uint8_t nullifier[64];    /* "given,family,dob" zero-padded (ConstructNullifier.result) */
  uint8_t pub[3][32];       /* out[0..2] = witness[1..3], 32-byte LE normal-form Fr */
} nzcb_nzcp_record;

size_t nzcb_nzcp_input_signals(const nzcb_nzcp_params* prm);
/* Host buffers: inputs count x nzcb_nzcp_input_signals() x 32 B; records: count. */
int nzcb_nzcp_witness(int device, const nzcb_nzcp_params* prm, const uint8_t* inputs, int count,
                      nzcb_nzcp_record* records, nzcb_err* err);
/* Device buffers, asynchronous on `stream` (a hipStream_t, NULL = default stream).
 * dev_records may be NULL. When dev_witness is not NULL, pass i's out[0..2] are also
 * written as witness[1..3] of the witness at dev_witness + i * witness_stride (bytes),
 * so the prover's public inputs come straight from the pass (fullProve on device). */
int nzcb_nzcp_witness_dev(int device, const nzcb_nzcp_params* prm, const void* dev_inputs, int count,
                          void* dev_records, void* dev_witness, size_t witness_stride, void* stream,
                          nzcb_err* err);

/* ---- Witness programs: the circom witness calculator on the GPU ------------------
 * Replaces circom_runtime's calculateWitness / snarkjs wtns_calculate (circom_runtime
 * 0.1.17, /root/reference/yarn.lock:2496) for circuits
 * compiled by nzcb-circom_amd/nzcb/circuit.py (nzcp_live = NZCPPubIdentity(1, 351, 0, 4,
 * 2, 4), nzcb/nzcpgen.py). The program (format: csrc/wvm.hip) is uploaded once; each
 * run computes `count` full witnesses, one workgroup each.
 *   inputs : count x (n_pub_in + n_prv_in) x 32-byte LE field elements, the main's
 *            input signals in declaration order (as nzcb_nzcp_input_signals for nzcp)
 *   witness: witness i at dev_witness + i * witness_stride: n_wires x 32-byte LE normal
 *            form (wire 0 = 1, outputs, inputs, intermediate signals), the wtns order
 *            that nzcb_prove_device / nzcb_prove_batch take
 *   status : per witness, 0 or the failure code of the first failing check in circuit
 *            order (nzcp: NZCB_NZCP_* codes), as circom's calculator throws */
typedef struct nzcb_wprog nzcb_wprog;
nzcb_wprog* nzcb_wprog_create(const uint8_t* prog, size_t len, int device, nzcb_err* err);
void nzcb_wprog_destroy(nzcb_wprog* prog);
/* info: n_wires, n_outputs, n_pub_inputs, n_prv_inputs, n_levels */
int nzcb_wprog_info(const nzcb_wprog* prog, uint32_t info[5]);
/* Device buffers; stream may be NULL; returns after the statuses are on the host. */
int nzcb_wprog_run_dev(nzcb_wprog* prog, const void* dev_inputs, int count, void* dev_witness,
                       size_t witness_stride, int32_t* status_out, void* stream, nzcb_err* err);
/* Host buffers: witness_out receives count x n_wires x 32 bytes. */
int nzcb_wprog_run(nzcb_wprog* prog, const uint8_t* inputs, int count, uint8_t* witness_out,
                   int32_t* status_out, nzcb_err* err);
/* Re-index a witness program to another wire order by signal name (a zkey
 * built from circom's own r1cs, /root/reference/Makefile:12-15,59-62, expects circom's
 * wire order). own_sym: the program's .sym text (nzcb/circuit.py Circuit.write_sym);
 * target_sym: the .sym of the target order (e.g. circom's nzcp_live.sym; lines
 * "label,wire,component,name", wire -1 = optimized out). Target wire t gets the program
 * signal of the same name; wire 0 stays the constant 1. The result (malloc'ed, release
 * with nzcb_free) runs like any program and writes witnesses of the target's wire count.
 * Fails with NZCB_ERR_FORMAT, *unmatched = the count, when a target signal has no
 * counterpart. Parity of the names with circom's own .sym is unpinned (nzcb/nzcpgen.py). */
int nzcb_wprog_remap(const uint8_t* prog, size_t prog_len, const char* own_sym, size_t own_len,
                     const char* target_sym, size_t target_len, uint8_t** prog_out, size_t* prog_out_len,
                     uint32_t* unmatched, nzcb_err* err);

/* ---- Witness check (snarkjs `wtns check <r1cs> <wtns>`, circom_tester checkConstraints) ----
 * An iden3 r1cs parsed once and kept resident on `device` (three sparse matrices, the distinct
 * coefficients in one table), then checked against batches of witnesses: constraint k of
 * witness w fails iff (A_k . w)(B_k . w) != C_k . w in Fr. An empty side is 0; wire 0 is read
 * from the witness like any other wire; repeated wires within a side add up; witness values
 * >= r count modulo r. device = NZCB_R1CS_HOST runs the same functions on the host, so the
 * library still checks without a GPU; the outputs are the same bytes on both paths and do not
 * depend on `count`, on the order of the witnesses or on the launch geometry. Unknown
 * sections of the file are ignored. NZCB_ERR_CURVE when the prime is not BN254's r,
 * NZCB_ERR_FORMAT for a malformed file (the setup reader's texts) or 2^32 or more terms. */
#define NZCB_R1CS_HOST (-1)
typedef struct nzcb_r1cs nzcb_r1cs;
nzcb_r1cs* nzcb_r1cs_create(const uint8_t* r1cs, size_t len, int device, nzcb_err* err);
/* The same from a file, memory-mapped (nothing retained after the call). */
nzcb_r1cs* nzcb_r1cs_create_file(const char* path, int device, nzcb_err* err);
/* info: n_wires, n_outputs, n_pub_inputs, n_prv_inputs, n_constraints, n_terms,
 * long_row_threshold (rows with at least that many terms get a wavefront each, the others a
 * lane), n_long_rows */
int nzcb_r1cs_info(const nzcb_r1cs* r, uint32_t info[8]);
typedef struct nzcb_r1cs_result {
  uint32_t n_bad;     /* failing constraints */
  uint32_t first_bad; /* the lowest failing index, 0xffffffff when n_bad = 0 */
} nzcb_r1cs_result;
/* `count` witnesses against the r1cs. kind: NZCB_WITNESS_WTNS (.wtns bytes, count = 1, n = byte
 * length), NZCB_WITNESS_HOST or NZCB_WITNESS_DEVICE (n = values per witness; witness i at
 * witness + i * witness_stride, n x 32-byte LE normal form: what nzcb_wprog_run_dev writes and
 * nzcb_prove_device reads; device pointers and strides are multiples of 16; witness_stride 0
 * with count = 1 means 32 n). results: count. bad_out (may be NULL): count x bad_cap u32,
 * witness i's lowest min(n_bad, bad_cap) failing constraint indices, ascending, the rest
 * 0xffffffff. Returns 0 whatever the verdicts (count = 0 is fine); NZCB_ERR_WITNESS_LEN
 * ("Invalid witness length. Circuit: ..., witness: ...") when n is not n_wires. stream: a
 * hipStream_t to order the work on, NULL = a stream of the call's own; either way the call
 * owns its buffers, returns with the results on the host and may run while a context proves on
 * the same device. */
int nzcb_r1cs_check(nzcb_r1cs* r, const void* witness, size_t n, int kind, int count, size_t witness_stride,
                    nzcb_r1cs_result* results, uint32_t* bad_out, uint32_t bad_cap, void* stream, nzcb_err* err);
void nzcb_r1cs_destroy(nzcb_r1cs* r);

/* ---- Pass signature (COSE ES256) ------------------------------------------------------ */
/* ECDSA over NIST P-256 with SHA-256, the signature of an NZ COVID Pass, verified in batches
 * (csrc/p256_verify.hip). The circuit does not check it; @vaxxnz/nzcp's verifyPassURIOffline
 * did that in the reference's flow. A key object validates a public key (coordinates below p,
 * on the curve, not (0, 0); otherwise NZCB_ERR_ARG "public key is not a point on P-256") and
 * keeps fixed-base window tables for G and for the key (about 1 MB) resident on GPU `device`,
 * built there; device = NZCB_P256_HOST builds them on the host with the same functions and
 * verifies there. Whether the key is to be trusted (the issuer's DID document) is the caller's
 * business. All byte strings are big-endian, as in a JWK, a COSE signature and a SHA-256
 * digest: pub_xy = x || y. */
#define NZCB_P256_HOST (-1)
enum { NZCB_SIG_OK = 0, NZCB_SIG_INVALID = 1, NZCB_SIG_RANGE = 2 }; /* RANGE: r or s not in [1, n-1] */
typedef struct nzcb_p256_key nzcb_p256_key;
nzcb_p256_key* nzcb_p256_key_create(const uint8_t pub_xy[64], int device, nzcb_err* err);
/* status_out[i] (host memory) = NZCB_SIG_* for hash i, 32 bytes at hashes + i * hash_stride
 * (the SHA-256 of the pass's COSE Sig_structure; a hash >= n counts modulo n), and signature i,
 * r || s at sigs + i * sig_stride. Standard ECDSA: no low-s rule. on_device: both are HBM
 * pointers on the key's device, pointers and strides multiples of 4, read in place: hashes =
 * dev_records + offsetof(nzcb_nzcp_record, tbs_sha256) with hash_stride =
 * sizeof(nzcb_nzcp_record) verifies what nzcb_nzcp_witness_dev wrote (a host key object
 * cannot); such buffers must be complete when the call starts, or their producer enqueued on
 * the same `stream` before it (a stream of the call's own waits for no other stream, and
 * nzcb_nzcp_witness_dev is asynchronous). Host buffers may have any strides >= 32 and 64. Returns 0 whatever the verdicts
 * (count = 0 is fine) and the statuses do not depend on the batch, its order or the path; the
 * call owns its device buffers, runs on `stream` (a HIP stream of the key's device) or on a
 * stream of its own, returns with the statuses on the host, and may run while a context
 * proves on the same device. */
int nzcb_p256_verify(nzcb_p256_key* k, const void* hashes, size_t hash_stride, const void* sigs, size_t sig_stride,
                     int count, int on_device, int32_t* status_out, void* stream, nzcb_err* err);
void nzcb_p256_key_destroy(nzcb_p256_key* k);

/* ---- Pass decode (NZCP:/<version>/<base32> -> COSE_Sign1 -> digest and circuit inputs) ---- */
/* What a holder presents is the URI. nzcb_nzcp_decode takes batches of them, one GPU workgroup
 * per pass (csrc/nzcp_decode.hip; the functions themselves are csrc/nzcp_decode.h, the same on
 * both paths, device = NZCB_NZCP_HOST runs them in a host loop), and leaves per pass a fixed-size
 * record, the SHA-256 of the COSE Sig_structure where nzcb_p256_verify reads it in place, and the
 * main's input signals where nzcb_nzcp_witness_dev / nzcb_wprog_run_dev read them. The input is
 * untrusted: no step reads outside the URI, the decoded COSE bytes or the item it is parsing, and
 * every length taken from the input is compared in 64 bits against the bytes left before it is
 * used. Steps, in this order; the first failing one sets status and detail and ends the pass:
 *   LENGTH    the URI is longer than NZCB_PASS_MAX_URI bytes (detail = its length)
 *   PREFIX    not "NZCP:/", one to nine decimal digits (version: reported, not judged), "/" and
 *             at least one more byte
 *   BASE32    a byte of the rest outside A-Z2-7 (detail = the lowest such index in the URI); no
 *             padding, no lower case. The COSE bytes are the floor(5 L / 8) whole bytes.
 *   CBOR heads, definite lengths only, shortest form not required: additional info 28..31 (the
 *             break byte included) gives CBOR; a head, a string body or an array / map item
 *             count that exceeds the bytes left of the region being parsed gives TRUNCATED
 *             (detail of both = the head's offset in the COSE bytes). Values that are not looked
 *             at are skipped with a counter of items still to read: any nesting depth, no stack.
 *   NOT_COSE  not tag 18 around an array of 4, or item 0 (protected header) or item 2 (payload)
 *             is not a byte string (detail = the offending head). Item 1 is skipped. Item 3: a
 *             byte string gives sig_len and, when it is 64 bytes, sig; anything else is skipped
 *             and NZCB_PASS_HAS_SIG stays clear. Bytes after the COSE item are ignored.
 *   HEADER    the protected bytes do not begin with a map. Key 1 with an integer value: alg
 *             (saturated to int32); key 4 with a byte string: kid.
 *   CLAIMS    the payload does not begin with a map. Key 1 with a text value: iss; 4 and 5 with
 *             unsigned values: exp, nbf; 7 with a byte string: cti. In both maps everything else
 *             is skipped, a repeated key's last occurrence counts, and a known key whose value
 *             has another type is absent. Both are parsed within their own byte string only.
 * Then ToBeSigned = 84 6a "Signature1" bstr(protected) 40 bstr(payload) with shortest heads,
 * tbs_len and tbs_sha256. On status != OK every field but status, detail and version is zero
 * (version is set once PREFIX has passed). */
#define NZCB_PASS_MAX_URI 2048
#define NZCB_NZCP_HOST (-1)
enum {
  NZCB_PASS_OK = 0,
  NZCB_PASS_ERR_LENGTH = 1,
  NZCB_PASS_ERR_PREFIX = 2,
  NZCB_PASS_ERR_BASE32 = 3,
  NZCB_PASS_ERR_TRUNCATED = 4,
  NZCB_PASS_ERR_CBOR = 5,
  NZCB_PASS_ERR_NOT_COSE = 6,
  NZCB_PASS_ERR_HEADER = 7,
  NZCB_PASS_ERR_CLAIMS = 8
};
enum {
  NZCB_PASS_HAS_ALG = 1,
  NZCB_PASS_HAS_KID = 2,
  NZCB_PASS_HAS_ISS = 4,
  NZCB_PASS_HAS_NBF = 8,
  NZCB_PASS_HAS_EXP = 16,
  NZCB_PASS_HAS_CTI = 32,
  NZCB_PASS_HAS_SIG = 64
};
typedef struct nzcb_nzcp_pass {
  int32_t status;          /* NZCB_PASS_* */
  uint32_t detail;
  uint32_t version;
  uint32_t present;        /* NZCB_PASS_HAS_* */
  int32_t alg;             /* -7 = ES256 */
  uint32_t kid_len, iss_len, cti_len, sig_len; /* true lengths; the arrays hold the first bytes */
  uint32_t cose_len;       /* COSE bytes consumed */
  uint32_t protected_off, protected_len, payload_off, payload_len; /* within the COSE bytes */
  uint32_t tbs_len;
  uint32_t fits;           /* 1: the pass's input block is filled */
  uint64_t nbf, exp;
  uint8_t kid[32];
  uint8_t cti[32];
  uint8_t iss[64];
  uint8_t sig[64];         /* r || s when sig_len = 64, zeros otherwise */
  uint8_t tbs_sha256[32];
} nzcb_nzcp_pass;
/* out = {sizeof(nzcb_nzcp_pass), offsetof sig, offsetof tbs_sha256}: both offsets are multiples
 * of 4 and the size of 8, so nzcb_p256_verify(k, recs + out[2], out[0], recs + out[1], out[0],
 * count, on_device = 1, ...) verifies a record array in place. */
void nzcb_nzcp_pass_layout(uint32_t out[3]);
/* Host buffers. uris: the URIs' bytes back to back, URI i = [offsets[i], offsets[i + 1]);
 * offsets: count + 1 values, non-decreasing, the last at most 2^31 (NZCB_ERR_ARG otherwise).
 * prm: the circuit whose inputs to build (only max_tbs_bytes counts), NULL = none. data20: count
 * x 20 pass-through bytes, NULL = zeros. passes_out: count records. inputs_out (may be NULL, needs
 * prm): count x nzcb_nzcp_input_signals(prm) x 32 bytes; pass i's block is the main's input
 * signals (toBeSigned bits, toBeSignedLen, data bits after the reversed-bytes / reversed-bits
 * rearrangement) when status = OK and tbs_len <= max_tbs_bytes (fits = 1), all zero bytes
 * otherwise (fits = 0). tbs_out (may be NULL): pass i's first min(tbs_len, tbs_stride) ToBeSigned
 * bytes at tbs_out + i * tbs_stride, zeros after them. Returns 0 whatever the verdicts (count = 0
 * is fine); the records do not depend on the batch, its order or the path. */
int nzcb_nzcp_decode(int device, const uint8_t* uris, const uint32_t* offsets, int count,
                     const nzcb_nzcp_params* prm, const uint8_t* data20, nzcb_nzcp_pass* passes_out,
                     uint8_t* inputs_out, uint8_t* tbs_out, size_t tbs_stride, nzcb_err* err);
/* The same over HBM buffers on `device`, asynchronous on `stream` (a hipStream_t, NULL = the
 * default stream) like nzcb_nzcp_witness_dev: work enqueued on the stream afterwards sees the
 * results. dev_passes is a multiple of 8, dev_inputs of 16. dev_offsets is read back once, ordered on
 * the stream, to validate it before the kernel is enqueued: the call waits for the stream's earlier
 * work, not for its own kernel. */
int nzcb_nzcp_decode_dev(int device, const void* dev_uris, const void* dev_offsets, int count,
                         const nzcb_nzcp_params* prm, const void* dev_data20, void* dev_passes, void* dev_inputs,
                         void* dev_tbs, size_t tbs_stride, void* stream, nzcb_err* err);

/* ---- Setup ------------------------------------------ */
/* snarkjs `plonk setup <r1cs> <ptau> <zkey>` (snarkjs 0.4.12 plonk_setup.js, run at
 * /root/reference/Makefile:55,60): iden3 r1cs + powers-of-tau file -> snarkjs-0.4 PLONK
 * zkey (malloc'ed, release with nzcb_free). Uses the ptau's tauG1 (section 2) and
 * tauG2 (section 3); NTTs and commitments run on `device`. */
int nzcb_plonk_setup(const uint8_t* r1cs, size_t r1cs_len, const uint8_t* ptau, size_t ptau_len, int device,
                     uint8_t** zkey_out, size_t* zkey_len, nzcb_err* err);
/* A powers-of-tau file (sections 1-3 of the snarkjs ptau layout: header, tauG1 =
 * [tau^i]G1 for i < 2^(power+1) - 1, tauG2 = [1]G2, [tau]G2) for a trapdoor tau (32 B LE),
 * built on `device`; malloc'ed, release with nzcb_free. The offline stand-in for
 * powersOfTau28_hez_final_21.ptau (/root/reference/README.md:40, Makefile:60). */
int nzcb_ptau_synth(int power, const uint8_t* tau, int device, uint8_t** ptau_out, size_t* ptau_len, nzcb_err* err);
void nzcb_free(void* p);

/* ---- Key material check (csrc/key_check.h, csrc/key_check.hip) --------------------------- */
/* Is a powers-of-tau file what it claims to be: P_i = [tau^i]G1 for the tau of its [tau]G2?
 * nzcb_plonk_setup copies its points into the key untested, and a wrong point shows up only as
 * "Invalid proof" later. The steps run in this order and the first that fails sets the
 * finding:
 *   G2        T = tauG2[1] has a stored coordinate >= q, is the point at infinity, is not on
 *             the twist, or [r]T != O (host, once);
 *   points    every P_i: a stored coordinate >= q (RANGE), or (0, 0) or y^2 != x^3 + 3
 *             (CURVE). status is that of the lowest defective point, index is that point and
 *             n_bad counts all defective points;
 *   generator P_0 != (1, 2), or tauG2[0] is not the G2 generator (index 0);
 *   sequence  with weights rho_i, L = sum rho_i P_i and R = sum rho_i P_(i+1) over
 *             0 <= i < m - 1 (two MSMs on the GPU): e(-L, T) e(R, [1]_2) = 1. When that fails,
 *             index is the lowest i >= 1 with P_i != tau P_(i-1), found by bisection with
 *             sub-sums of the same terms: pairing_checks is 1 on the clean path and at most
 *             2 + ceil(log2 m) on a failing one. A wrong file passes a check with probability
 *             of order 2^-128.
 * rho_i is the low 128 bits of keccak256(seed || LE32(i)) (the digest read as a big-endian
 * integer; zero becomes 1), nzcb_verify_batch's rule. seed = NULL draws a 32-byte seed from the
 * OS CSPRNG. A caller-given seed is FOR REPRODUCIBLE TESTS ONLY: whoever knows the weights
 * before making the file can make wrong points cancel.
 * The points go through the GPU in chunks that overlap by one point, so HBM use does not grow
 * with the file. device = NZCB_KEY_HOST runs the same steps on the host (no speed target);
 * the findings are the same. A call owns its stream and buffers, needs no nzcb_ctx and may run
 * while a context proves on the same device.
 * NOT examined: the ceremony's contributions (what snarkjs `powersoftau verify` audits), the
 * alpha and beta sections, the Lagrange sections and tauG2 past [tau]G2. */
#define NZCB_KEY_HOST (-1)
enum {
  NZCB_KEY_OK = 0,
  NZCB_KEY_ERR_G2,
  NZCB_KEY_ERR_RANGE,
  NZCB_KEY_ERR_CURVE,
  NZCB_KEY_ERR_GENERATOR,
  NZCB_KEY_ERR_SEQUENCE,
  NZCB_KEY_ERR_COSETS,       /* zkey findings from here on */
  NZCB_KEY_ERR_NONCANONICAL,
  NZCB_KEY_ERR_LAGRANGE,
  NZCB_KEY_ERR_EVALS,
  NZCB_KEY_ERR_COMMIT
};
typedef struct nzcb_key_finding {
  int32_t status;          /* NZCB_KEY_* */
  uint32_t pairing_checks; /* pairing checks the call ran; a zkey part: commit_checked, 1 if rule 4 ran */
  uint64_t index;          /* the point the status speaks of (0 when it names none) */
  uint64_t n_bad;          /* RANGE / CURVE: all defective points */
  uint64_t checked;        /* points examined */
} nzcb_key_finding;
/* ptau: header (section 1: n8 = 32, q, power), tauG1 (section 2) and tauG2 (section 3); other
 * sections are ignored. count = 0 checks every point the header promises, 2^(power+1) - 1;
 * otherwise the first `count` (a circuit of domain 2^p uses 2^p + 6). Returns 0 with the
 * verdict in *out whatever the content says; NZCB_ERR_FORMAT for a missing or short section,
 * NZCB_ERR_ARG for a count larger than section 2 holds. */
int nzcb_ptau_check(const uint8_t* ptau, size_t len, uint64_t count, int device /* >= 0, or NZCB_KEY_HOST */,
                    const uint8_t* seed /* 32 B or NULL */, nzcb_key_finding* out, nzcb_err* err);
/* The same from a file, memory-mapped (a power-28 ptau is 34 GB). */
int nzcb_ptau_check_file(const char* path, uint64_t count, int device, const uint8_t* seed, nzcb_key_finding* out,
                         nzcb_err* err);
/* Is a PLONK zkey consistent with itself? A truncated download or a flipped bit in its
 * evaluations loads without complaint today and surfaces as "Invalid proof" or "T Polynomial
 * is not divisible". The file is parsed as nzcb_ctx_create parses it (its errors are this
 * call's non-zero returns); every verdict about the content returns 0:
 *   header_srs[0]  NZCB_KEY_ERR_COSETS when k1^n = 1, k2^n = 1 or (k2 / k1)^n = 1 (or one is
 *                  zero): <w>, k1 <w>, k2 <w> are then not three disjoint cosets.
 *                  NZCB_KEY_ERR_NONCANONICAL when k1 (index 0) or k2 (index 1) is stored >= r;
 *   header_srs[1]  the check of nzcb_ptau_check over section 14's n + 6 points against the
 *                  header's X_2;
 *   parts[0..7]    Qm, Ql, Qr, Qo, Qc, S1, S2, S3, then parts[8 + j], the max(nPublic, 1)
 *                  Lagrange polynomials. Each is n coefficients and 4n evaluations; every part
 *                  is examined whatever the others say and its status is the first rule it fails:
 *     NONCANONICAL one of its 5n stored values is >= r (index: the lowest, in 0..5n; n_bad: all);
 *     LAGRANGE     Lagrange parts only: the n-point transform of the coefficients is not the
 *                  unit vector e_j (index: the lowest mismatch; n_bad: all);
 *     EVALS        the 4n stored evaluations are not byte-equal to the 4n-point transform of
 *                  the coefficients padded with zeros, which is what `plonk setup` writes
 *                  (index: the lowest mismatch; n_bad: the number of mismatches);
 *     COMMIT       parts 0..7 only, and only when header_srs[1] is OK: the header's point is
 *                  not the MSM of the coefficients over PTau[0..n). pairing_checks records
 *                  whether this rule ran (commit_checked).
 * parts_cap findings are written at most; *n_parts is always 8 + max(nPublic, 1). *ok = 1 iff
 * every finding is NZCB_KEY_OK. device and seed as for nzcb_ptau_check.
 * OUT OF SCOPE: whether sigma is the permutation of YOUR circuit, the A/B/C maps and the
 * additions; they need the r1cs. Regenerating the key with `plonk setup` and comparing remains
 * the way to check those. */
int nzcb_zkey_check(const uint8_t* zkey, size_t len, int device, const uint8_t* seed, int* ok,
                    nzcb_key_finding* header_srs /* [2] */, nzcb_key_finding* parts, uint32_t parts_cap,
                    uint32_t* n_parts, nzcb_err* err);
/* The same from a file, memory-mapped (nzcp_live's zkey is ~3.9 GB). */
int nzcb_zkey_check_file(const char* path, int device, const uint8_t* seed, int* ok, nzcb_key_finding* header_srs,
                         nzcb_key_finding* parts, uint32_t parts_cap, uint32_t* n_parts, nzcb_err* err);

/* ---- Powers of tau: new, contribute, prepare phase 2 (csrc/ptau_ops.h, csrc/ptau_ops.hip) ---- */
/* The three steps of snarkjs's `phase1` recipe (`powersoftau new`, `contribute`, `prepare phase2`)
 * for bn128 and 1 <= power <= 24 (NZCB_ERR_ARG outside that). Points are LEM affine as in the
 * other sections this library reads; the point at infinity is all zero bytes. A file holds
 *   1 header (n8 = 32, q, power, ceremonyPower), 2 tauG1 (2^(power+1) - 1 points), 3 tauG2
 *   (2^power), 4 alphaTauG1 (2^power), 5 betaTauG1 (2^power), 6 betaG2 (1), 7 contributions,
 * and a prepared file also 12, 13, 14, 15, the Lagrange forms of 2, 3, 4, 5.
 * Each operation has a buffer form (result malloc'ed, release with nzcb_free) and a _file form
 * that maps the input and writes the output path itself (a prepared power-21 file is 2.25 GiB);
 * the output path must not be the input file. device = NZCB_PTAU_HOST runs the same steps on the
 * host (no speed target); the bytes are identical. A call owns its stream and buffers, needs no
 * nzcb_ctx and may run while a context proves on the same device.
 *
 * nzcb_ptau_new: sections 1-7 with every point its group's generator and section 7 = u32 0.
 * Host only.
 *
 * nzcb_ptau_contribute: with `old` the input's point at index i, the output holds
 *   tauG1[i] = tau^i old, tauG2[i] = tau^i old, alphaTauG1[i] = alpha tau^i old,
 *   betaTauG1[i] = beta tau^i old, betaG2 = beta old;
 * sections 1 and 7 are copied, sections 12-15 and unknown sections are dropped (they would be
 * stale). secrets: 96 B, tau || alpha || beta, 32-byte LE each, in [1, r) (NZCB_ERR_ARG
 * otherwise), or NULL: 96 bytes from the OS CSPRNG, each secret keccak256(random || entropy ||
 * k) mod r for k = 0, 1, 2 (k one byte, the digest read as a big-endian integer; a zero result
 * is redrawn); entropy may be NULL with entropy_len = 0. Caller-given secrets are FOR
 * REPRODUCIBLE TESTS ONLY: whoever knows them knows the trapdoor of the output. The secrets
 * are wiped from host and device memory before the call returns and are never logged or
 * returned. Before any arithmetic every input point is tested on the GPU: a stored coordinate
 * below q and the point on its curve (G1: y^2 = x^3 + 3; G2: the twist y^2 = x^3 + 3 / (9 + u));
 * (0, 0) fails. The failure is NZCB_ERR_FORMAT "ptau: section <id> point <lowest bad index> ...".
 * Membership of a G2 point in the subgroup of order r is NOT tested per point.
 * NO CONTRIBUTION RECORD IS WRITTEN: no blake2b challenge chain and no proofs of knowledge, so
 * `snarkjs powersoftau verify` does not accept the output. The use is re-randomising a file for
 * yourself so that nobody knows its trapdoor, not an audited multi-party ceremony.
 *
 * nzcb_ptau_prepare_phase2: copies sections 1-7 and appends 12-15. For a source section with
 * points P_i and a level p, n = 2^p: out_p[k] = sum_{i<n} (1/n) w_n^(-ik) P_i in natural order,
 * w_n the root of unity the prover's transforms use. A section is its levels p = 0..power back
 * to back (level 0 is P_0); section 12 also carries level power + 1 over the 2^(power+1) - 1
 * tauG1 points followed by the point at infinity. (0, 0) in the input is the point at infinity;
 * the input's points are not tested. */
#define NZCB_PTAU_HOST (-1)
int nzcb_ptau_new(int power, uint8_t** ptau_out, size_t* ptau_len, nzcb_err* err);
int nzcb_ptau_new_file(int power, const char* out_path, nzcb_err* err);
int nzcb_ptau_contribute(const uint8_t* ptau, size_t len, const uint8_t* secrets /* 96 B or NULL */,
                         const uint8_t* entropy, size_t entropy_len, int device /* >= 0, or NZCB_PTAU_HOST */,
                         uint8_t** ptau_out, size_t* ptau_len, nzcb_err* err);
int nzcb_ptau_contribute_file(const char* in_path, const char* out_path, const uint8_t* secrets,
                              const uint8_t* entropy, size_t entropy_len, int device, nzcb_err* err);
int nzcb_ptau_prepare_phase2(const uint8_t* ptau, size_t len, int device, uint8_t** ptau_out, size_t* ptau_len,
                             nzcb_err* err);
int nzcb_ptau_prepare_phase2_file(const char* in_path, const char* out_path, int device, nzcb_err* err);

/* ---- Groth16 key generation: setup, zkey contribute, verification key (csrc/groth16.h, .hip) ---- */
/* The first three lines of snarkjs's `phase2` recipe (`groth16 setup`, `zkey contribute`, `zkey
 * export verificationkey`) for bn128. This is key generation only: there is no Groth16 prover,
 * verifier or Solidity verifier here, and nzcb_vk_from_zkey, nzcb_ctx_create and nzcb_zkey_check
 * keep rejecting a Groth16 key ("zkey file is not plonk").
 *
 * THE FILE LAYOUT BELOW IS THE SPECIFICATION; PARITY WITH snarkjs 0.4.12 IS UNPINNED (it is
 * restated from the published format, and snarkjs was not available to compare with).
 * NO CIRCUIT HASH AND NO CONTRIBUTION RECORDS ARE WRITTEN: section 10 is 64 zero bytes and a
 * count of 0, there is no blake2b transcript and no proof of knowledge, so `snarkjs zkey verify`
 * does not accept a key made or contributed to here. The use is making a key for yourself whose
 * delta nobody knows, not an audited multi-party ceremony.
 *
 * nzcb_groth16_setup: an iden3 r1cs over BN254's r (NZCB_ERR_CURVE otherwise) with m constraints,
 * nVars wires and nPublic = nOutputs + nPubInputs, and a powers-of-tau file with sections 1-7 and
 * 12-15 as nzcb_ptau_prepare_phase2 writes them (NZCB_ERR_FORMAT "ptau: not prepared for phase 2
 * (section 12 is missing)" otherwise). cirPower = floor(log2(m + nPublic)) + 1, n = 2^cirPower;
 * cirPower above the file's power is NZCB_ERR_ARG "circuit too big for this power of tau
 * ceremony. <m>*2 > 2**<power>". With L12..L15 level cirPower of sections 12-15, T level
 * cirPower + 1 of section 12 and a, b, c the coefficients of constraint c' at signal s:
 *   A[s]  = sum a L12[c']  (+ L12[m + s] for s <= nPublic)                       G1, nVars
 *   B1[s] = sum b L12[c'],  B2[s] = sum b L13[c'] (G2)                           nVars each
 *   K[s]  = sum a L15[c'] + b L14[c'] + c L12[c']  (+ L15[m + s] for s <= nPublic)
 *   IC = K[0..nPublic], C = K[nPublic + 1..nVars - 1], H[i] = T[2 i + 1] for i < n,
 *   alpha1 = section 4 point 0, beta1 = section 5 point 0, beta2 = section 6,
 *   gamma2 = delta2 = [1]G2, delta1 = [1]G1.
 * A FRESH KEY HAS delta = gamma = 1: ANYONE CAN FORGE PROOFS UNDER IT UNTIL IT HAS BEEN
 * CONTRIBUTED TO. A zero coefficient adds nothing to a point but stays in section 4; a wire
 * listed twice in a linear combination counts twice; an empty sum is the point at infinity.
 * The file: magic "zkey", version 1, sections 1..10 in order, points LEM affine, infinity all
 * zero bytes:
 *   1  u32 1 (groth16)
 *   2  u32 32, q, u32 32, r, u32 nVars, u32 nPublic, u32 n, alpha1, beta1, beta2, gamma2, delta1, delta2
 *   3  IC, nPublic + 1 G1
 *   4  u32 nCoefs, then per entry u32 matrix (0 = A, 1 = B), u32 constraint, u32 signal, 32 B value:
 *      per constraint in file order A's terms then B's, then nPublic + 1 entries (0, m + s, s, 1).
 *      A value is coefficient * R^2 mod r, R = 2^256, normal form LE. C's terms are not stored.
 *   5 A, 6 B1, 7 B2 (G2), 8 C, 9 H
 *   10 64 zero bytes, u32 0
 * Every point read is tested on the GPU before any arithmetic (range and curve; all zero bytes
 * pass as infinity in the Lagrange levels): NZCB_ERR_FORMAT "ptau: section <id> point <lowest bad
 * index> ...", the index counted within the section. Levels the setup does not read are not
 * tested. Only the levels used are uploaded.
 *
 * nzcb_groth16_contribute: C and H times 1/d, delta1 and delta2 times d; sections 1, 3-7 and 10
 * are copied. secret: 32 B LE in [1, r) (NZCB_ERR_ARG otherwise), or NULL: d is drawn as
 * nzcb_ptau_contribute draws tau, keccak256(96 bytes of the OS CSPRNG || entropy || 0) mod r,
 * redrawn on zero. A caller-given secret is FOR REPRODUCIBLE TESTS ONLY: whoever knows it can
 * forge proofs. The secret is wiped from host and device memory before the call returns. Every
 * point of sections 8 and 9 ((0, 0) passes) and the two deltas are tested first: NZCB_ERR_FORMAT
 * "zkey: section <id> point <lowest bad index> ...". A zkey whose protocol id is not 1:
 * NZCB_ERR_FORMAT "zkey file is not groth16".
 *
 * The _file forms map their inputs (a prepared power-21 ptau is 2.25 GiB) and write the output
 * path themselves; it must not be an input path. device = NZCB_GROTH16_HOST runs the same steps
 * on the host with up to 16 threads; the bytes are identical.
 *
 * nzcb_groth16_vk_to_json: {"protocol":"groth16","curve":"bn128","nPublic", "vk_alpha_1",
 * "vk_beta_2","vk_gamma_2","vk_delta_2","IC"} in this order, decimal strings, G1 [x, y, "1"], G2
 * [[x0, x1], [y0, y1], ["1", "0"]]. snarkjs's vk_alphabeta_12 IS LEFT OUT: its Fq12 layout cannot
 * be pinned here, and neither snarkjs's verifier nor its Solidity template reads it. Returns 0,
 * or minus the size needed when cap is short (out may be NULL), or the NZCB_ERR_* code of a file
 * that is no Groth16 key, with the message in out as far as cap allows. */
#define NZCB_GROTH16_HOST (-1)
int nzcb_groth16_setup(const uint8_t* r1cs, size_t r1cs_len, const uint8_t* ptau, size_t ptau_len,
                       int device /* >= 0, or NZCB_GROTH16_HOST */, uint8_t** zkey_out, size_t* zkey_len,
                       nzcb_err* err);
int nzcb_groth16_setup_file(const char* r1cs_path, const char* ptau_path, const char* zkey_path, int device,
                            nzcb_err* err);
int nzcb_groth16_contribute(const uint8_t* zkey, size_t len, const uint8_t* secret /* 32 B LE in [1, r), or NULL */,
                            const uint8_t* entropy, size_t entropy_len, int device, uint8_t** zkey_out,
                            size_t* zkey_len, nzcb_err* err);
int nzcb_groth16_contribute_file(const char* in_path, const char* out_path, const uint8_t* secret,
                                 const uint8_t* entropy, size_t entropy_len, int device, nzcb_err* err);
int nzcb_groth16_vk_to_json(const uint8_t* zkey, size_t len, char* out, size_t cap);
/* The same from a file, memory-mapped. */
int nzcb_groth16_vk_to_json_file(const char* zkey_path, char* out, size_t cap);

/* ---- HBM buffers (witnesses for nzcb_prove_device / nzcb_prove_batch on device) ---- */
void* nzcb_dev_alloc(size_t bytes);
/* The same on `device`; the calling thread's current device is left as it was (the N-API
 * addon's per-call threads allocate witness buffers on the witness program's device). */
void* nzcb_dev_alloc_on(int device, size_t bytes);
void nzcb_dev_free(void* p);
int nzcb_memcpy_h2d(void* dst, const void* src, size_t bytes);
int nzcb_memcpy_d2h(void* dst, const void* src, size_t bytes);
int nzcb_memcpy_d2d(void* dst, const void* src, size_t bytes);
/* The same ordered on a HIP stream (no host wait): work enqueued on `stream` afterwards
 * sees the copy (nzcb/msmsplit.py: scalars into the scatter rows on torch's stream). */
int nzcb_memcpy_d2d_async(void* dst, const void* src, size_t bytes, void* stream);

/* ---- Serving side of nzcb_ctx_set_msm_split (one per serving rank) ---------------- */
/* A resident fixed-base MSM table over n device bases (affine LEM, e.g. a PTau range),
 * the prover's shifted-base schedule for PTau (c = 20): the serving ranks of nzcb_ctx_set_msm_split
 * keep one and answer every commitment with one run. out_affine: 64 bytes, x || y normal
 * form LE (infinity = zeros); scalars: `count` <= n 32-byte values in HBM, Montgomery
 * form when scalars_mont (the prover's coefficients). */
typedef struct nzcb_msm_table nzcb_msm_table;
nzcb_msm_table* nzcb_msm_table_create(int device, const void* dev_bases, size_t n, nzcb_err* err);
/* The serving side of the Lagrange-basis commitments (NZCB_MSM_LAGRANGE): the points [lo, hi)
 * of the n + 2-point Lagrange basis of a 2^log_n domain ([L_k(tau)] for k < n, then
 * [tau^n] - [1], [tau^(n+1)] - [tau]), computed on `device` from its PTau (ptau_n >= n + 2
 * affine LEM points in HBM, e.g. a zkey's section 14) by the elliptic-curve inverse NTT the
 * prover runs at context creation, and kept as a table of the Lagrange window and its
 * schedule for small scalars. Scalars passed to nzcb_msm_table_run are the range's slice. */
nzcb_msm_table* nzcb_msm_table_create_lagrange(int device, const void* dev_ptau, size_t ptau_n, int log_n, size_t lo,
                                               size_t hi, nzcb_err* err);
int nzcb_msm_table_run(nzcb_msm_table* t, const void* dev_scalars, size_t count, int scalars_mont,
                       uint8_t* out_affine, nzcb_err* err);
void nzcb_msm_table_destroy(nzcb_msm_table* t);

#ifdef __cplusplus
}
#endif
#ifdef NZCB_WITH_INTERNAL  /* the pre-round-4 declarations (source compatibility) */
#include "nzcb_internal.h"
#endif
#endif
