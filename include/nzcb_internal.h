/*
 * nzcb internal ABI: kernel-level entry points for tests, microbenchmarks and tuning
 * (SURVEY.md §8d config 2). Exported by libnzcb.so next to the product ABI of nzcb.h, but
 * not part of the drop-in boundary and not stable.
 */
#ifndef NZCB_INTERNAL_H
#define NZCB_INTERNAL_H

#include "nzcb.h"

#ifdef __cplusplus
extern "C" {
#endif

/* HIP-event timing of the MSM bucket-accumulation kernel (the dominant kernel):
 * out = {total ms, launches, MSM points, bucket entries} accumulated since the last
 * reset; enable = 1 / 0 turns timing on / off and resets (waiting for the proofs in flight),
 * -1 only reads (without waiting: the totals may include a proof in flight). Timing adds no
 * host synchronisation (the entry count is copied with the MSM's window sums). */
int nzcb_ctx_kernel_stats(nzcb_ctx* ctx, int enable, double out[4]);

/* Guard words (csrc/common.h GuardScope): every device buffer a prover context allocates
 * (proving key, lanes' working sets, MSM and NTT scratch) carries 4 KiB of a known pattern
 * past its end. nzcb_debug_guard_check reads every guard on `device` (-1: all) back: 0
 * when all are intact, NZCB_ERR_INTERNAL with the damaged buffers in err otherwise
 * (checked / damaged: counts). Call it with no proof in flight. nzcb_debug_guard_selftest
 * writes one word past a fresh guarded buffer and checks that exactly that is found. */
int nzcb_debug_guard_check(int device, size_t* checked, int* damaged, nzcb_err* err);
int nzcb_debug_guard_selftest(int device, nzcb_err* err);

/* Fault injection (tests of the prover's own checks): the context's next proof, whichever
 * lane takes it, perturbs its quotient t after round 3 (kind NZCB_FAULT_QUOTIENT: t[1] += 1),
 * which the xi check must report as NZCB_ERR_INTERNAL "quotient check failed". One-shot per
 * context (until round 5 per lane: the lanes that did not take it stayed armed); kind 0
 * clears it. */
#define NZCB_FAULT_QUOTIENT 1
/* Not a fault: kind NZCB_DEBUG_GENERIC_K makes the next proof's grand product form
 * k1 beta w^i and k2 beta w^i by their own Shoup products (the path for k1, k2 other than
 * snarkjs' 2, 3) instead of 2 beta w^i and 3 beta w^i by additions; the proof must be the
 * same. One-shot per context, like the fault. */
#define NZCB_DEBUG_GENERIC_K 2
/* Kind NZCB_FAULT_LANE_ALLOC arms the context's next nzcb_ctx_set_lanes growth instead of a
 * proof: after its first new lane a real device allocation larger than HBM fails (HIP's
 * per-thread last error then holds the out-of-memory code, as after a real failed growth) and
 * the call returns NZCB_ERR_HIP. The rollback must leave lanes() at its old value, the
 * pool consistent and the thread's last error cleared. One-shot. */
#define NZCB_FAULT_LANE_ALLOC 3
int nzcb_debug_inject_fault(nzcb_ctx* ctx, int kind);

/* ---- The signal basis (csrc/sigbasis.h): A, B, C committed over the witness signals ---------- */
/* The expansion of a key's additions gives up, and the context commits from the Lagrange basis,
 * past per_constraint * 3 * nConstraints terms (the library's constant is 64; < 0 restores it).
 * Sets it for the contexts created after the call and returns the previous value. For tests. */
int nzcb_debug_signal_basis_cap(int per_constraint);
/* out[0] = 1 if the context commits A, B, C over the signal basis, [1..3] the rows (signals
 * present) of A, B, C, [4] the points per set in the table (the most rows + 2), [5] the (set,
 * signal, gate) terms of the expansion, [6] the bytes of the signal table. */
int nzcb_debug_signal_basis_info(const nzcb_ctx* ctx, uint64_t out[7]);
/* A, B and C's commitments of a witness (n_witness x 32 B LE normal form, which need not satisfy
 * the circuit) under `blinding` (11 x 32 B, as nzcb_prove_witness) without a proof: out = 3 x 64 B
 * affine LEM. signal_basis = 1: over the signal basis; 0: over the Lagrange basis, the three in one
 * schedule. NZCB_ERR_ARG when the context does not have that path. Runs on lane 0 with no proof
 * in flight. */
int nzcb_debug_commit_abc(nzcb_ctx* ctx, const uint8_t* witness, size_t n_witness, const uint8_t* blinding,
                          int signal_basis, uint8_t* out, nzcb_err* err);
/* The signal basis's rows of set 0, 1, 2 (A, B, C), compacted to the signals that have one:
 * rows_out = info[1 + set] x 64 B affine LEM, signals_out = their signal indices, ascending (cap:
 * the rows both arrays hold). A signal not listed has no row in the set. */
int nzcb_debug_signal_rows(nzcb_ctx* ctx, int set, uint8_t* rows_out, uint32_t* signals_out, size_t cap,
                           nzcb_err* err);

/* The 9x29-bit products of csrc/f29.h as compiled for the device (the generated column asm),
 * over `count` host items of 32-bit limb words (9 per value), for tests against exact
 * integers. op 1: mul_shoup(x, w, ws) (27 words in, 9 out); 2: mul_shoup_x2 (54 / 18);
 * 3: mul29<Fq29>(a, b) (18 / 9); 4: mul29x2<Fr29>(a, b, c, d) (36 / 18); 5: sqr29x2(a, c)
 * (18 / 18); 6: mul2sum29(a, b, c, d) (36 / 9); 7: div2k29(x, K) (10 words in: x, then K in
 * 1..28; 9 out). Synchronous; count <= 2^24. */
int nzcb_debug_f29(int device, int op, const uint32_t* in, size_t count, uint32_t* out, nzcb_err* err);

/* ---- The prover's round 2-5 kernels alone (csrc/prover.hip) ---------------------------------- */
/* Each entry launches the kernels and host helpers the prover launches for that step, on `device`
 * with a stream and buffers of its own, synchronously, and needs no context. Field values are
 * 32-byte LE Montgomery words ("LEM", as nzcb_engine_ntt) in host memory and canonical (below r;
 * NZCB_ERR_ARG otherwise), so a caller chooses the raw words the kernels load. Arrays of several
 * columns are column-major ([k][n]: column k at k * n). At most 2^26 elements per column. */
/* Round 2's grand product (k_perm_tile, k_perm_factors, k_apply_tiles): z_out[i] = prod_{k<i} N_k
 * prod_{k>=i} D_k / prod D over n >= 1 elements, with N_i = (a_i + beta x_i + gamma)(b_i + k1 beta
 * x_i + gamma)(c_i + k2 beta x_i + gamma) and D_i the same over sigma: (a_i + beta s1_i + gamma)(..)
 * (..). x stands in for the prover's table of w^i and may hold any field elements. totals_out: 2
 * words, prod N and prod D as the kernels form them, both times the same power of two (the
 * prover compares them; this entry does not). The k beta x_i are formed by additions when (k1,
 * k2) = (2, 3) and generic_k = 0, else by their own products. prod D = 0 has no defined result. */
int nzcb_debug_grand_product(int device, const uint8_t* abc /* [3][n] */, const uint8_t* sigma /* [3][n] */,
                             const uint8_t* x /* [n] */, size_t n, const uint8_t* beta, const uint8_t* gamma,
                             const uint8_t* k1, const uint8_t* k2, int generic_k, uint8_t* z_out /* [n] */,
                             uint8_t* totals_out /* [2] */, nzcb_err* err);
/* Round 5's divPol1 (the power tables for d, k_lin_tile, k_tile_heads, k_div_check): q_out[i] =
 * p[i + 1] + d q_out[i + 1] for i < m - 1, q_out[m - 1] = 0, m >= 2. *divides_out = 1 when p[0] -
 * p0_adjust = -d q_out[0], else 0: the check that makes a proof fail with NZCB_ERR_DIVPOL. */
int nzcb_debug_div_pol1(int device, const uint8_t* p /* [m] */, size_t m, const uint8_t* d, const uint8_t* p0_adjust,
                        uint8_t* q_out /* [m] */, int* divides_out, nzcb_err* err);
/* Round 4's evaluations (k_eval_pows, k_eval_multi, k_eval_sum): out[j] = polys[j](xs[j]) for np
 * = 1 or 7 polynomials (the two forms the prover runs) of lens[j] >= 1 coefficients each. */
int nzcb_debug_eval_many(int device, int np, const uint8_t* const* polys, const size_t* lens,
                         const uint8_t* xs /* [np] */, uint8_t* out /* [np] */, nzcb_err* err);
/* Round 3's quotient numerator at P points of the domain n = 2^power (power >= 2), point by point:
 *   N = qm a b + ql a + qr b + qo c + qc - sum_j L_j apub_j
 *       + alpha [(a + beta x + gamma)(b + k1 beta x + gamma)(c + k2 beta x + gamma) z
 *                - (a + beta s1 + gamma)(b + beta s2 + gamma)(c + beta s3 + gamma) z(w x)]
 *       + alpha^2 (z - 1) L_0
 * in the kernels' own point order, with w4 the 4n-th root of unity and g = 5. three = 1: P = 3n,
 * index j n + m is x = g w4^(4m + j) and z(w x) is z at j n + (m + 1 mod n); t_out = N
 * (k_beta_xlo when (k1, k2) = (2, 3), k_quotient_coset29<true>; npub <= 8, NZCB_ERR_ARG past it).
 * three = 0: P = 4n, x_i = g w4^i, z(w x) is z at (i + 4) mod 4n; t_out = N / (x^n - 1)
 * (k_quotient_coset29<false> for npub <= 8, the 8x32 k_quotient_coset past it). Inputs are
 * unscaled: the entry applies the context's exponent pre-scaling and builds the point tables.
 * l holds max(npub, 1) columns (L_0 is read with npub = 0 too). */
int nzcb_debug_quotient(int device, int power, int three, uint32_t npub, const uint8_t* abcz /* [4][P] */,
                        const uint8_t* q /* [5][P] */, const uint8_t* s /* [3][P] */,
                        const uint8_t* l /* [max(npub, 1)][P] */, const uint8_t* apub /* [npub] */, const uint8_t* beta,
                        const uint8_t* gamma, const uint8_t* alpha, const uint8_t* k1, const uint8_t* k2,
                        uint8_t* t_out /* [P] */, nzcb_err* err);

/* ---- Synthetic circuit + setup ------- */
/* Builds the seeded synthetic circuit of oracle/synth.py and its snarkjs-0.4
 * PLONK zkey with trapdoor tau (32-byte LE normal) on `device`. Buffers are
 * malloc'ed by the library; free them with nzcb_free. */
int nzcb_synth_setup(int power, int n_public, int n_inputs, uint64_t seed, uint32_t n_constraints,
                     const uint8_t* tau, int device, uint8_t** zkey_out, size_t* zkey_len, uint8_t** wtns_out,
                     size_t* wtns_len, nzcb_err* err);
/* Same with flags: NZCB_SYNTH_FREE_PUBLIC keeps the public signals off every gate but
 * their public-input gate, so any public values satisfy the circuit. The bench's
 * fullProve pipeline writes the nzcp outputs of each pass there (nzcb_nzcp_witness_dev). */
#define NZCB_SYNTH_FREE_PUBLIC 1u
int nzcb_synth_setup_ex(int power, int n_public, int n_inputs, uint64_t seed, uint32_t n_constraints, uint32_t flags,
                        const uint8_t* tau, int device, uint8_t** zkey_out, size_t* zkey_len, uint8_t** wtns_out,
                        size_t* wtns_len, nzcb_err* err);
/* ---- Kernel-level entry points ------------------------------------------------ */
typedef struct nzcb_engine nzcb_engine;
nzcb_engine* nzcb_engine_create(int device, int max_log_ntt, size_t max_msm_points, nzcb_err* err);
void nzcb_engine_destroy(nzcb_engine* e);
/* Host-buffer variants. Field elements are 32-byte LE Montgomery ("LEM", zkey layout). */
int nzcb_engine_ntt(nzcb_engine* e, const uint8_t* in_lem, uint8_t* out_lem, int log_n, int inverse, nzcb_err* err);
/* bases: n x 64-byte LEM affine; scalars: n x 32 B LE (Montgomery if scalars_mont);
 * out: 64-byte affine x||y LE normal (infinity = zeros). */
int nzcb_engine_msm(nzcb_engine* e, const uint8_t* bases_lem, const uint8_t* scalars, size_t n, int scalars_mont,
                    uint8_t* out_affine, nzcb_err* err);
/* The forward transform on the coset c<w> through a per-coset twiddle table (csrc/ntt.h
 * ntt_coset_twiddles, NttIo::tw; the prover's round-3 inputs): builds the table for c (32-byte
 * LEM) at 2^log_n and runs one transform, out[i] = sum_j in[j] (c w^i)^j over the
 * n + fold_len input coefficients (fold_len <= n: those past n are folded in with x^n = c^n,
 * as the prover folds the blinding terms). 1 <= log_n <= the engine's max_log_ntt. */
int nzcb_debug_ntt_coset(nzcb_engine* e, const uint8_t* in_lem, uint8_t* out_lem, int log_n, const uint8_t* c_lem,
                         int fold_len, nzcb_err* err);
/* Device-resident variants for benchmarks (pointers from nzcb_dev_alloc, nzcb.h). */
int nzcb_engine_ntt_dev(nzcb_engine* e, const void* in, void* out, int log_n, int inverse, nzcb_err* err);
int nzcb_engine_msm_dev(nzcb_engine* e, const void* bases, const void* scalars, size_t n, int scalars_mont,
                        uint8_t* out_affine, nzcb_err* err);
/* Average milliseconds per call of `reps` back-to-back device NTTs, timed with HIP
 * events on the engine's stream. */
int nzcb_engine_time_ntt(nzcb_engine* e, const void* in, void* out, int log_n, int inverse, int reps, double* ms,
                         nzcb_err* err);
/* Microbench inputs: n pseudo-random Fr (Montgomery, < 2^253)
 * from `seed`, and [s_i]G1 bases (LEM affine) from Montgomery scalars. Device pointers. */
int nzcb_engine_random_fr(nzcb_engine* e, void* dev_out, size_t n, uint64_t seed, nzcb_err* err);
int nzcb_engine_fixed_base(nzcb_engine* e, const void* dev_scalars_mont, size_t n, void* dev_out, nzcb_err* err);
/* Lagrange-basis SRS (csrc/lagrange.hip): dev_out[k] = [L_k(tau)] for k < 2^log_n, then
 * [tau^n] - [1] and [tau^(n+1)] - [tau], from ptau_n >= 2^log_n + 2 PTau points (LEM affine,
 * device pointers). The prover commits A, B, C from their evaluations with it. */
int nzcb_engine_lagrange_basis(nzcb_engine* e, const void* dev_ptau, size_t ptau_n, int log_n, void* dev_out,
                               nzcb_err* err);
/* Average wall ms per MSM over `reps` (host-synchronised) and the average bucket-
 * accumulation kernel ms (HIP events). */
int nzcb_engine_time_msm(nzcb_engine* e, const void* bases, const void* scalars, size_t n, int scalars_mont, int reps,
                         double* ms, double* acc_ms, nzcb_err* err);
/* Fixed-base schedule (the prover's): builds the shifted-base table of the first
 * n_table bases (the PTau tables' window, c = 20 by default: 2^(20w) multiples, 13 rows), then
 * runs the MSM of the first n. One-shot (table and scratch freed on return); for parity tests. */
int nzcb_engine_msm_fixed_dev(nzcb_engine* e, const void* bases, size_t n_table, const void* scalars, size_t n,
                              int scalars_mont, uint8_t* out_affine, nzcb_err* err);
/* The same with the table's window (16..20, 0 = the PTau tables' default) and schedule:
 * sparse = 1 is the Lagrange-basis table's (device-derived accumulation chunk, log-depth
 * carry trees; msm.hip dyn_chunk), sparse = 0 the dense one (fixed 48-entry chunk). fold = 1
 * builds the table as the prover builds its PTau tables (MsmBaseTable::mont_folded: rows of
 * 2^-256 B_i): the digits are then taken from the scalars' raw 256-bit Montgomery integers m_i
 * and the result is sum (m_i 2^-256 mod r) B_i; it needs scalars_mont = 1 (NZCB_ERR_ARG
 * otherwise). */
int nzcb_engine_msm_table_dev(nzcb_engine* e, const void* bases, size_t n_table, const void* scalars, size_t n,
                              int scalars_mont, int window, int sparse, int fold, uint8_t* out_affine,
                              nzcb_err* err);
/* nzcb_engine_msm_table_dev's dense schedule, and the segment plan it accumulated by (msm.hip
 * msm_seg_scatter_kernel; NZCB_ACC_SEGMENTS): info[0] = 1 if the MSM ran by segments (0: by
 * chunks, nothing else is filled), info[1] = bucket keys, info[2] = segments, info[3] = the
 * segment cap kSegMax. offsets: info[1] + 1 bucket offsets; seg: the segments' first entry, then
 * their lengths, then their buckets, info[2] values each, in plan order. NZCB_ERR_ARG if
 * offsets_cap < info[1] + 1 or seg_cap < 3 * info[2]. */
int nzcb_debug_msm_plan(nzcb_engine* e, const void* bases, size_t n_table, const void* scalars, size_t n,
                        int scalars_mont, int window, int fold, uint32_t* info, uint32_t* offsets, size_t offsets_cap,
                        uint32_t* seg, size_t seg_cap, uint8_t* out_affine, nzcb_err* err);
/* `sets` (1..3) MSMs of n scalars each (device pointers scalars[0..sets)) over ONE Lagrange-window
 * table of the first n_table bases in one schedule (msm.hip msm_enqueue_sets: the prover's A, B,
 * C commitments since round 6); sparse = 0 is the schedule the prover runs by default, sparse = 1
 * the one NZCB_SPARSE=1 selects. out_affine: sets x 64 bytes (n = 0: `sets` infinities). */
int nzcb_engine_msm_sets_dev(nzcb_engine* e, const void* bases, size_t n_table, const void* const* scalars, int sets,
                             size_t n, int scalars_mont, int sparse, uint8_t* out_affine, nzcb_err* err);
/* Per-phase MSM timing (HIP events, average over reps after three warm-up runs):
 * out[0] wall ms, out[1..7] keys, sort, offsets, accumulate, finalize, reduce, sums,
 * out[8] table build ms (fixed_base only), out[9] bucket entries per MSM (nonzero digits),
 * out[10] host ms per MSM from the device results' arrival to the affine result (the
 * window combination on the CPU: the Horner over the window slots), out[11] host ms of the
 * enqueue (kernel launches), out[12] of which the library radix sort's host call (generic
 * schedule). out holds 13 doubles. fixed_base: 0 generic, 1 the PTau tables' schedule, 2 the
 * Lagrange table's (window 17, sparse), 3 window 17 with the dense schedule. */
int nzcb_engine_time_msm2(nzcb_engine* e, const void* bases, const void* scalars, size_t n, int scalars_mont,
                          int fixed_base, int reps, double* out, nzcb_err* err);
/* Field self-test helpers: out[i] = a[i] * b[i] (Montgomery, device), n elements. */
int nzcb_engine_fr_mul(nzcb_engine* e, const uint8_t* a_lem, const uint8_t* b_lem, uint8_t* out_lem, size_t n,
                       int field_q, nzcb_err* err);

/* ---- Batch verification (csrc/verify_batch.hip) -------------------------------------- */
/* Weighted sums of G1 points in groups, on GPU `device` or on the host (NZCB_VERIFY_HOST; the
 * same functions compiled for the host, byte-equal results). Needs no engine or context: own
 * stream and buffers per call. points: n x 64 B (x || y, 32-byte LE normal form, zeros =
 * infinity); scalars: n x 32 B LE normal form, < r; group_end: `groups` exclusive ends,
 * non-decreasing, n = the last one (<= 2^24); out: groups x 64 B, group g = the sum of
 * scalars[i] * points[i] over group_end[g - 1] <= i < group_end[g], in the points' format. */
int nzcb_engine_g1_lincomb(int device, const uint8_t* points, const uint8_t* scalars, const uint32_t* group_end,
                           size_t groups, uint8_t* out, nzcb_err* err);
/* nzcb_verify_batch (nzcb.h) with its intermediate results. points_out (may be NULL): count x
 * 128 B, L'_i || R'_i = rho_i L_i || rho_i R_i (the two pairing inputs of item i under its
 * weight), zeros for items rejected before the sums (malformed, off-curve, wrong n_public).
 * pairing_checks (may be NULL): how many pairing checks the call ran. */
int nzcb_engine_verify_batch(const uint8_t* vk, const uint8_t* proofs, const uint8_t* pubs, size_t pub_stride,
                             int n_public, int count, int transcript_public, int device, const uint8_t* seed,
                             int* valid_out, uint8_t* points_out, int* pairing_checks, nzcb_err* err);
/* Milliseconds of the calling thread's last nzcb_(engine_)verify_batch: [0] host parsing,
 * challenges and weighted scalars, [1] the group sums (wall, with copies), [2] the scalar-
 * multiplication kernel and [3] the group-sum kernel (HIP events; 0 on the host path),
 * [4] the pairing checks with their host sums, [5] the number of pairing checks. Returns the
 * number of values written (cap <= 6). */
int nzcb_debug_verify_batch_timings(double* ms, int cap);

/* ---- Witness check (csrc/r1cs_check.hip) ---------------------------------------------- */
/* nzcb_r1cs_create with the tuning knobs: long_row_threshold (0 = the library's constant) and
 * witness_tile, the most witnesses a lane or wave evaluates per row (0 = the library's, 1; 2 or
 * 4: tiles of that many, then the smaller tiles for what is left of a batch). The outputs are
 * the same for every setting. */
nzcb_r1cs* nzcb_engine_r1cs_create(const uint8_t* r1cs, size_t len, int device, uint32_t long_row_threshold,
                                   int witness_tile, nzcb_err* err);
/* Kernel milliseconds (HIP events) of the calling thread's last nzcb_r1cs_check on a device:
 * [0] the lane-per-row kernel, [1] the wave-per-row kernel, [2] the bitmap collection. Returns
 * the number of values written (cap <= 3). */
int nzcb_debug_r1cs_check_timings(double* ms, int cap);

/* ---- Pass signature (csrc/p256.h, csrc/p256_verify.hip) -------------------------------- */
/* nzcb_p256_key_create with the window width of the fixed-base tables: 4 or 8 (0 = the
 * library's default). The statuses do not depend on it. */
nzcb_p256_key* nzcb_engine_p256_key_create(const uint8_t pub_xy[64], int device, int window, nzcb_err* err);
/* The P-256 field arithmetic as compiled for `device` (or for the host, NZCB_P256_HOST):
 * out[i] = a[i] op b[i] in F_p (field 0) or F_n (field 1), `count` <= 2^24 operands of 32
 * big-endian bytes each in normal form, below the modulus (NZCB_ERR_ARG otherwise); sqr and
 * inv read a only (inv: 0 -> 0). Products go through the Montgomery form and back. */
#define NZCB_P256_OP_ADD 0
#define NZCB_P256_OP_SUB 1
#define NZCB_P256_OP_MUL 2
#define NZCB_P256_OP_SQR 3
#define NZCB_P256_OP_INV 4
int nzcb_debug_p256_field(int device, int op, int field, const uint8_t* a, const uint8_t* b, size_t count,
                          uint8_t* out, nzcb_err* err);
/* out_xy[i] = u1[i] G + u2[i] Q, affine x || y (64 zero bytes for the point at infinity), for
 * the key object's Q, device and window, through the table code the verifier runs. u1, u2:
 * `count` <= 2^24 scalars of 32 big-endian bytes (any 256-bit value). */
int nzcb_debug_p256_mul2(nzcb_p256_key* k, const uint8_t* u1, const uint8_t* u2, size_t count, uint8_t* out_xy,
                         nzcb_err* err);
/* Milliseconds of the calling thread's last calls: [0] the table build of nzcb_p256_key_create
 * (the kernel, HIP events; wall time on the host path), [1] the verify kernel of
 * nzcb_p256_verify (HIP events; 0 on the host path), [2] that call's wall time. Returns the
 * number of values written (cap <= 3). */
int nzcb_debug_p256_timings(double* ms, int cap);

/* ---- Pass decode (csrc/nzcp_decode.h, csrc/nzcp_decode.hip) ----------------------------- */
/* Milliseconds of the calling thread's last nzcb_nzcp_decode: [0] the decode kernel (HIP events;
 * 0 on the host path), [1] the call's wall time. Returns the number of values written (cap <= 2). */
int nzcb_debug_nzcp_decode_timings(double* ms, int cap);

/* ---- Key material check (csrc/key_check.h, csrc/key_check.hip) -------------------------- */
/* The check behind nzcb_ptau_check (nzcb.h) on bare arrays: points = m x 64 B (x || y, LE
 * Montgomery: ptau section 2, zkey section 14), m >= 1; g2 = 128 B, the layout of X_2; seed as
 * there. chunk_points: points per device chunk with the one overlap point (0 = the library's
 * constant, otherwise 2..2^22); the finding does not depend on it. lr_out (may be NULL): L || R
 * of the whole range, affine, 32-byte LE normal form, zeros for infinity or when an earlier
 * step ended the check. */
int nzcb_engine_srs_check(int device, const uint8_t* points, uint64_t m, const uint8_t* g2, const uint8_t* seed,
                          uint32_t chunk_points, nzcb_key_finding* finding, uint8_t* lr_out /* 128 B */,
                          nzcb_err* err);
/* Milliseconds of the calling thread's last key check: [0] the point kernel, [1] the weight
 * kernel, [2] the two MSMs (wall, with their host part), [3] host-to-device copies and the
 * rest of the device pass (wall), [4] the pairing checks on the host, [5] the call, and for a
 * zkey [6] the transforms, [7] the compare kernel, [8] the commitments' MSMs (wall). Kernel
 * times are HIP events; 0 on the host path except [4] and [5]. Returns the number written
 * (cap <= 9). */
int nzcb_debug_key_check_timings(double* ms, int cap);

/* ---- Powers of tau operations (csrc/ptau_ops.h, csrc/ptau_ops.hip) ----------------------- */
/* Milliseconds of the calling thread's last nzcb_ptau_contribute or nzcb_ptau_prepare_phase2:
 * [0] the kernels (HIP events; 0 on the host path), [1] the call's wall time. Returns the number
 * of values written (cap <= 2). */
int nzcb_debug_ptau_timings(double* ms, int cap);
/* The device path of nzcb_ptau_prepare_phase2 transforms the levels 0..batch_top of a section in
 * one run (one launch per stage for all of them) and every larger level in a run of its own, so
 * its work space is that of the top level. Sets batch_top for the calls that follow (the
 * library's constant is 16; level < 0 restores it) and returns the previous value. The bytes do
 * not depend on it. Not thread-safe: for tests. */
int nzcb_debug_ptau_batch_top(int level);

/* ---- Groth16 key generation (csrc/groth16.h, csrc/groth16.hip) --------------------------- */
/* The kernel family behind nzcb_groth16_setup on bare arrays: out[row] = sum over the row's
 * terms t in [row_off[row], row_off[row + 1]) of coefs[t] * points[idx[t]], affine LEM, all zero
 * bytes for the point at infinity. points: n_points LEM affine points, 64 B each (G1) or 128 B
 * with g2 != 0, IN DEVICE MEMORY on `device` (in host memory with device = NZCB_GROTH16_HOST);
 * (0, 0) among them is the point at infinity; they are not tested. row_off: n_rows + 1 ascending
 * offsets from 0; idx below n_points; coefs: 32 B LE normal form below r each (NZCB_ERR_ARG
 * otherwise). out: n_rows points in host memory. Runs under the current schedule (below). */
int nzcb_engine_groth16_rows(int device, int g2, const void* points, uint64_t n_points, const uint64_t* row_off,
                             uint64_t n_rows, const uint32_t* idx, const uint8_t* coefs, uint8_t* out,
                             nzcb_err* err);
/* A row is cut into chunks of at most `chunk` terms (and, past a chunk's first term, at most
 * 4 * chunk expected additions, half a coefficient's bits each), one lane each, and the chunk
 * partials of a row are folded `fan_in` at a time, level by level. Sets both for the calls that follow (the
 * library's constants are 32 and 8; <= 0 restores a constant; chunk <= 1024, 2 <= fan_in <= 1024,
 * NZCB_ERR_ARG otherwise) and writes the previous values (either pointer may be NULL). The bytes
 * do not depend on them. Not thread-safe: for tests. */
int nzcb_debug_groth16_schedule(int chunk, int fan_in, int* prev_chunk, int* prev_fan_in);
/* Of the calling thread's last nzcb_groth16_setup, nzcb_groth16_contribute or
 * nzcb_engine_groth16_rows. Milliseconds: [0] all kernels (HIP events; 0 on the host path), [1]
 * the call's wall time, [2] the G1 rows (A, B1 and K in one run: chunks, folds, store), [3] the
 * G2 rows (B2), [4] the point tests, [5] the scaling of a contribution, [6] the host's reading of
 * the r1cs, transposed lists and schedule (wall). Counts: [7] terms of A, [8] B1, [9] B2, [10] K
 * (zero coefficients included), [11] chunks of the G1 run, [12] of the G2 run. Returns the number
 * of values written (cap <= 13). */
int nzcb_debug_groth16_timings(double* out, int cap);

#ifdef __cplusplus
}
#endif
#endif
