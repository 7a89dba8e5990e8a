"""ctypes binding of ``libnzcb.so`` (the C-ABI in ``include/nzcb.h``).

Host-side mirror of the reference's prover interface for this path
(snarkjs 0.4.12 ``plonk.prove(zkeyFileName, witnessFileName, logger)`` [EXT],
``/root/reference/package.json:18``): ``plonk.prove`` takes a
zkey and a witness (paths or bytes) and returns ``{proof, publicSignals}`` in
snarkjs's decimal-string JSON layout, raising with snarkjs's error text.

The library is the product: there is no CPU fallback. Loading fails loudly when
``lib/libnzcb.so`` has not been built, and every compute call needs a HIP device.
"""
from __future__ import annotations

import ctypes
import json
import os
from ctypes import POINTER, c_char, c_double, c_int, c_size_t, c_uint8, c_uint32, c_uint64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NZCB_LIB", os.path.join(os.path.dirname(_HERE), "lib", "libnzcb.so"))

PROOF_BYTES = 9 * 64 + 7 * 32
BLINDING_BYTES = 11 * 32
VK_BYTES = 8 + 2 * 32 + 8 * 64 + 4 * 32 + 32
PROOF_POINTS = ("A", "B", "C", "Z", "T1", "T2", "T3", "Wxi", "Wxiw")
PROOF_EVALS = ("eval_a", "eval_b", "eval_c", "eval_s1", "eval_s2", "eval_zw", "eval_r")
VK_POINTS = ("Qm", "Ql", "Qr", "Qo", "Qc", "S1", "S2", "S3")

ERROR_NAMES = {
    0: "OK", 1: "ARG", 2: "FORMAT", 3: "NOT_PLONK", 4: "CURVE", 5: "WITNESS_LEN", 6: "COPY",
    7: "T_DIV", 8: "TZ", 9: "DIVPOL", 10: "HIP", 11: "INTERNAL",
}

EXPORTED_SYMBOLS = [
    "nzcb_version", "nzcb_device_count", "nzcb_ctx_create", "nzcb_ctx_destroy", "nzcb_ctx_set_logger",
    "nzcb_ctx_set_transcript_public", "nzcb_ctx_info", "nzcb_prove", "nzcb_prove_witness", "nzcb_prove_device",
    "nzcb_ctx_kernel_stats",
    "nzcb_ctx_last_timings", "nzcb_proof_to_json", "nzcb_public_to_json", "nzcb_synth_setup", "nzcb_free",
    "nzcb_engine_create", "nzcb_engine_destroy", "nzcb_engine_ntt", "nzcb_engine_msm", "nzcb_dev_alloc",
    "nzcb_dev_free", "nzcb_memcpy_h2d", "nzcb_memcpy_d2h", "nzcb_engine_ntt_dev", "nzcb_engine_msm_dev",
    "nzcb_engine_time_ntt", "nzcb_engine_fr_mul", "nzcb_engine_random_fr", "nzcb_engine_fixed_base",
    "nzcb_engine_time_msm", "nzcb_engine_msm_fixed_dev", "nzcb_engine_msm_table_dev", "nzcb_engine_msm_sets_dev", "nzcb_engine_time_msm2", "nzcb_ctx_set_lanes",
    "nzcb_ctx_lanes", "nzcb_prove_batch", "nzcb_vk_from_zkey", "nzcb_vk_from_zkey_file", "nzcb_vk_to_json", "nzcb_verify",
    "nzcb_proof_to_calldata", "nzcb_vk_to_solidity", "nzcb_engine_lagrange_basis", "nzcb_ctx_set_msm_devices", "nzcb_nzcp_input_signals", "nzcb_nzcp_witness",
    "nzcb_nzcp_witness_dev", "nzcb_synth_setup_ex", "nzcb_memcpy_d2d",
    "nzcb_plonk_setup", "nzcb_prove_batch_status", "nzcb_wprog_remap", "nzcb_prove_logged", "nzcb_memcpy_d2d_async",
    "nzcb_debug_guard_check", "nzcb_debug_guard_selftest", "nzcb_debug_inject_fault", "nzcb_debug_f29",
    "nzcb_debug_ntt_coset", "nzcb_debug_msm_plan",
    "nzcb_msm_table_create_lagrange",
    "nzcb_verify_batch", "nzcb_engine_g1_lincomb", "nzcb_engine_verify_batch", "nzcb_debug_verify_batch_timings",
    "nzcb_r1cs_create", "nzcb_r1cs_create_file", "nzcb_r1cs_info", "nzcb_r1cs_check", "nzcb_r1cs_destroy",
    "nzcb_engine_r1cs_create", "nzcb_debug_r1cs_check_timings",
    "nzcb_p256_key_create", "nzcb_p256_verify", "nzcb_p256_key_destroy", "nzcb_engine_p256_key_create",
    "nzcb_debug_p256_field", "nzcb_debug_p256_mul2", "nzcb_debug_p256_timings",
    "nzcb_nzcp_pass_layout", "nzcb_nzcp_decode", "nzcb_nzcp_decode_dev", "nzcb_debug_nzcp_decode_timings",
    "nzcb_ptau_check", "nzcb_ptau_check_file", "nzcb_zkey_check", "nzcb_zkey_check_file", "nzcb_engine_srs_check",
    "nzcb_debug_key_check_timings",
    "nzcb_ptau_new", "nzcb_ptau_new_file", "nzcb_ptau_contribute", "nzcb_ptau_contribute_file",
    "nzcb_ptau_prepare_phase2", "nzcb_ptau_prepare_phase2_file", "nzcb_debug_ptau_timings",
    "nzcb_debug_ptau_batch_top",
    "nzcb_groth16_setup", "nzcb_groth16_setup_file", "nzcb_groth16_contribute", "nzcb_groth16_contribute_file",
    "nzcb_groth16_vk_to_json", "nzcb_groth16_vk_to_json_file", "nzcb_engine_groth16_rows",
    "nzcb_debug_groth16_schedule", "nzcb_debug_groth16_timings",
    "nzcb_debug_signal_basis_cap", "nzcb_debug_signal_basis_info", "nzcb_debug_commit_abc", "nzcb_debug_signal_rows",
    "nzcb_debug_grand_product", "nzcb_debug_div_pol1", "nzcb_debug_eval_many", "nzcb_debug_quotient",
]

NZCB_FAULT_QUOTIENT = 1  # include/nzcb_internal.h
NZCB_DEBUG_GENERIC_K = 2  # include/nzcb_internal.h
NZCB_FAULT_LANE_ALLOC = 3  # include/nzcb_internal.h
VERIFY_HOST = -1  # include/nzcb.h NZCB_VERIFY_HOST: verify_batch with the scalar multiplications on the host
R1CS_HOST = -1  # include/nzcb.h NZCB_R1CS_HOST: the witness check on the host
WITNESS_WTNS, WITNESS_HOST, WITNESS_DEVICE = 0, 1, 2  # include/nzcb.h NZCB_WITNESS_*
P256_HOST = -1  # include/nzcb.h NZCB_P256_HOST: signature verification on the host
SIG_OK, SIG_INVALID, SIG_RANGE = 0, 1, 2  # include/nzcb.h NZCB_SIG_*
NZCP_HOST = -1  # include/nzcb.h NZCB_NZCP_HOST: the pass decode on the host
PASS_MAX_URI = 2048  # include/nzcb.h NZCB_PASS_MAX_URI
PASS_STATUS_NAMES = ("OK", "LENGTH", "PREFIX", "BASE32", "TRUNCATED", "CBOR", "NOT_COSE", "HEADER",
                     "CLAIMS")  # include/nzcb.h NZCB_PASS_*
PASS_HAS_ALG, PASS_HAS_KID, PASS_HAS_ISS, PASS_HAS_NBF, PASS_HAS_EXP, PASS_HAS_CTI, PASS_HAS_SIG = (
    1, 2, 4, 8, 16, 32, 64)  # include/nzcb.h NZCB_PASS_HAS_*
KEY_HOST = -1  # include/nzcb.h NZCB_KEY_HOST: the key material check on the host
PTAU_HOST = -1  # include/nzcb.h NZCB_PTAU_HOST: the powers-of-tau operations on the host
GROTH16_HOST = -1  # include/nzcb.h NZCB_GROTH16_HOST: Groth16 setup and zkey contribute on the host
KEY_STATUS_NAMES = ("OK", "G2", "RANGE", "CURVE", "GENERATOR", "SEQUENCE", "COSETS", "NONCANONICAL", "LAGRANGE",
                    "EVALS", "COMMIT")  # include/nzcb.h NZCB_KEY_*
KEY_PARTS = ("Qm", "Ql", "Qr", "Qo", "Qc", "S1", "S2", "S3")  # nzcb_zkey_check's parts 0..7, then L0, L1, ...
P256_OPS = {"add": 0, "sub": 1, "mul": 2, "sqr": 3, "inv": 4}  # include/nzcb_internal.h NZCB_P256_OP_*


def lagrange_commit_enabled() -> bool:
    """Whether prover contexts commit A, B, C over the Lagrange basis (csrc/prover.hip
    lagrange_commit_enabled: NZCB_LAGRANGE_COMMIT unset or non-zero), which decides whether
    the MSM split has Lagrange-basis ranges (nzcb.msmsplit)."""
    import re
    e = os.environ.get("NZCB_LAGRANGE_COMMIT")
    if e is None:
        return True
    m = re.match(r"\s*[+-]?\d+", e)   # as C's atoi: the leading integer, 0 without one
    return bool(m) and int(m.group()) != 0


def signal_basis_cap(per_constraint: int = -1) -> int:
    """The signal basis's expansion gives up past per_constraint * 3 * nConstraints terms, for the
    contexts created after this call (nzcb_debug_signal_basis_cap; < 0 restores the library's 64).
    Returns the previous value."""
    return load().nzcb_debug_signal_basis_cap(per_constraint)


def guard_check(device: int = -1) -> int:
    """Every guard word past the prover contexts' device buffers on `device` (-1: all) is
    intact; returns how many guards were checked, raises NzcbError listing the damaged
    buffers otherwise (include/nzcb_internal.h nzcb_debug_guard_check)."""
    err, checked, bad = _Err(), c_size_t(0), c_int(0)
    _check(load().nzcb_debug_guard_check(device, ctypes.byref(checked), ctypes.byref(bad), ctypes.byref(err)), err)
    return checked.value


F29_WORDS = {1: (27, 9), 2: (54, 18), 3: (18, 9), 4: (36, 18), 5: (18, 18), 6: (36, 9), 7: (10, 9)}


def f29_check(op: int, words, device: int = 0):
    """Run csrc/f29.h's device product `op` (include/nzcb_internal.h nzcb_debug_f29) over
    items of F29_WORDS[op][0] limb words each; returns the flat list of output words."""
    win, wout = F29_WORDS[op]
    count = len(words) // win
    assert count * win == len(words)
    arr = (c_uint32 * max(1, len(words)))(*words)
    out = (c_uint32 * max(1, count * wout))()
    err = _Err()
    _check(load().nzcb_debug_f29(device, op, arr, count, out, ctypes.byref(err)), err)
    return list(out)[:count * wout]


def debug_grand_product(abc: bytes, sigma: bytes, x: bytes, beta: bytes, gamma: bytes, k1: bytes, k2: bytes,
                        generic_k: bool = False, device: int = 0):
    """Round 2's kernels alone (include/nzcb_internal.h nzcb_debug_grand_product): abc, sigma = 3
    columns of n words, x = n words, all 32-byte LE Montgomery. Returns (z, totals) as bytes."""
    n = len(x) // 32
    assert len(x) == 32 * n and len(abc) == 96 * n and len(sigma) == 96 * n
    z, tot, err = _out(32 * n), _out(64), _Err()
    _check(load().nzcb_debug_grand_product(device, abc, sigma, x, n, beta, gamma, k1, k2, int(generic_k), z, tot,
                                           ctypes.byref(err)), err)
    return bytes(z)[:32 * n], bytes(tot)


def debug_div_pol1(p: bytes, d: bytes, p0_adjust: bytes = bytes(32), device: int = 0):
    """Round 5's divPol1 kernels alone (nzcb_debug_div_pol1) over m = len(p) / 32 coefficients.
    Returns (q, divides): the m quotient words and whether the division check held."""
    m = len(p) // 32
    assert len(p) == 32 * m
    q, ok, err = _out(32 * m), c_int(-1), _Err()
    _check(load().nzcb_debug_div_pol1(device, p, m, d, p0_adjust, q, ctypes.byref(ok), ctypes.byref(err)), err)
    return bytes(q)[:32 * m], bool(ok.value)


def debug_eval_many(polys, xs: bytes, device: int = 0) -> bytes:
    """Round 4's evaluation kernels alone (nzcb_debug_eval_many): polys = 1 or 7 byte strings of
    coefficients, xs = one point each. Returns the evaluations, 32 bytes each."""
    np_ = len(polys)
    assert len(xs) == 32 * np_ and all(len(p) % 32 == 0 for p in polys)
    arr = (ctypes.c_char_p * max(np_, 1))(*polys)
    lens = (c_size_t * max(np_, 1))(*[len(p) // 32 for p in polys])
    out, err = _out(32 * np_), _Err()
    _check(load().nzcb_debug_eval_many(device, np_, arr, lens, xs, out, ctypes.byref(err)), err)
    return bytes(out)[:32 * np_]


def debug_quotient(power: int, three: bool, npub: int, abcz: bytes, q: bytes, s: bytes, l: bytes, apub: bytes,
                   beta: bytes, gamma: bytes, alpha: bytes, k1: bytes, k2: bytes, device: int = 0) -> bytes:
    """Round 3's quotient kernels alone (nzcb_debug_quotient) over P = 3n (three) or 4n points of
    the domain n = 2^power: abcz, q, s, l = 4, 5, 3, max(npub, 1) columns of P words. Returns the
    P words the kernel stores."""
    pts = (3 if three else 4) << power
    assert len(abcz) == 128 * pts and len(q) == 160 * pts and len(s) == 96 * pts
    assert len(l) == 32 * pts * max(npub, 1) and len(apub) == 32 * npub
    out, err = _out(32 * pts), _Err()
    _check(load().nzcb_debug_quotient(device, power, int(three), npub, abcz, q, s, l, apub, beta, gamma, alpha, k1, k2,
                                      out, ctypes.byref(err)), err)
    return bytes(out)[:32 * pts]


def guard_selftest(device: int = 0) -> None:
    """A one-word overrun past a fresh guarded buffer is found, and only it."""
    err = _Err()
    _check(load().nzcb_debug_guard_selftest(device, ctypes.byref(err)), err)


class NzcbError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(msg)
        self.code = code
        self.name = ERROR_NAMES.get(code, str(code))


class _Err(ctypes.Structure):
    _fields_ = [("code", c_int), ("msg", c_char * 256)]


class NzcpParams(ctypes.Structure):
    """NZCPPubIdentity(IsLive, MaxToBeSignedBytes, MaxCborArrayLenVC, MaxCborMapLenVC, ...)."""
    _fields_ = [("is_live", ctypes.c_int32), ("max_tbs_bytes", ctypes.c_int32),
                ("max_array_len_vc", ctypes.c_int32), ("max_map_len_vc", ctypes.c_int32)]


class NzcpRecord(ctypes.Structure):
    _fields_ = [("status", ctypes.c_int32), ("detail", ctypes.c_int32), ("exp", ctypes.c_uint32),
                ("vc_pos", ctypes.c_int32), ("given_len", ctypes.c_int32), ("family_len", ctypes.c_int32),
                ("dob_len", ctypes.c_int32), ("nullifier_len", ctypes.c_int32),
                ("tbs_sha256", c_uint8 * 32), ("nullifier_sha512", c_uint8 * 64), ("nullifier", c_uint8 * 64),
                ("pub", (c_uint8 * 32) * 3)]


class NzcpPass(ctypes.Structure):
    """include/nzcb.h nzcb_nzcp_pass; load() asserts the layout against nzcb_nzcp_pass_layout."""
    _fields_ = [("status", ctypes.c_int32), ("detail", c_uint32), ("version", c_uint32), ("present", c_uint32),
                ("alg", ctypes.c_int32), ("kid_len", c_uint32), ("iss_len", c_uint32), ("cti_len", c_uint32),
                ("sig_len", c_uint32), ("cose_len", c_uint32), ("protected_off", c_uint32),
                ("protected_len", c_uint32), ("payload_off", c_uint32), ("payload_len", c_uint32),
                ("tbs_len", c_uint32), ("fits", c_uint32), ("nbf", c_uint64), ("exp", c_uint64),
                ("kid", c_uint8 * 32), ("cti", c_uint8 * 32), ("iss", c_uint8 * 64), ("sig", c_uint8 * 64),
                ("tbs_sha256", c_uint8 * 32)]


# circuits/nzcp_live.circom / nzcp_example.circom mains
NZCP_LIVE = dict(is_live=1, max_tbs_bytes=351, max_array_len_vc=0, max_map_len_vc=4)
NZCP_EXAMPLE = dict(is_live=0, max_tbs_bytes=314, max_array_len_vc=0, max_map_len_vc=4)

LOG_FN = ctypes.CFUNCTYPE(None, c_void_p, ctypes.c_char_p)
# nzcb_ctx_set_msm_split callbacks (include/nzcb.h)
MSM_SEND_FN = ctypes.CFUNCTYPE(c_int, c_void_p, c_int, c_void_p, c_size_t)
MSM_GATHER_FN = ctypes.CFUNCTYPE(c_int, c_void_p, c_int, POINTER(c_uint8), POINTER(c_uint8))
MSM_LAGRANGE = 0x100   # include/nzcb.h NZCB_MSM_LAGRANGE: the slot's commitment is over the Lagrange basis

class KeyFinding(ctypes.Structure):  # include/nzcb.h nzcb_key_finding
    _fields_ = [("status", ctypes.c_int32), ("pairing_checks", c_uint32), ("index", ctypes.c_uint64),
                ("n_bad", ctypes.c_uint64), ("checked", ctypes.c_uint64)]


_lib = None


def load(path: str | None = None):
    """Load the shared library (raises OSError if it is missing)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    # proof lanes and commitment streams need more than HIP's default 4 hardware queues
    # per process (kernels of independent streams sharing a queue serialise); only
    # effective when the HIP runtime has not been initialised yet in this process
    if os.environ.get("GPU_MAX_HW_QUEUES", "4") == "4":  # unset or HIP's default
        os.environ["GPU_MAX_HW_QUEUES"] = "24"
    lib = ctypes.CDLL(path or LIB_PATH)
    u8p = POINTER(c_uint8)
    sigs = {
        "nzcb_version": (ctypes.c_char_p, []),
        "nzcb_device_count": (c_int, []),
        "nzcb_ctx_create": (c_void_p, [u8p, c_size_t, c_int, POINTER(_Err)]),
        "nzcb_ctx_destroy": (None, [c_void_p]),
        "nzcb_ctx_set_logger": (None, [c_void_p, LOG_FN, c_void_p]),
        "nzcb_ctx_set_transcript_public": (None, [c_void_p, c_int]),
        "nzcb_ctx_info": (c_int, [c_void_p, POINTER(c_uint32)]),
        "nzcb_prove": (c_int, [c_void_p, u8p, c_size_t, u8p, u8p, u8p, c_size_t, POINTER(_Err)]),
        "nzcb_prove_witness": (c_int, [c_void_p, u8p, c_size_t, u8p, u8p, u8p, c_size_t, POINTER(_Err)]),
        "nzcb_prove_device": (c_int, [c_void_p, c_void_p, c_size_t, u8p, u8p, u8p, c_size_t, POINTER(_Err)]),
        "nzcb_prove_logged": (c_int, [c_void_p, c_void_p, c_size_t, c_int, u8p, u8p, u8p, c_size_t, LOG_FN, c_void_p,
                                      POINTER(_Err)]),
        "nzcb_ctx_kernel_stats": (c_int, [c_void_p, c_int, POINTER(c_double)]),
        "nzcb_ctx_set_lanes": (c_int, [c_void_p, c_int, POINTER(_Err)]),
        "nzcb_ctx_set_msm_devices": (c_int, [c_void_p, POINTER(c_int), c_int, POINTER(_Err)]),
        "nzcb_vk_from_zkey": (c_int, [u8p, c_size_t, u8p, POINTER(_Err)]),
        "nzcb_vk_from_zkey_file": (c_int, [ctypes.c_char_p, u8p, POINTER(_Err)]),
        "nzcb_vk_to_json": (c_int, [u8p, ctypes.c_char_p, c_size_t]),
        "nzcb_verify": (c_int, [u8p, u8p, u8p, c_int, c_int, POINTER(c_int), POINTER(_Err)]),
        "nzcb_proof_to_calldata": (c_int, [u8p, u8p, c_int, ctypes.c_char_p, c_size_t]),
        "nzcb_vk_to_solidity": (c_int, [u8p, ctypes.c_char_p, c_int, ctypes.c_char_p, c_size_t]),
        "nzcb_engine_lagrange_basis": (c_int, [c_void_p, c_void_p, c_size_t, c_int, c_void_p, POINTER(_Err)]),
        "nzcb_ctx_lanes": (c_int, [c_void_p]),
        "nzcb_prove_batch": (c_int, [c_void_p, POINTER(c_void_p), c_size_t, c_int, c_int, u8p, u8p, u8p, c_size_t,
                                     POINTER(_Err)]),
        "nzcb_prove_batch_status": (c_int, [c_void_p, POINTER(c_void_p), c_size_t, c_int, c_int, u8p, u8p, u8p,
                                            c_size_t, POINTER(c_int), POINTER(_Err)]),
        "nzcb_ctx_last_timings": (c_int, [c_void_p, POINTER(c_double), c_int]),
        "nzcb_proof_to_json": (c_int, [u8p, ctypes.c_char_p, c_size_t]),
        "nzcb_public_to_json": (c_int, [u8p, c_int, ctypes.c_char_p, c_size_t]),
        "nzcb_synth_setup": (c_int, [c_int, c_int, c_int, c_uint64, c_uint32, u8p, c_int,
                                     POINTER(POINTER(c_uint8)), POINTER(c_size_t),
                                     POINTER(POINTER(c_uint8)), POINTER(c_size_t), POINTER(_Err)]),
        "nzcb_synth_setup_ex": (c_int, [c_int, c_int, c_int, c_uint64, c_uint32, c_uint32, u8p, c_int,
                                        POINTER(POINTER(c_uint8)), POINTER(c_size_t),
                                        POINTER(POINTER(c_uint8)), POINTER(c_size_t), POINTER(_Err)]),
        "nzcb_free": (None, [c_void_p]),
        "nzcb_engine_create": (c_void_p, [c_int, c_int, c_size_t, POINTER(_Err)]),
        "nzcb_engine_destroy": (None, [c_void_p]),
        "nzcb_engine_ntt": (c_int, [c_void_p, u8p, u8p, c_int, c_int, POINTER(_Err)]),
        "nzcb_debug_ntt_coset": (c_int, [c_void_p, u8p, u8p, c_int, u8p, c_int, POINTER(_Err)]),
        "nzcb_engine_msm": (c_int, [c_void_p, u8p, u8p, c_size_t, c_int, u8p, POINTER(_Err)]),
        "nzcb_dev_alloc": (c_void_p, [c_size_t]),
        "nzcb_dev_alloc_on": (c_void_p, [c_int, c_size_t]),
        "nzcb_dev_free": (None, [c_void_p]),
        "nzcb_memcpy_h2d": (c_int, [c_void_p, c_void_p, c_size_t]),
        "nzcb_memcpy_d2h": (c_int, [c_void_p, c_void_p, c_size_t]),
        "nzcb_memcpy_d2d": (c_int, [c_void_p, c_void_p, c_size_t]),
        "nzcb_memcpy_d2d_async": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p]),
        "nzcb_engine_ntt_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, POINTER(_Err)]),
        "nzcb_engine_msm_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_int, u8p, POINTER(_Err)]),
        "nzcb_engine_time_ntt": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, POINTER(c_double),
                                         POINTER(_Err)]),
        "nzcb_engine_fr_mul": (c_int, [c_void_p, u8p, u8p, u8p, c_size_t, c_int, POINTER(_Err)]),
        "nzcb_engine_random_fr": (c_int, [c_void_p, c_void_p, c_size_t, c_uint64, POINTER(_Err)]),
        "nzcb_engine_fixed_base": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p, POINTER(_Err)]),
        "nzcb_engine_time_msm": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_int, c_int, POINTER(c_double),
                                         POINTER(c_double), POINTER(_Err)]),
        "nzcb_engine_msm_fixed_dev": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p, c_size_t, c_int, u8p,
                                              POINTER(_Err)]),
        "nzcb_engine_msm_table_dev": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p, c_size_t, c_int, c_int, c_int,
                                              c_int, u8p, POINTER(_Err)]),
        "nzcb_engine_msm_sets_dev": (c_int, [c_void_p, c_void_p, c_size_t, POINTER(c_void_p), c_int, c_size_t, c_int,
                                             c_int, u8p, POINTER(_Err)]),
        "nzcb_debug_msm_plan": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p, c_size_t, c_int, c_int, c_int,
                                        POINTER(c_uint32), POINTER(c_uint32), c_size_t, POINTER(c_uint32), c_size_t,
                                        u8p, POINTER(_Err)]),
        "nzcb_plonk_setup": (c_int, [ctypes.c_char_p, c_size_t, ctypes.c_char_p, c_size_t, c_int, POINTER(POINTER(c_uint8)),
                                     POINTER(c_size_t), POINTER(_Err)]),
        "nzcb_nzcp_input_signals": (c_size_t, [POINTER(NzcpParams)]),
        "nzcb_nzcp_witness": (c_int, [c_int, POINTER(NzcpParams), u8p, c_int, POINTER(NzcpRecord), POINTER(_Err)]),
        "nzcb_nzcp_witness_dev": (c_int, [c_int, POINTER(NzcpParams), c_void_p, c_int, c_void_p, c_void_p, c_size_t,
                                          c_void_p, POINTER(_Err)]),
        "nzcb_engine_time_msm2": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_int, c_int, c_int,
                                          POINTER(c_double), POINTER(_Err)]),
        "nzcb_ctx_create_devices": (c_void_p, [u8p, c_size_t, POINTER(c_int), c_int, POINTER(_Err)]),
        "nzcb_ctx_devices": (c_int, [c_void_p]),
        "nzcb_ctx_set_msm_split": (c_int, [c_void_p, c_int, c_size_t, c_size_t, MSM_SEND_FN, MSM_GATHER_FN,
                                           c_void_p, POINTER(_Err)]),
        "nzcb_msm_table_create": (c_void_p, [c_int, c_void_p, c_size_t, POINTER(_Err)]),
        "nzcb_msm_table_create_lagrange": (c_void_p, [c_int, c_void_p, c_size_t, c_int, c_size_t, c_size_t,
                                                      POINTER(_Err)]),
        "nzcb_msm_table_run": (c_int, [c_void_p, c_void_p, c_size_t, c_int, u8p, POINTER(_Err)]),
        "nzcb_msm_table_destroy": (None, [c_void_p]),
        "nzcb_ptau_synth": (c_int, [c_int, u8p, c_int, POINTER(POINTER(c_uint8)), POINTER(c_size_t), POINTER(_Err)]),
        "nzcb_wprog_create": (c_void_p, [ctypes.c_char_p, c_size_t, c_int, POINTER(_Err)]),
        "nzcb_wprog_destroy": (None, [c_void_p]),
        "nzcb_wprog_info": (c_int, [c_void_p, POINTER(c_uint32)]),
        "nzcb_wprog_run_dev": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_size_t, POINTER(ctypes.c_int32),
                                       c_void_p, POINTER(_Err)]),
        "nzcb_wprog_run": (c_int, [c_void_p, ctypes.c_char_p, c_int, u8p, POINTER(ctypes.c_int32), POINTER(_Err)]),
        "nzcb_wprog_remap": (c_int, [ctypes.c_char_p, c_size_t, ctypes.c_char_p, c_size_t, ctypes.c_char_p, c_size_t,
                                     POINTER(POINTER(c_uint8)), POINTER(c_size_t), POINTER(c_uint32), POINTER(_Err)]),
        "nzcb_debug_guard_check": (c_int, [c_int, POINTER(c_size_t), POINTER(c_int), POINTER(_Err)]),
        "nzcb_debug_guard_selftest": (c_int, [c_int, POINTER(_Err)]),
        "nzcb_debug_inject_fault": (c_int, [c_void_p, c_int]),
        "nzcb_debug_f29": (c_int, [c_int, c_int, POINTER(c_uint32), c_size_t, POINTER(c_uint32), POINTER(_Err)]),
        "nzcb_verify_batch": (c_int, [u8p, u8p, u8p, c_size_t, c_int, c_int, c_int, c_int, u8p, POINTER(c_int),
                                      POINTER(_Err)]),
        "nzcb_engine_g1_lincomb": (c_int, [c_int, u8p, u8p, POINTER(c_uint32), c_size_t, u8p, POINTER(_Err)]),
        "nzcb_engine_verify_batch": (c_int, [u8p, u8p, u8p, c_size_t, c_int, c_int, c_int, c_int, u8p, POINTER(c_int),
                                             u8p, POINTER(c_int), POINTER(_Err)]),
        "nzcb_debug_verify_batch_timings": (c_int, [POINTER(c_double), c_int]),
        "nzcb_r1cs_create": (c_void_p, [ctypes.c_char_p, c_size_t, c_int, POINTER(_Err)]),
        "nzcb_r1cs_create_file": (c_void_p, [ctypes.c_char_p, c_int, POINTER(_Err)]),
        "nzcb_engine_r1cs_create": (c_void_p, [ctypes.c_char_p, c_size_t, c_int, c_uint32, c_int, POINTER(_Err)]),
        "nzcb_r1cs_info": (c_int, [c_void_p, POINTER(c_uint32)]),
        "nzcb_r1cs_check": (c_int, [c_void_p, c_void_p, c_size_t, c_int, c_int, c_size_t, POINTER(c_uint32),
                                    POINTER(c_uint32), c_uint32, c_void_p, POINTER(_Err)]),
        "nzcb_r1cs_destroy": (None, [c_void_p]),
        "nzcb_debug_r1cs_check_timings": (c_int, [POINTER(c_double), c_int]),
        "nzcb_p256_key_create": (c_void_p, [ctypes.c_char_p, c_int, POINTER(_Err)]),
        "nzcb_engine_p256_key_create": (c_void_p, [ctypes.c_char_p, c_int, c_int, POINTER(_Err)]),
        "nzcb_p256_verify": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p, c_size_t, c_int, c_int,
                                     POINTER(ctypes.c_int32), c_void_p, POINTER(_Err)]),
        "nzcb_p256_key_destroy": (None, [c_void_p]),
        "nzcb_debug_p256_field": (c_int, [c_int, c_int, c_int, ctypes.c_char_p, ctypes.c_char_p, c_size_t, u8p,
                                          POINTER(_Err)]),
        "nzcb_debug_p256_mul2": (c_int, [c_void_p, ctypes.c_char_p, ctypes.c_char_p, c_size_t, u8p, POINTER(_Err)]),
        "nzcb_debug_p256_timings": (c_int, [POINTER(c_double), c_int]),
        "nzcb_nzcp_pass_layout": (None, [POINTER(c_uint32)]),
        "nzcb_nzcp_decode": (c_int, [c_int, ctypes.c_char_p, POINTER(c_uint32), c_int, POINTER(NzcpParams),
                                     ctypes.c_char_p, POINTER(NzcpPass), u8p, u8p, c_size_t, POINTER(_Err)]),
        "nzcb_nzcp_decode_dev": (c_int, [c_int, c_void_p, c_void_p, c_int, POINTER(NzcpParams), c_void_p, c_void_p,
                                         c_void_p, c_void_p, c_size_t, c_void_p, POINTER(_Err)]),
        "nzcb_debug_nzcp_decode_timings": (c_int, [POINTER(c_double), c_int]),
        "nzcb_ptau_check": (c_int, [c_void_p, c_size_t, ctypes.c_uint64, c_int, u8p, POINTER(KeyFinding),
                                    POINTER(_Err)]),
        "nzcb_ptau_check_file": (c_int, [ctypes.c_char_p, ctypes.c_uint64, c_int, u8p, POINTER(KeyFinding),
                                         POINTER(_Err)]),
        "nzcb_zkey_check": (c_int, [c_void_p, c_size_t, c_int, u8p, POINTER(c_int), POINTER(KeyFinding),
                                    POINTER(KeyFinding), c_uint32, POINTER(c_uint32), POINTER(_Err)]),
        "nzcb_zkey_check_file": (c_int, [ctypes.c_char_p, c_int, u8p, POINTER(c_int), POINTER(KeyFinding),
                                         POINTER(KeyFinding), c_uint32, POINTER(c_uint32), POINTER(_Err)]),
        "nzcb_engine_srs_check": (c_int, [c_int, c_void_p, ctypes.c_uint64, u8p, u8p, c_uint32, POINTER(KeyFinding),
                                          u8p, POINTER(_Err)]),
        "nzcb_debug_key_check_timings": (c_int, [POINTER(c_double), c_int]),
        "nzcb_ptau_new": (c_int, [c_int, POINTER(POINTER(c_uint8)), POINTER(c_size_t), POINTER(_Err)]),
        "nzcb_ptau_new_file": (c_int, [c_int, ctypes.c_char_p, POINTER(_Err)]),
        "nzcb_ptau_contribute": (c_int, [c_void_p, c_size_t, u8p, ctypes.c_char_p, c_size_t, c_int,
                                         POINTER(POINTER(c_uint8)), POINTER(c_size_t), POINTER(_Err)]),
        "nzcb_ptau_contribute_file": (c_int, [ctypes.c_char_p, ctypes.c_char_p, u8p, ctypes.c_char_p, c_size_t,
                                              c_int, POINTER(_Err)]),
        "nzcb_ptau_prepare_phase2": (c_int, [c_void_p, c_size_t, c_int, POINTER(POINTER(c_uint8)),
                                             POINTER(c_size_t), POINTER(_Err)]),
        "nzcb_ptau_prepare_phase2_file": (c_int, [ctypes.c_char_p, ctypes.c_char_p, c_int, POINTER(_Err)]),
        "nzcb_debug_ptau_timings": (c_int, [POINTER(c_double), c_int]),
        "nzcb_debug_ptau_batch_top": (c_int, [c_int]),
        "nzcb_groth16_setup": (c_int, [c_void_p, c_size_t, c_void_p, c_size_t, c_int, POINTER(POINTER(c_uint8)),
                                       POINTER(c_size_t), POINTER(_Err)]),
        "nzcb_groth16_setup_file": (c_int, [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, c_int, POINTER(_Err)]),
        "nzcb_groth16_contribute": (c_int, [c_void_p, c_size_t, u8p, ctypes.c_char_p, c_size_t, c_int,
                                            POINTER(POINTER(c_uint8)), POINTER(c_size_t), POINTER(_Err)]),
        "nzcb_groth16_contribute_file": (c_int, [ctypes.c_char_p, ctypes.c_char_p, u8p, ctypes.c_char_p, c_size_t,
                                                 c_int, POINTER(_Err)]),
        "nzcb_groth16_vk_to_json": (c_int, [c_void_p, c_size_t, ctypes.c_char_p, c_size_t]),
        "nzcb_groth16_vk_to_json_file": (c_int, [ctypes.c_char_p, ctypes.c_char_p, c_size_t]),
        "nzcb_engine_groth16_rows": (c_int, [c_int, c_int, c_void_p, ctypes.c_uint64, POINTER(ctypes.c_uint64),
                                             ctypes.c_uint64, POINTER(c_uint32), u8p, u8p, POINTER(_Err)]),
        "nzcb_debug_groth16_schedule": (c_int, [c_int, c_int, POINTER(c_int), POINTER(c_int)]),
        "nzcb_debug_groth16_timings": (c_int, [POINTER(c_double), c_int]),
        "nzcb_debug_signal_basis_cap": (c_int, [c_int]),
        "nzcb_debug_signal_basis_info": (c_int, [c_void_p, POINTER(c_uint64)]),
        "nzcb_debug_commit_abc": (c_int, [c_void_p, u8p, c_size_t, u8p, c_int, u8p, POINTER(_Err)]),
        "nzcb_debug_signal_rows": (c_int, [c_void_p, c_int, u8p, POINTER(c_uint32), c_size_t, POINTER(_Err)]),
        "nzcb_debug_grand_product": (c_int, [c_int, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, c_size_t,
                                             ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, c_int,
                                             u8p, u8p, POINTER(_Err)]),
        "nzcb_debug_div_pol1": (c_int, [c_int, ctypes.c_char_p, c_size_t, ctypes.c_char_p, ctypes.c_char_p, u8p,
                                        POINTER(c_int), POINTER(_Err)]),
        "nzcb_debug_eval_many": (c_int, [c_int, c_int, POINTER(ctypes.c_char_p), POINTER(c_size_t), ctypes.c_char_p,
                                         u8p, POINTER(_Err)]),
        "nzcb_debug_quotient": (c_int, [c_int, c_int, c_int, c_uint32, ctypes.c_char_p, ctypes.c_char_p,
                                        ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p,
                                        ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, u8p,
                                        POINTER(_Err)]),
    }
    lib.missing_symbols = []
    for name, (res, args) in sigs.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            lib.missing_symbols.append(name)
            continue
        fn.restype = res
        fn.argtypes = args
    if "nzcb_nzcp_pass_layout" not in lib.missing_symbols:
        lay = (c_uint32 * 3)()
        lib.nzcb_nzcp_pass_layout(lay)
        if list(lay) != [ctypes.sizeof(NzcpPass), NzcpPass.sig.offset, NzcpPass.tbs_sha256.offset]:
            raise OSError(f"NzcpPass does not mirror nzcb_nzcp_pass: the library reports {list(lay)}")
    _lib = lib
    return lib


def _buf(data: bytes):
    return (c_uint8 * len(data)).from_buffer_copy(data) if data else (c_uint8 * 1)()


def _out(n: int):
    return (c_uint8 * max(n, 1))()


def _check(rc: int, err: _Err):
    if rc != 0:
        raise NzcbError(rc, err.msg.decode(errors="replace"))


def version() -> str:
    return load().nzcb_version().decode()


def device_count() -> int:
    return load().nzcb_device_count()


def nzcp_input_signals(params: dict) -> int:
    """Input signals per pass: toBeSigned[8*MaxToBeSignedBytes], toBeSignedLen, data[160]."""
    return load().nzcb_nzcp_input_signals(ctypes.byref(NzcpParams(**params)))


def _record_dict(r: NzcpRecord) -> dict:
    return {
        "status": r.status, "detail": r.detail, "exp": r.exp, "vc_pos": r.vc_pos, "given_len": r.given_len,
        "family_len": r.family_len, "dob_len": r.dob_len, "nullifier_len": r.nullifier_len,
        "tbs_sha256": bytes(r.tbs_sha256), "nullifier_sha512": bytes(r.nullifier_sha512),
        "nullifier": bytes(r.nullifier), "out": [int.from_bytes(bytes(r.pub[k]), "little") for k in range(3)],
    }


def nzcp_witness(inputs: bytes, count: int, params: dict = NZCP_LIVE, device: int = 0) -> list:
    """NZCPPubIdentity witness on the GPU for `count` passes (include/nzcb.h
    nzcb_nzcp_witness). `inputs`: count x nzcp_input_signals(params) x 32-byte LE field
    elements. Returns one dict per pass (status, detail, exp, vc_pos, lengths,
    tbs_sha256, nullifier_sha512, nullifier, out = the 3 public signals as ints)."""
    lib = load()
    prm = NzcpParams(**params)
    need = lib.nzcb_nzcp_input_signals(ctypes.byref(prm)) * 32 * count
    if len(inputs) != need:
        raise ValueError(f"nzcp inputs are {len(inputs)} bytes, expected {need}")
    recs = (NzcpRecord * max(count, 1))()
    err = _Err()
    _check(lib.nzcb_nzcp_witness(device, ctypes.byref(prm), _buf(inputs), count, recs, ctypes.byref(err)), err)
    return [_record_dict(recs[i]) for i in range(count)]


def nzcp_witness_dev(dev_inputs: int, count: int, params: dict = NZCP_LIVE, device: int = 0,
                     dev_records: int | None = None, dev_witness: int | None = None, witness_stride: int = 0,
                     stream: int | None = None):
    """Device-pointer variant (asynchronous on `stream`); see nzcb_nzcp_witness_dev."""
    lib = load()
    err = _Err()
    _check(lib.nzcb_nzcp_witness_dev(device, ctypes.byref(NzcpParams(**params)), dev_inputs, count, dev_records,
                                     dev_witness, witness_stride, stream, ctypes.byref(err)), err)


def nzcp_records_from_bytes(raw: bytes, count: int) -> list:
    size = ctypes.sizeof(NzcpRecord)
    return [_record_dict(NzcpRecord.from_buffer_copy(raw[i * size:(i + 1) * size])) for i in range(count)]


def _pass_dict(r: NzcpPass) -> dict:
    """A record with its strings cut to their stored bytes: kid, cti, sig as bytes, iss as str. A
    field the pass does not have (its `present` bit is clear) is None."""
    has = lambda bit: bool(r.present & bit)  # noqa: E731
    return {
        "status": r.status, "status_name": PASS_STATUS_NAMES[r.status], "detail": r.detail, "version": r.version,
        "present": r.present, "alg": r.alg if has(PASS_HAS_ALG) else None,
        "kid": bytes(r.kid)[:min(r.kid_len, 32)] if has(PASS_HAS_KID) else None, "kid_len": r.kid_len,
        "iss": bytes(r.iss)[:min(r.iss_len, 64)].decode(errors="replace") if has(PASS_HAS_ISS) else None,
        "iss_len": r.iss_len, "nbf": r.nbf if has(PASS_HAS_NBF) else None,
        "exp": r.exp if has(PASS_HAS_EXP) else None,
        "cti": bytes(r.cti)[:min(r.cti_len, 32)] if has(PASS_HAS_CTI) else None, "cti_len": r.cti_len,
        "sig": bytes(r.sig) if has(PASS_HAS_SIG) else None, "sig_len": r.sig_len, "cose_len": r.cose_len,
        "protected_off": r.protected_off, "protected_len": r.protected_len, "payload_off": r.payload_off,
        "payload_len": r.payload_len, "tbs_len": r.tbs_len, "fits": r.fits, "tbs_sha256": bytes(r.tbs_sha256),
    }


def nzcp_passes_from_bytes(raw: bytes, count: int) -> list:
    size = ctypes.sizeof(NzcpPass)
    return [_pass_dict(NzcpPass.from_buffer_copy(raw[i * size:(i + 1) * size])) for i in range(count)]


def pack_uris(uris):
    """URIs (str or bytes) -> (their bytes back to back, count + 1 offsets as a c_uint32 array)."""
    raw = [u.encode("utf-8", "surrogateescape") if isinstance(u, str) else bytes(u) for u in uris]
    offs, at = [0], 0
    for b in raw:
        at += len(b)
        offs.append(at)
    if at > 1 << 31:
        raise ValueError("more than 2^31 bytes of URIs")
    return b"".join(raw), (c_uint32 * len(offs))(*offs)


def nzcp_decode_raw(uris, params: dict | None = None, data20=None, device: int = 0, want_tbs: int = 0,
                    offsets=None):
    """include/nzcb.h nzcb_nzcp_decode over host buffers -> (record bytes, input bytes or None,
    ToBeSigned bytes at stride want_tbs or None). uris: a list, or the packed bytes with `offsets`
    (count + 1 integers, passed on as they are). data20: count x 20 bytes, or None for zeros."""
    lib = load()
    if offsets is None:
        blob, offs = pack_uris(uris)
    else:
        blob, offs = bytes(uris), (c_uint32 * len(offsets))(*offsets)
    count = len(offs) - 1
    if data20 is not None:
        data20 = b"".join(data20) if isinstance(data20, (list, tuple)) else bytes(data20)
        if len(data20) != 20 * count:
            raise ValueError("data is 20 bytes per pass")
    prm = NzcpParams(**params) if params else None
    recs = (NzcpPass * max(count, 1))()
    inputs = _out(lib.nzcb_nzcp_input_signals(ctypes.byref(prm)) * 32 * count) if prm else None
    tbs = _out(want_tbs * count) if want_tbs else None
    err = _Err()
    _check(lib.nzcb_nzcp_decode(device, blob, offs, count, ctypes.byref(prm) if prm else None, data20, recs, inputs,
                                tbs, want_tbs, ctypes.byref(err)), err)
    size = ctypes.sizeof(NzcpPass)
    return (bytes(recs)[:size * count],
            bytes(inputs)[:lib.nzcb_nzcp_input_signals(ctypes.byref(prm)) * 32 * count] if prm else None,
            bytes(tbs)[:want_tbs * count] if want_tbs else None)


def nzcp_decode(uris, params: dict | None = None, data20=None, device: int = 0):
    """Pass URIs -> one dict per pass (include/nzcb.h nzcb_nzcp_pass: status, status_name, detail,
    version, alg, kid, iss, nbf, exp, cti, sig, the lengths and offsets, tbs_len, tbs_sha256, fits;
    absent fields None), decoded on GPU `device` or on the host (NZCP_HOST). With `params`
    (NZCP_LIVE, NZCP_EXAMPLE) returns (dicts, inputs): pass i's input signals for nzcp_witness /
    WitnessProgram.run at inputs[i * nzcp_input_signals(params) * 32:], zeros where fits = 0."""
    uris = list(uris)
    recs, inputs, _ = nzcp_decode_raw(uris, params, data20, device)
    out = nzcp_passes_from_bytes(recs, len(uris))
    return (out, inputs) if params else out


def nzcp_decode_dev(dev_uris: int, dev_offsets: int, count: int, dev_passes: int, params: dict | None = None,
                    dev_data20: int | None = None, dev_inputs: int | None = None, dev_tbs: int | None = None,
                    tbs_stride: int = 0, device: int = 0, stream: int | None = None):
    """Device-pointer variant, asynchronous on `stream`; see nzcb_nzcp_decode_dev. dev_passes takes
    count x sizeof(NzcpPass) bytes (nzcp_passes_from_bytes reads them once copied down); record i's
    sig and tbs_sha256 are where P256Key.verify_dev reads them with stride sizeof(NzcpPass)."""
    lib = load()
    err = _Err()
    prm = NzcpParams(**params) if params else None
    _check(lib.nzcb_nzcp_decode_dev(device, dev_uris, dev_offsets, count, ctypes.byref(prm) if prm else None,
                                    dev_data20, dev_passes, dev_inputs, dev_tbs, tbs_stride, stream,
                                    ctypes.byref(err)), err)


def nzcp_decode_timings() -> list:
    """Milliseconds of this thread's last nzcp_decode: the kernel, the call."""
    ms = (c_double * 2)()
    n = load().nzcb_debug_nzcp_decode_timings(ms, 2)
    return list(ms)[:n]


class Engine:
    """Kernel-level access (NTT, MSM, field mul) for tests and microbenchmarks."""

    def __init__(self, device: int = 0, max_log_ntt: int = 12, max_msm_points: int = 1 << 12):
        self.lib = load()
        err = _Err()
        self.h = self.lib.nzcb_engine_create(device, max_log_ntt, max_msm_points, ctypes.byref(err))
        if not self.h:
            raise NzcbError(err.code, err.msg.decode(errors="replace"))

    def close(self):
        if self.h:
            self.lib.nzcb_engine_destroy(self.h)
            self.h = None

    __del__ = close

    def ntt(self, data_lem: bytes, log_n: int, inverse: bool = False) -> bytes:
        n = 1 << log_n
        assert len(data_lem) == 32 * n
        out = _out(32 * n)
        err = _Err()
        _check(self.lib.nzcb_engine_ntt(self.h, _buf(data_lem), out, log_n, int(inverse), ctypes.byref(err)), err)
        return bytes(out)

    def ntt_coset(self, data_lem: bytes, log_n: int, c_lem: bytes) -> bytes:
        """The forward transform on the coset c<w> through a per-coset twiddle table
        (include/nzcb_internal.h nzcb_debug_ntt_coset): 2^log_n + fold coefficients in, the
        fold <= 2^log_n ones past 2^log_n folded in with x^n = c^n; 2^log_n evaluations out."""
        n = 1 << log_n
        fold = len(data_lem) // 32 - n
        assert len(data_lem) == 32 * (n + fold) and fold >= 0 and len(c_lem) == 32
        out = _out(32 * n)
        err = _Err()
        _check(self.lib.nzcb_debug_ntt_coset(self.h, _buf(data_lem), out, log_n, _buf(c_lem), fold,
                                             ctypes.byref(err)), err)
        return bytes(out)

    def msm(self, bases_lem: bytes, scalars: bytes, scalars_mont: bool = False) -> bytes:
        n = len(scalars) // 32
        assert len(bases_lem) == 64 * n
        out = _out(64)
        err = _Err()
        _check(self.lib.nzcb_engine_msm(self.h, _buf(bases_lem), _buf(scalars), n, int(scalars_mont), out,
                                        ctypes.byref(err)), err)
        return bytes(out)

    def field_mul(self, a_lem: bytes, b_lem: bytes, field_q: bool = False) -> bytes:
        n = len(a_lem) // 32
        out = _out(32 * n)
        err = _Err()
        _check(self.lib.nzcb_engine_fr_mul(self.h, _buf(a_lem), _buf(b_lem), out, n, int(field_q),
                                           ctypes.byref(err)), err)
        return bytes(out)

    def time_ntt(self, dev_in: int, dev_out: int, log_n: int, inverse: bool, reps: int) -> float:
        ms = c_double()
        err = _Err()
        _check(self.lib.nzcb_engine_time_ntt(self.h, dev_in, dev_out, log_n, int(inverse), reps, ctypes.byref(ms),
                                             ctypes.byref(err)), err)
        return ms.value

    def random_fr(self, dev_out: int, n: int, seed: int):
        err = _Err()
        _check(self.lib.nzcb_engine_random_fr(self.h, dev_out, n, seed, ctypes.byref(err)), err)

    def fixed_base(self, dev_scalars: int, n: int, dev_out: int):
        err = _Err()
        _check(self.lib.nzcb_engine_fixed_base(self.h, dev_scalars, n, dev_out, ctypes.byref(err)), err)

    def lagrange_basis(self, dev_ptau: int, ptau_n: int, log_n: int, dev_out: int):
        """dev_out[k] = [L_k(tau)] (k < 2^log_n), then [tau^n] - [1], [tau^(n+1)] - [tau]."""
        err = _Err()
        _check(self.lib.nzcb_engine_lagrange_basis(self.h, dev_ptau, ptau_n, log_n, dev_out, ctypes.byref(err)), err)

    def time_msm(self, dev_bases: int, dev_scalars: int, n: int, scalars_mont: bool, reps: int):
        ms = c_double()
        acc = c_double()
        err = _Err()
        _check(self.lib.nzcb_engine_time_msm(self.h, dev_bases, dev_scalars, n, int(scalars_mont), reps,
                                             ctypes.byref(ms), ctypes.byref(acc), ctypes.byref(err)), err)
        return ms.value, acc.value

    MSM_PHASES = ("keys", "sort", "offsets", "accumulate", "finalize", "reduce", "sums")

    def time_msm_phases(self, dev_bases: int, dev_scalars: int, n: int, scalars_mont: bool, fixed_base: bool,
                        reps: int) -> dict:
        """Wall ms per MSM and HIP-event ms per phase (generic or fixed-base schedule)."""
        out = (c_double * 13)()
        err = _Err()
        _check(self.lib.nzcb_engine_time_msm2(self.h, dev_bases, dev_scalars, n, int(scalars_mont), int(fixed_base),
                                              reps, out, ctypes.byref(err)), err)
        d = {"wall": out[0], "table_build": out[8], "entries": out[9]}
        d.update({k: out[1 + i] for i, k in enumerate(self.MSM_PHASES)})
        d["host_finish"] = out[10]
        d["host_enqueue"] = out[11]     # host time, overlapping the device phases
        d["host_sort_call"] = out[12]
        return d

    def msm_fixed_dev(self, dev_bases: int, n_table: int, dev_scalars: int, n: int, scalars_mont: bool,
                      window: int = 0, sparse: bool = False, fold: bool = False) -> bytes:
        """Fixed-base (shifted-table) MSM of the first n of n_table device bases; window 0 = the
        PTau tables' default, sparse = the Lagrange table's schedule (msm.hip dyn_chunk), fold =
        the prover's 2^-256-folded PTau table: the scalars' raw Montgomery integers m_i are the
        digit source and the result is sum (m_i 2^-256 mod r) B_i (needs scalars_mont)."""
        out = _out(64)
        err = _Err()
        if window or sparse or fold:
            _check(self.lib.nzcb_engine_msm_table_dev(self.h, dev_bases, n_table, dev_scalars, n, int(scalars_mont),
                                                      int(window), int(sparse), int(fold), out, ctypes.byref(err)),
                   err)
        else:
            _check(self.lib.nzcb_engine_msm_fixed_dev(self.h, dev_bases, n_table, dev_scalars, n, int(scalars_mont),
                                                      out, ctypes.byref(err)), err)
        return bytes(out)

    def msm_plan(self, dev_bases: int, n_table: int, dev_scalars: int, n: int, scalars_mont: bool, window: int = 0,
                 fold: bool = False):
        """msm_fixed_dev's dense MSM together with the segment plan it accumulated by
        (include/nzcb_internal.h nzcb_debug_msm_plan): (result, plan), plan = None when the MSM ran
        in chunks (NZCB_ACC_SEGMENTS=0), else a dict of seg_max and the lists offsets (buckets + 1),
        start, len and bucket of the segments in plan order."""
        c = window or 20
        off_cap = (1 << (c - 1)) + 1
        seg_cap = 3 * (n * ((255 + c - 1) // c) + 1)
        info, off, seg = (c_uint32 * 4)(), (c_uint32 * off_cap)(), (c_uint32 * seg_cap)()
        out = _out(64)
        err = _Err()
        _check(self.lib.nzcb_debug_msm_plan(self.h, dev_bases, n_table, dev_scalars, n, int(scalars_mont), int(window),
                                            int(fold), info, off, off_cap, seg, seg_cap, out, ctypes.byref(err)), err)
        if not info[0]:
            return bytes(out), None
        nk, ns = info[1], info[2]
        return bytes(out), {"seg_max": info[3], "offsets": off[:nk + 1], "start": seg[:ns], "len": seg[ns:2 * ns],
                            "bucket": seg[2 * ns:3 * ns]}

    def msm_sets_dev(self, dev_bases: int, n_table: int, dev_scalars: list, n: int, scalars_mont: bool, *,
                     sparse: bool) -> list:
        """len(dev_scalars) (1..3) MSMs of n scalars over one Lagrange-window table in one schedule
        (the prover's A, B, C commitments): one 64-byte affine result per set. sparse=False is the
        schedule the prover runs by default, sparse=True the one NZCB_SPARSE=1 selects."""
        k = len(dev_scalars)
        out = _out(64 * k)
        err = _Err()
        arr = (c_void_p * k)(*dev_scalars)
        _check(self.lib.nzcb_engine_msm_sets_dev(self.h, dev_bases, n_table, arr, k, n, int(scalars_mont),
                                                 int(bool(sparse)), out, ctypes.byref(err)), err)
        return [bytes(out)[64 * i:64 * i + 64] for i in range(k)]

    def msm_dev(self, dev_bases: int, dev_scalars: int, n: int, scalars_mont: bool) -> bytes:
        out = _out(64)
        err = _Err()
        _check(self.lib.nzcb_engine_msm_dev(self.h, dev_bases, dev_scalars, n, int(scalars_mont), out,
                                            ctypes.byref(err)), err)
        return bytes(out)

    # The batch verifier's entries (include/nzcb_internal.h) take a device, not an engine.
    @staticmethod
    def g1_lincomb(points: bytes, scalars: bytes, group_end, device: int = 0) -> list:
        """Per group the sum of scalars[i] * points[i] (nzcb_engine_g1_lincomb): points n x 64 B
        affine LE normal form (zeros = infinity), scalars n x 32 B LE, group_end the groups'
        exclusive ends; device = VERIFY_HOST runs the host path. Returns one 64-byte point per group."""
        groups = len(group_end)
        n = group_end[-1] if groups else 0
        assert len(points) == 64 * n and len(scalars) == 32 * n
        ends = (c_uint32 * max(groups, 1))(*group_end)
        out = _out(64 * groups)
        err = _Err()
        _check(load().nzcb_engine_g1_lincomb(device, _buf(points), _buf(scalars), ends, groups, out,
                                             ctypes.byref(err)), err)
        return [bytes(out)[64 * g:64 * g + 64] for g in range(groups)]

    @staticmethod
    def verify_batch(vk: bytes, proofs, publics, transcript_public: bool = True, device: int = 0,
                     seed: bytes | None = None, n_public: int | None = None):
        """nzcb_engine_verify_batch: (verdicts, per-item L' || R' points (128 B each, zeros for
        items rejected before the sums), number of pairing checks)."""
        count = len(proofs)
        assert len(publics) == count and all(len(p) == PROOF_BYTES for p in proofs)
        if n_public is None:
            n_public = len(publics[0]) // 32 if count else 0
        stride = max([32 * n_public] + [len(p) for p in publics])
        pubs = b"".join(bytes(p).ljust(stride, b"\0") for p in publics)
        assert seed is None or len(seed) == 32
        valid = (c_int * max(count, 1))()
        pts = _out(128 * count)
        checks = c_int(0)
        err = _Err()
        _check(load().nzcb_engine_verify_batch(_buf(vk), _buf(b"".join(proofs)), _buf(pubs), stride, n_public, count,
                                               int(transcript_public), device, _buf(seed) if seed else None, valid,
                                               pts, ctypes.byref(checks), ctypes.byref(err)), err)
        raw = bytes(pts)
        return ([bool(valid[i]) for i in range(count)], [raw[128 * i:128 * i + 128] for i in range(count)],
                checks.value)

    @staticmethod
    def verify_batch_timings() -> list:
        """Milliseconds of this thread's last verify_batch (nzcb_debug_verify_batch_timings)."""
        ms = (c_double * 6)()
        k = load().nzcb_debug_verify_batch_timings(ms, 6)
        return list(ms)[:k]

    @staticmethod
    def srs_check(points: bytes, g2: bytes, device: int = 0, seed: bytes | None = None, chunk_points: int = 0):
        """nzcb_engine_srs_check: (finding, L || R of the whole range, 128 B) for m x 64-byte LEM points
        against the 128-byte G2 point; device = KEY_HOST runs the host path."""
        assert len(points) % 64 == 0 and len(g2) == 128 and (seed is None or len(seed) == 32)
        f = KeyFinding()
        lr = _out(128)
        err = _Err()
        _check(load().nzcb_engine_srs_check(device, ctypes.cast(_buf(points), c_void_p), len(points) // 64, _buf(g2),
                                            _buf(seed) if seed else None, chunk_points, ctypes.byref(f), lr,
                                            ctypes.byref(err)), err)
        return _finding_dict(f), bytes(lr)

    @staticmethod
    def key_check_timings() -> list:
        """Milliseconds of this thread's last key check (nzcb_debug_key_check_timings)."""
        ms = (c_double * 9)()
        k = load().nzcb_debug_key_check_timings(ms, 9)
        return list(ms)[:k]


def dev_alloc(nbytes: int) -> int:
    p = load().nzcb_dev_alloc(nbytes)
    if not p:
        raise NzcbError(10, "hipMalloc failed")
    return p


def dev_free(p: int):
    load().nzcb_dev_free(p)


def h2d(dst: int, data: bytes):
    buf = ctypes.create_string_buffer(data, len(data))
    rc = load().nzcb_memcpy_h2d(dst, buf, len(data))
    if rc:
        raise NzcbError(rc, "h2d failed")


def memcpy_h2d_ptr(dst: int, src_addr: int, nbytes: int):
    """Host memory at a raw address (e.g. inside a library-owned zkey buffer) -> device."""
    rc = load().nzcb_memcpy_h2d(dst, src_addr, nbytes)
    if rc:
        raise NzcbError(rc, "h2d failed")


def d2d(dst: int, src: int, nbytes: int):
    if load().nzcb_memcpy_d2d(dst, src, nbytes) != 0:
        raise NzcbError(10, "hipMemcpy D2D failed")


def d2d_async(dst: int, src: int, nbytes: int, stream: int):
    """Device copy ordered on HIP stream `stream` (no host wait)."""
    if load().nzcb_memcpy_d2d_async(dst, src, nbytes, stream) != 0:
        raise NzcbError(10, "hipMemcpyAsync D2D failed")


def d2h(src: int, nbytes: int) -> bytes:
    buf = ctypes.create_string_buffer(nbytes)
    rc = load().nzcb_memcpy_d2h(buf, src, nbytes)
    if rc:
        raise NzcbError(rc, "d2h failed")
    return buf.raw


def _read(x) -> bytes:
    """snarkjs accepts a file name or {type: "mem", data}; here: path, bytes or {"type": "mem", "data": ...}."""
    if isinstance(x, (bytes, bytearray, memoryview)):
        return bytes(x)
    if isinstance(x, dict) and x.get("type") == "mem":
        return bytes(x["data"])
    with open(x, "rb") as f:
        return f.read()


class ProverContext:
    """A zkey uploaded once to one GPU (``nzcb_ctx_create``); prove many witnesses against it."""

    def __init__(self, zkey, device: int = 0, logger=None, transcript_public: bool = True, _raw=None,
                 devices=None):
        """devices: a device set (nzcb_ctx_create_devices): batches spread over all of them,
        single proofs run on devices[0]."""
        self.lib = load()
        self.devices = list(devices) if devices else [device]
        self.device = self.devices[0]
        err = _Err()
        vk = _out(VK_BYTES)
        if _raw is not None:            # (pointer, length) owned by the caller: no host copy
            zptr, zlen = ctypes.cast(_raw[0], POINTER(c_uint8)), _raw[1]
        else:
            data = _read(zkey)
            zptr, zlen = _buf(data), len(data)
        if len(self.devices) > 1:
            devs = (c_int * len(self.devices))(*self.devices)
            self.h = self.lib.nzcb_ctx_create_devices(zptr, zlen, devs, len(self.devices), ctypes.byref(err))
        else:
            self.h = self.lib.nzcb_ctx_create(zptr, zlen, self.device, ctypes.byref(err))
        if not self.h:
            raise NzcbError(err.code, err.msg.decode(errors="replace"))
        verr = _Err()
        _check(self.lib.nzcb_vk_from_zkey(zptr, zlen, vk, ctypes.byref(verr)), verr)
        self.vk = bytes(vk)  # binary verification key (nzcb.verify / vk_to_json)
        info = (c_uint32 * 5)()
        self.lib.nzcb_ctx_info(self.h, info)
        self.domain_size, self.n_public, self.n_vars, self.n_additions, self.n_constraints = list(info)
        self._logcb = None
        if logger is not None:
            self.set_logger(logger)
        if not transcript_public:
            self.lib.nzcb_ctx_set_transcript_public(self.h, 0)

    def set_logger(self, logger):
        fn = getattr(logger, "debug", logger)
        self._logcb = LOG_FN(lambda _u, m: fn(m.decode()))
        self.lib.nzcb_ctx_set_logger(self.h, self._logcb, None)

    def close(self):
        if getattr(self, "h", None):
            self.lib.nzcb_ctx_destroy(self.h)
            self.h = None

    __del__ = close

    def prove_raw(self, wtns, blinding: bytes | None = None):
        """Returns (proof_bytes, public_bytes) in the C-ABI layout. blinding None draws
        random scalars (snarkjs Fr.random(), zero-knowledge); pass fixed bytes, e.g.
        bytes(352), only for reproducible test proofs."""
        data = _read(wtns)
        proof = _out(PROOF_BYTES)
        pub = _out(32 * self.n_public)
        err = _Err()
        bl = _buf(blinding) if blinding is not None else None
        if blinding is not None and len(blinding) != BLINDING_BYTES:
            raise ValueError("blinding must be 11 x 32 bytes")
        _check(self.lib.nzcb_prove(self.h, _buf(data), len(data), bl, proof, pub, 32 * self.n_public,
                                   ctypes.byref(err)), err)
        return bytes(proof), bytes(pub)[:32 * self.n_public]

    def prove_witness_raw(self, witness_le: bytes, blinding: bytes | None = None):
        n = len(witness_le) // 32
        proof = _out(PROOF_BYTES)
        pub = _out(32 * self.n_public)
        err = _Err()
        bl = _buf(blinding) if blinding is not None else None
        _check(self.lib.nzcb_prove_witness(self.h, _buf(witness_le), n, bl, proof, pub, 32 * self.n_public,
                                           ctypes.byref(err)), err)
        return bytes(proof), bytes(pub)[:32 * self.n_public]

    def prove_device_raw(self, dev_witness: int, n_witness: int, blinding: bytes | None = None):
        """Witness already resident in HBM (device pointer, normal-form LE values)."""
        proof = _out(PROOF_BYTES)
        pub = _out(32 * self.n_public)
        err = _Err()
        bl = _buf(blinding) if blinding is not None else None
        _check(self.lib.nzcb_prove_device(self.h, dev_witness, n_witness, bl, proof, pub, 32 * self.n_public,
                                          ctypes.byref(err)), err)
        return bytes(proof), bytes(pub)[:32 * self.n_public]

    def set_lanes(self, lanes: int):
        """Proofs kept in flight by prove_batch (extra lanes share the resident proving key)."""
        err = _Err()
        _check(self.lib.nzcb_ctx_set_lanes(self.h, lanes, ctypes.byref(err)), err)

    def set_msm_devices(self, devices):
        """Split each commitment MSM over these devices (first = the context's device)."""
        arr = (c_int * len(devices))(*devices)
        err = _Err()
        _check(self.lib.nzcb_ctx_set_msm_devices(self.h, arr, len(devices), ctypes.byref(err)), err)

    def set_msm_split(self, world: int, own_points: int, send, gather, own_lagrange: int = 0):
        """Split every commitment MSM across ranks (nzcb_ctx_set_msm_split; nzcb.msmsplit
        builds the callbacks): rank 0 keeps PTau points [0, own_points) and, when
        own_lagrange > 0, Lagrange-basis points [0, own_lagrange) of A, B and C (their slot
        carries MSM_LAGRANGE). send(slot, dev_ptr, count) -> None; gather(slot, own64) ->
        world x 64 bytes. world = 1 restores the local schedule."""
        if world <= 1:
            self._split_cbs = None
            _check(self.lib.nzcb_ctx_set_msm_split(self.h, 1, 0, 0, MSM_SEND_FN(), MSM_GATHER_FN(), None,
                                                   ctypes.byref(_Err())), _Err())
            return

        def _send(_u, slot, ptr, count):
            try:
                send(slot, ptr, count)
                return 0
            except Exception:  # reported through the proof's error
                import traceback
                traceback.print_exc()
                return 1

        def _gather(_u, slot, own, out):
            try:
                parts = gather(slot, ctypes.string_at(own, 64))
                if len(parts) != 64 * world:
                    return 1
                ctypes.memmove(out, parts, len(parts))
                return 0
            except Exception:
                import traceback
                traceback.print_exc()
                return 1

        self._split_cbs = (MSM_SEND_FN(_send), MSM_GATHER_FN(_gather))  # keep alive
        err = _Err()
        _check(self.lib.nzcb_ctx_set_msm_split(self.h, world, own_points, own_lagrange, self._split_cbs[0],
                                               self._split_cbs[1], None, ctypes.byref(err)), err)

    @property
    def lanes(self) -> int:
        return self.lib.nzcb_ctx_lanes(self.h)

    def prove_batch_raw(self, witnesses, n_witness: int | None = None, blindings=None, on_device: bool = False,
                        statuses: list | None = None):
        """Independent proofs over the lanes. witnesses: list of bytes (host) or device
        pointers (on_device). blindings: list of 352-byte values / None. Returns [(proof, pub)].
        With a `statuses` list, a failed proof does not stop the batch: the list receives
        each item's error code (0 = proved; a failed item's bytes are zero) and nothing is
        raised (nzcb_prove_batch_status)."""
        count = len(witnesses)
        keep = []
        ptrs = (c_void_p * max(count, 1))()
        for i, w in enumerate(witnesses):
            if on_device:
                ptrs[i] = w
            else:
                b = _buf(w)
                keep.append(b)
                ptrs[i] = ctypes.cast(b, c_void_p).value
                if n_witness is None:
                    n_witness = len(w) // 32
        bl = None
        if blindings is not None:
            # an item without blinding gets fresh random scalars (snarkjs Fr.random()), never zeros
            bl = _buf(b"".join(x if x is not None else random_blinding() for x in blindings))
        proofs = _out(PROOF_BYTES * count)
        stride = 32 * max(self.n_public, 1)
        pubs = _out(stride * count)
        err = _Err()
        if statuses is None:
            _check(self.lib.nzcb_prove_batch(self.h, ptrs, n_witness or 0, count, int(on_device), bl, proofs, pubs,
                                             stride, ctypes.byref(err)), err)
        else:
            st = (c_int * max(count, 1))()
            rc = self.lib.nzcb_prove_batch_status(self.h, ptrs, n_witness or 0, count, int(on_device), bl, proofs,
                                                  pubs, stride, st, ctypes.byref(err))
            if rc and not any(st[i] for i in range(count)):  # argument errors, before any proof
                _check(rc, err)
            statuses[:] = [st[i] for i in range(count)]
        P, Q = bytes(proofs), bytes(pubs)
        return [(P[i * PROOF_BYTES:(i + 1) * PROOF_BYTES], Q[i * stride:i * stride + 32 * self.n_public])
                for i in range(count)]

    def inject_fault(self, kind: int = NZCB_FAULT_QUOTIENT) -> None:
        """The next proof on each lane perturbs its quotient t (NZCB_FAULT_QUOTIENT: tests of
        the xi check) or takes the grand product's generic k1, k2 path (NZCB_DEBUG_GENERIC_K:
        the same proof), or the next set_lanes growth fails after one new lane
        (NZCB_FAULT_LANE_ALLOC: tests of the rollback); 0 clears it."""
        if self.lib.nzcb_debug_inject_fault(self.h, kind) != 0:
            raise ValueError(f"bad fault kind {kind}")

    def signal_basis_info(self) -> dict:
        """The context's signal basis (include/nzcb_internal.h nzcb_debug_signal_basis_info):
        whether A, B, C are committed over it, the rows per set, the points per set in the table,
        the expansion's terms and the table's bytes."""
        out = (c_uint64 * 7)()
        self.lib.nzcb_debug_signal_basis_info(self.h, out)
        return {"on": bool(out[0]), "rows": [int(out[1]), int(out[2]), int(out[3])], "stride": int(out[4]),
                "terms": int(out[5]), "table_bytes": int(out[6])}

    def commit_abc(self, witness_le: bytes, blinding: bytes, signal_basis: bool):
        """A, B and C's commitments of a witness (32-byte LE normal-form values, which need not
        satisfy the circuit) without a proof, over the signal basis or over the Lagrange basis
        (nzcb_debug_commit_abc): three 64-byte affine LEM points."""
        if len(blinding) != BLINDING_BYTES:
            raise ValueError("blinding must be 11 x 32 bytes")
        out = _out(192)
        err = _Err()
        _check(self.lib.nzcb_debug_commit_abc(self.h, _buf(witness_le), len(witness_le) // 32, _buf(blinding),
                                              int(signal_basis), out, ctypes.byref(err)), err)
        b = bytes(out)
        return b[:64], b[64:128], b[128:]

    def signal_rows(self, k: int) -> dict:
        """Set k's rows of the signal basis (0, 1, 2 = A, B, C; nzcb_debug_signal_rows): signal ->
        64-byte affine LEM row. A signal that is not a key has no row in the set."""
        cnt = self.signal_basis_info()["rows"][k]
        rows = _out(64 * cnt)
        sig = (c_uint32 * max(cnt, 1))()
        err = _Err()
        _check(self.lib.nzcb_debug_signal_rows(self.h, k, rows, sig, cnt, ctypes.byref(err)), err)
        b = bytes(rows)
        return {int(sig[i]): b[64 * i:64 * i + 64] for i in range(cnt)}

    def kernel_stats(self, enable: int = -1):
        """MSM bucket-accumulation kernel timing: (ms, launches, points, entries); enable 1/0 resets."""
        out = (c_double * 4)()
        self.lib.nzcb_ctx_kernel_stats(self.h, enable, out)
        return tuple(out)

    def prove(self, wtns, blinding: bytes | None = None):
        """snarkjs-shaped result: {"proof": {...}, "publicSignals": [...]}."""
        proof, pub = self.prove_raw(wtns, blinding)
        return {"proof": proof_to_json(proof), "publicSignals": public_to_json(pub, self.n_public)}

    def last_timings(self):
        """The last proof's phases in ms (include/nzcb.h nzcb_ctx_last_timings): host wall
        clock per round, host time in the MSM calls and enqueueing transforms, and (with
        kernel_stats on) the GPU time of the MSMs and of the transforms."""
        ms = (c_double * 11)()
        k = self.lib.nzcb_ctx_last_timings(self.h, ms, 11)
        names = ["total", "witness", "round1", "round2", "round3", "round4", "round5", "msm_host_wait",
                 "ntt_host_enqueue", "msm_gpu", "ntt_gpu"]
        out = dict(zip(names[:k], list(ms)[:k]))
        return {key: v for key, v in out.items() if v >= 0}


class MsmTable:
    """Resident fixed-base MSM table over device bases (include/nzcb.h nzcb_msm_table_*)."""

    def __init__(self, dev_bases: int, n: int, device: int = 0, _handle=None):
        self.lib = load()
        err = _Err()
        self.n = n
        self.h = _handle or self.lib.nzcb_msm_table_create(device, dev_bases, n, ctypes.byref(err))
        if not self.h:
            raise NzcbError(err.code, err.msg.decode(errors="replace"))

    @classmethod
    def lagrange(cls, dev_ptau: int, ptau_n: int, log_n: int, lo: int, hi: int, device: int = 0):
        """Points [lo, hi) of the Lagrange basis of a 2^log_n domain, from PTau in HBM
        (nzcb_msm_table_create_lagrange): the serving side of the A, B, C commitments."""
        lib = load()
        err = _Err()
        h = lib.nzcb_msm_table_create_lagrange(device, dev_ptau, ptau_n, log_n, lo, hi, ctypes.byref(err))
        if not h:
            raise NzcbError(err.code, err.msg.decode(errors="replace"))
        return cls(0, hi - lo, device, _handle=h)

    def run(self, dev_scalars: int, count: int, scalars_mont: bool = True) -> bytes:
        out = _out(64)
        err = _Err()
        _check(self.lib.nzcb_msm_table_run(self.h, dev_scalars, count, int(scalars_mont), out, ctypes.byref(err)), err)
        return bytes(out)

    def close(self):
        if getattr(self, "h", None):
            self.lib.nzcb_msm_table_destroy(self.h)
            self.h = None

    __del__ = close


class WitnessProgram:
    """A circuit's witness calculator on the GPU (include/nzcb.h nzcb_wprog_*): the
    program written by nzcb.circuit.Circuit.write_program (nzcp_live: nzcb.nzcpgen),
    uploaded once, run for a batch of input vectors, one workgroup per witness."""

    def __init__(self, program: bytes, device: int = 0):
        self.lib = load()
        self.device = device
        err = _Err()
        self.h = self.lib.nzcb_wprog_create(program, len(program), device, ctypes.byref(err))
        if not self.h:
            raise NzcbError(err.code, err.msg.decode(errors="replace"))
        info = (c_uint32 * 5)()
        self.lib.nzcb_wprog_info(self.h, info)
        self.n_wires, self.n_out, self.n_pub_in, self.n_prv_in, self.n_levels = list(info)
        self.n_inputs = self.n_pub_in + self.n_prv_in

    def close(self):
        if getattr(self, "h", None):
            self.lib.nzcb_wprog_destroy(self.h)
            self.h = None

    __del__ = close

    def run(self, inputs: bytes, count: int):
        """Host path: returns (witnesses bytes count x n_wires x 32, statuses)."""
        out = _out(max(1, count * self.n_wires * 32))
        st = (ctypes.c_int32 * max(count, 1))()
        err = _Err()
        _check(self.lib.nzcb_wprog_run(self.h, inputs, count, out, st, ctypes.byref(err)), err)
        return bytes(out)[:count * self.n_wires * 32], [st[i] for i in range(count)]

    def run_dev(self, dev_inputs: int, count: int, dev_witness: int, stride: int) -> list:
        """Device path: witnesses written at dev_witness + i * stride; returns statuses."""
        st = (ctypes.c_int32 * max(count, 1))()
        err = _Err()
        _check(self.lib.nzcb_wprog_run_dev(self.h, dev_inputs, count, dev_witness, stride, st, None,
                                           ctypes.byref(err)), err)
        return [st[i] for i in range(count)]


class R1cs:
    """An r1cs resident on the GPU and the witness check against it (include/nzcb.h
    nzcb_r1cs_*; snarkjs ``wtns check``). data_or_path: the iden3 r1cs bytes, or a file name
    (memory-mapped). device = R1CS_HOST (-1) runs the same check on the host. ``info`` holds
    n_wires, n_outputs, n_pub_inputs, n_prv_inputs, n_constraints, n_terms, long_row_threshold
    and n_long_rows. long_row_threshold / witness_tile: tuning knobs (include/nzcb_internal.h
    nzcb_engine_r1cs_create); the results do not depend on them."""

    INFO = ("n_wires", "n_outputs", "n_pub_inputs", "n_prv_inputs", "n_constraints", "n_terms",
            "long_row_threshold", "n_long_rows")

    def __init__(self, data_or_path, device: int = 0, long_row_threshold: int = 0, witness_tile: int = 0):
        self.lib = load()
        self.device = device
        err = _Err()
        if isinstance(data_or_path, (bytes, bytearray, memoryview)):
            data = bytes(data_or_path)
            if long_row_threshold or witness_tile:
                self.h = self.lib.nzcb_engine_r1cs_create(data, len(data), device, long_row_threshold, witness_tile,
                                                          ctypes.byref(err))
            else:
                self.h = self.lib.nzcb_r1cs_create(data, len(data), device, ctypes.byref(err))
        elif long_row_threshold or witness_tile:
            raise ValueError("the tuning knobs take the r1cs as bytes")
        else:
            self.h = self.lib.nzcb_r1cs_create_file(os.fsencode(data_or_path), device, ctypes.byref(err))
        if not self.h:
            raise NzcbError(err.code, err.msg.decode(errors="replace"))
        info = (c_uint32 * 8)()
        self.lib.nzcb_r1cs_info(self.h, info)
        self.info = dict(zip(self.INFO, list(info)))
        self.n_wires = self.info["n_wires"]

    def close(self):
        if getattr(self, "h", None):
            self.lib.nzcb_r1cs_destroy(self.h)
            self.h = None

    __del__ = close

    def _check(self, witness, n: int, kind: int, count: int, stride: int, bad_cap: int) -> list:
        res = (c_uint32 * (2 * max(count, 1)))()
        bad = (c_uint32 * max(count * bad_cap, 1))()
        err = _Err()
        _check(self.lib.nzcb_r1cs_check(self.h, witness, n, kind, count, stride, res, bad, bad_cap, None,
                                        ctypes.byref(err)), err)
        out = []
        for i in range(count):
            n_bad = res[2 * i]
            out.append({"n_bad": n_bad, "first_bad": res[2 * i + 1] if n_bad else None,
                        "bad": list(bad[i * bad_cap:i * bad_cap + min(n_bad, bad_cap)])})
        return out

    def check(self, witnesses, count=None, bad_cap: int = 8, stride=None) -> list:
        """witnesses: .wtns bytes (one witness), or `count` witnesses of 32-byte LE values,
        witness i at byte i * stride (default: packed, and count = all that the bytes hold).
        Returns one dict per witness: n_bad, first_bad (None when satisfied) and bad, the lowest
        min(n_bad, bad_cap) failing constraint indices in ascending order."""
        data = bytes(witnesses)
        if data[:4] == b"wtns":
            return self._check(data, len(data), WITNESS_WTNS, 1, 0, bad_cap)
        wbytes = 32 * self.n_wires
        if stride is not None:
            n = self.n_wires
            if count is None:
                count = (len(data) + stride - wbytes) // stride if stride else 0
            if count and (count - 1) * stride + wbytes > len(data):
                raise ValueError("the witnesses do not fit the buffer")
        else:
            if count is None:
                count = len(data) // wbytes if wbytes and len(data) % wbytes == 0 else 1
            n = len(data) // 32 // count if count else self.n_wires
            stride = 32 * n
            if count and len(data) != count * stride:
                raise ValueError("the buffer is not `count` witnesses of whole values")
        return self._check(data, n, WITNESS_HOST, count, stride, bad_cap)

    def check_dev(self, dev_witness: int, count: int, stride: int, bad_cap: int = 8) -> list:
        """`count` witnesses in HBM, witness i at dev_witness + i * stride (what
        WitnessProgram.run_dev writes), checked in place."""
        return self._check(c_void_p(dev_witness), self.n_wires, WITNESS_DEVICE, count, stride, bad_cap)

    @staticmethod
    def timings() -> list:
        """Kernel ms of this thread's last device check: lane-per-row, wave-per-row, collect."""
        ms = (c_double * 3)()
        n = load().nzcb_debug_r1cs_check_timings(ms, 3)
        return list(ms)[:n]


def _b64url(s: str) -> bytes:
    import base64
    return base64.urlsafe_b64decode(s + "=" * (-len(s) % 4))


def p256_field(op: str, field: str, a, b=None, device: int = 0) -> list:
    """csrc/p256.h's field arithmetic as compiled for `device` (P256_HOST: for the host), over
    lists of integers below the modulus: op in P256_OPS, field "p" or "n" (include/
    nzcb_internal.h nzcb_debug_p256_field). Returns the list of results."""
    b = a if b is None else b
    if len(a) != len(b):
        raise ValueError("operand lists differ in length")
    ab = b"".join(int(x).to_bytes(32, "big") for x in a)
    bb = b"".join(int(x).to_bytes(32, "big") for x in b)
    out = _out(32 * len(a))
    err = _Err()
    _check(load().nzcb_debug_p256_field(device, P256_OPS[op], {"p": 0, "n": 1}[field], ab, bb, len(a), out,
                                        ctypes.byref(err)), err)
    raw = bytes(out)
    return [int.from_bytes(raw[32 * i:32 * i + 32], "big") for i in range(len(a))]


class P256Key:
    """An ECDSA P-256 public key with its fixed-base tables resident on the GPU, and batch
    verification of SHA-256 digests against r || s signatures (include/nzcb.h nzcb_p256_*; COSE
    ES256, the signature of an NZ COVID Pass). The key is (x, y) as integers or 32-byte
    big-endian strings, 64 bytes x || y, or a JWK / DID-document dict with base64url "x" and "y".
    device = P256_HOST (-1) builds the tables and verifies on the host. Whether the key is the
    issuer's is the caller's business. window: the tables' window width, 4 or 8 (0: the
    library's default; include/nzcb_internal.h); the statuses do not depend on it."""

    def __init__(self, x, y=None, device: int = 0, window: int = 0):
        if isinstance(x, dict):
            xy = _b64url(x["x"]) + _b64url(x["y"])
        elif y is None:
            xy = bytes(x)
        else:
            xy = b"".join(v.to_bytes(32, "big") if isinstance(v, int) else bytes(v) for v in (x, y))
        if len(xy) != 64:
            raise ValueError("a P-256 public key is 32 + 32 bytes")
        self.lib = load()
        self.device = device
        self.xy = xy
        err = _Err()
        if window:
            self.h = self.lib.nzcb_engine_p256_key_create(xy, device, window, ctypes.byref(err))
        else:
            self.h = self.lib.nzcb_p256_key_create(xy, device, ctypes.byref(err))
        if not self.h:
            raise NzcbError(err.code, err.msg.decode(errors="replace"))

    def close(self):
        if getattr(self, "h", None):
            self.lib.nzcb_p256_key_destroy(self.h)
            self.h = None

    __del__ = close

    def _verify(self, hashes, hash_stride: int, sigs, sig_stride: int, count: int, on_device: bool,
                stream=None) -> list:
        st = (ctypes.c_int32 * max(count, 1))()
        err = _Err()
        _check(self.lib.nzcb_p256_verify(self.h, hashes, hash_stride, sigs, sig_stride, count, int(on_device), st,
                                         stream, ctypes.byref(err)), err)
        return [st[i] for i in range(count)]

    def verify(self, hashes, sigs, hash_stride: int = 32, sig_stride: int = 64) -> list:
        """hashes: 32-byte digests, sigs: 64-byte r || s, each a list of byte strings or one
        buffer with item i at i * stride. Returns one SIG_OK / SIG_INVALID / SIG_RANGE each."""
        if isinstance(hashes, (list, tuple)):
            if any(len(h) != 32 for h in hashes):
                raise ValueError("a hash is 32 bytes")
            hashes, hash_stride = b"".join(hashes), 32
        if isinstance(sigs, (list, tuple)):
            if any(len(s) != 64 for s in sigs):
                raise ValueError("a signature is 64 bytes (r || s)")
            sigs, sig_stride = b"".join(sigs), 64
        hashes, sigs = bytes(hashes), bytes(sigs)
        if hash_stride < 32 or sig_stride < 64:
            raise ValueError("strides are at least 32 and 64")
        def items(buf, stride, size, what):
            if stride == size and len(buf) % size:
                raise ValueError(f"the {what} are not whole {size}-byte items")
            return (len(buf) + stride - size) // stride if len(buf) >= size else 0

        count = items(hashes, hash_stride, 32, "hashes")
        if items(sigs, sig_stride, 64, "signatures") != count or (not count and (hashes or sigs)):
            raise ValueError("the signatures do not match the hashes")
        return self._verify(hashes, hash_stride, sigs, sig_stride, count, False)

    def verify_dev(self, dev_hashes: int, hash_stride: int, dev_sigs: int, sig_stride: int, count: int,
                   stream: int | None = None) -> list:
        """The same over HBM buffers on the key's device, read in place (pointers and strides
        multiples of 4). The buffers must be complete when the call starts, or their producer
        enqueued on `stream` (a HIP stream handle) before it: without one the call runs on a
        stream of its own, which waits for no other stream."""
        return self._verify(c_void_p(dev_hashes), hash_stride, c_void_p(dev_sigs), sig_stride, count, True, stream)

    def verify_records(self, dev_records: int, dev_sigs: int, count: int, stream: int | None = None) -> list:
        """`count` nzcb_nzcp_record in HBM, as nzcp_witness_dev wrote them: record i's tbs_sha256
        against the 64-byte signature at dev_sigs + 64 i. nzcp_witness_dev is asynchronous: pass
        the stream it ran on, or synchronise first (see verify_dev)."""
        return self.verify_dev(dev_records + NzcpRecord.tbs_sha256.offset, ctypes.sizeof(NzcpRecord), dev_sigs, 64,
                               count, stream)

    def verify_passes(self, uris) -> list:
        """Pass URIs -> one dict each: valid, status (SIG_*, or None when the pass was not sent
        to the verifier), reason (None when valid), alg, kid, iss, nbf, exp. The Sig_structure is
        hashed on the host; an alg other than -7 (ES256), a signature that is not 64 bytes or a
        pass that does not decode is reported with its reason and not verified."""
        import hashlib
        from . import nzcp
        out, hashes, sigs, sent = [], [], [], []
        for uri in uris:
            d = {"valid": False, "status": None, "reason": None, "alg": None, "kid": None, "iss": None,
                 "nbf": None, "exp": None}
            out.append(d)
            try:
                protected, payload, sig = nzcp.decode_pass(uri)
                hdr = nzcp.protected_header(uri)
                claims, _ = nzcp.cbor_decode(payload)
                d.update(alg=hdr.get(1), kid=hdr.get(4), iss=claims.get(1), nbf=claims.get(5), exp=claims.get(4))
            except Exception as e:  # noqa: BLE001  (any malformed pass is a verdict, not a failure of the batch)
                d["reason"] = f"malformed pass: {e}"
                continue
            if d["alg"] != -7:
                d["reason"] = f"unsupported alg {d['alg']} (ES256 is -7)"
            elif not isinstance(sig, bytes) or len(sig) != 64:
                d["reason"] = "signature is not 64 bytes"
            else:
                hashes.append(hashlib.sha256(nzcp.sig_structure(protected, payload)).digest())
                sigs.append(sig)
                sent.append(d)
        for d, st in zip(sent, self.verify(hashes, sigs) if sent else []):
            d["status"] = st
            d["valid"] = st == SIG_OK
            d["reason"] = None if st == SIG_OK else ("invalid signature" if st == SIG_INVALID
                                                      else "signature out of range")
        return out

    def verify_uris(self, uris) -> list:
        """verify_passes with the decoding on the key's device too: the URIs' bytes go up, the
        decode kernel (nzcp_decode_dev) and the verification, which reads each record's digest and
        signature in place, run on one stream, and the records come down once. The dicts have
        verify_passes' keys and reason texts, except that a pass that does not decode is reported
        as "malformed pass: <status name> at <detail>" (PASS_STATUS_NAMES). The record keeps the
        first 32 bytes of a kid and 64 of an iss. A host key decodes and verifies on the host."""
        uris = list(uris)
        n = len(uris)
        if not n:
            return []
        size, off_h, off_s = ctypes.sizeof(NzcpPass), NzcpPass.tbs_sha256.offset, NzcpPass.sig.offset
        if self.device == P256_HOST:
            raw, _, _ = nzcp_decode_raw(uris, device=NZCP_HOST)
            statuses = self.verify(raw[off_h:], raw[off_s:], hash_stride=size, sig_stride=size)
        else:
            blob, offs = pack_uris(uris)
            lib = self.lib
            prev, stream, bufs = c_int(-1), c_void_p(), []
            if lib.hipGetDevice(ctypes.byref(prev)) or lib.hipSetDevice(self.device):
                raise NzcbError(10, "cannot select the key's device")
            try:
                for nbytes in (len(blob), 4 * (n + 1), size * n):
                    bufs.append(lib.nzcb_dev_alloc_on(self.device, max(nbytes, 4)))
                    if not bufs[-1]:
                        raise MemoryError("device allocation failed")
                d_uris, d_off, d_rec = bufs
                if blob:
                    h2d(d_uris, blob)
                h2d(d_off, bytes(offs))
                if lib.hipStreamCreate(ctypes.byref(stream)):
                    raise NzcbError(10, "cannot create a HIP stream")
                nzcp_decode_dev(d_uris, d_off, n, d_rec, device=self.device, stream=stream)
                statuses = self.verify_dev(d_rec + off_h, size, d_rec + off_s, size, n, stream)
                raw = d2h(d_rec, size * n)
            finally:
                if stream:
                    lib.hipStreamDestroy(stream)
                for p in bufs:
                    if p:
                        lib.nzcb_dev_free(p)
                lib.hipSetDevice(prev)
        out = []
        for r, st in zip(nzcp_passes_from_bytes(raw, n), statuses):
            d = {"valid": False, "status": None, "reason": None, "alg": None, "kid": None, "iss": None,
                 "nbf": None, "exp": None}
            out.append(d)
            if r["status"]:
                d["reason"] = f"malformed pass: {r['status_name']} at {r['detail']}"
                continue
            d.update(alg=r["alg"], kid=r["kid"], iss=r["iss"], nbf=r["nbf"], exp=r["exp"])
            if d["alg"] != -7:
                d["reason"] = f"unsupported alg {d['alg']} (ES256 is -7)"
            elif r["sig"] is None or r["sig_len"] != 64:
                d["reason"] = "signature is not 64 bytes"
            else:   # every other pass's verdict, computed over a zeroed signature, is dropped
                d["status"] = st
                d["valid"] = st == SIG_OK
                d["reason"] = None if st == SIG_OK else ("invalid signature" if st == SIG_INVALID
                                                          else "signature out of range")
        return out

    def mul2(self, u1, u2) -> list:
        """u1[i] G + u2[i] Q through the verifier's table code (include/nzcb_internal.h
        nzcb_debug_p256_mul2): affine (x, y) integer pairs, None for the point at infinity."""
        if len(u1) != len(u2):
            raise ValueError("scalar lists differ in length")
        a = b"".join(int(v).to_bytes(32, "big") for v in u1)
        b = b"".join(int(v).to_bytes(32, "big") for v in u2)
        out = _out(64 * len(u1))
        err = _Err()
        _check(self.lib.nzcb_debug_p256_mul2(self.h, a, b, len(u1), out, ctypes.byref(err)), err)
        raw = bytes(out)
        pts = []
        for i in range(len(u1)):
            x, y = int.from_bytes(raw[64 * i:64 * i + 32], "big"), int.from_bytes(raw[64 * i + 32:64 * i + 64], "big")
            pts.append(None if x == 0 and y == 0 else (x, y))
        return pts

    @staticmethod
    def timings() -> list:
        """Milliseconds of this thread's last calls: table build, verify kernel, verify call."""
        ms = (c_double * 3)()
        n = load().nzcb_debug_p256_timings(ms, 3)
        return list(ms)[:n]


def wprog_remap(program: bytes, own_sym: bytes, target_sym: bytes) -> bytes:
    """nzcb_wprog_remap: the witness program re-indexed to the wire order of target_sym
    (a circom .sym), matching signals by name against the program's own .sym
    (Circuit.write_sym). Raises NzcbError (unmatched count in .unmatched) when a target
    signal has no counterpart."""
    lib = load()
    out = POINTER(c_uint8)()
    n = c_size_t(0)
    miss = c_uint32(0)
    err = _Err()
    rc = lib.nzcb_wprog_remap(program, len(program), own_sym, len(own_sym), target_sym, len(target_sym),
                              ctypes.byref(out), ctypes.byref(n), ctypes.byref(miss), ctypes.byref(err))
    if rc:
        e = NzcbError(err.code, err.msg.decode(errors="replace"))
        e.unmatched = miss.value
        raise e
    try:
        return ctypes.string_at(out, n.value)
    finally:
        lib.nzcb_free(out)


class NzcpProver:
    """fullProve for nzcp passes on one GPU: the nzcp witness kernel computes each pass's
    public signals (NZCPPubIdentity out[0..2], include/nzcb.h nzcb_nzcp_witness_dev)
    straight into that proof's HBM witness, then nzcb_prove_batch proves them.

    The circuit is a zkey whose public signals are witness[1..3] (snarkjs convention:
    main's outputs first). The rest of each witness is `base_witness` (the nzcp_live
    stand-in of SURVEY.md §8d: a synthetic circuit built with free_public=True, since
    the real r1cs/wasm cannot be built offline). A pass whose witness calculation
    fails raises like circom_runtime's calculateWitness does."""

    def __init__(self, ctx: ProverContext, base_witness: bytes, params: dict = NZCP_LIVE):
        if ctx.n_public != 3:
            raise ValueError("nzcp circuits have 3 public signals")
        self.ctx, self.params = ctx, dict(params)
        self.device = ctx.device
        self.n_witness = len(base_witness) // 32
        self.n_inputs = nzcp_input_signals(self.params)
        self._base = dev_alloc(len(base_witness))
        h2d(self._base, base_witness)
        self._block, self._block_count = None, 0   # per-proof device witnesses, grown on demand
        self._rec = None                          # device records of the same passes
        self._inputs, self._inputs_cap = None, 0

    def close(self):
        for p in (self._block, self._rec, self._base, self._inputs):
            if p:
                dev_free(p)
        self._block = self._rec = self._base = self._inputs = None

    def witness_buffers(self, count: int):
        """Device pointers of `count` witnesses, one contiguous block (stride n_witness x 32 B),
        each initialised from the base witness."""
        stride = self.n_witness * 32
        if count > self._block_count:
            if self._block:
                dev_free(self._block)
                dev_free(self._rec)
            self._block = dev_alloc(stride * count)
            self._rec = dev_alloc(ctypes.sizeof(NzcpRecord) * count)
            for i in range(count):
                d2d(self._block + i * stride, self._base, stride)
            self._block_count = count
        return [self._block + i * stride for i in range(count)]

    def upload_inputs(self, inputs: bytes) -> int:
        """Stage count x n_inputs x 32 B of input signals in HBM; returns the pass count."""
        per = self.n_inputs * 32
        if len(inputs) % per:
            raise ValueError("inputs are not a whole number of passes")
        if len(inputs) > self._inputs_cap:
            if self._inputs:
                dev_free(self._inputs)
            self._inputs, self._inputs_cap = dev_alloc(len(inputs)), len(inputs)
        h2d(self._inputs, inputs)
        return len(inputs) // per

    def witness_staged(self, count: int) -> list:
        """nzcp witness of the staged passes: public signals into witness[1..3] of each
        proof's HBM witness; returns the records. Raises on a failed pass."""
        if count == 0:
            return []
        bufs = self.witness_buffers(count)
        rec_size = ctypes.sizeof(NzcpRecord)
        nzcp_witness_dev(self._inputs, count, self.params, self.device, self._rec, bufs[0], self.n_witness * 32)
        recs = nzcp_records_from_bytes(d2h(self._rec, rec_size * count), count)
        for i, r in enumerate(recs):
            if r["status"] != 0:
                raise NzcbError(r["status"], f"nzcp witness of pass {i} failed: "
                                             f"{NZCP_STATUS.get(r['status'], r['status'])} (detail {r['detail']})")
        return recs

    def full_prove_staged(self, count: int, blindings=None):
        """Witness + proof for the `count` passes staged by upload_inputs (all in HBM).
        Returns ([(proof, public)], records)."""
        recs = self.witness_staged(count)
        res = self.ctx.prove_batch_raw(self.witness_buffers(count), n_witness=self.n_witness, blindings=blindings,
                                       on_device=True)
        return res, recs

    def full_prove(self, inputs: bytes, blindings=None):
        return self.full_prove_staged(self.upload_inputs(inputs), blindings)


NZCP_STATUS = {0: "ok", 1: "toBeSigned bit check", 2: "toBeSignedLen > MaxToBeSignedBytes",
               3: "LessThan operands out of range", 4: "QuinSelector index out of range",
               5: "CBOR type is not a map", 6: "CBOR map length > 23", 7: "CBOR type is not a string",
               8: "negative toBeSignedLen (unpinned)"}


def proof_to_json(proof: bytes) -> dict:
    lib = load()
    cap = 8192
    out = ctypes.create_string_buffer(cap)
    rc = lib.nzcb_proof_to_json(_buf(proof), out, cap)
    if rc:
        raise NzcbError(1, "json buffer too small")
    return json.loads(out.value.decode())


def public_to_json(pub: bytes, n_public: int) -> list:
    lib = load()
    cap = 80 * n_public + 8
    out = ctypes.create_string_buffer(cap)
    rc = lib.nzcb_public_to_json(_buf(pub), n_public, out, cap)
    if rc:
        raise NzcbError(1, "json buffer too small")
    return json.loads(out.value.decode())


def _json_text(fn, *args) -> str:
    need = fn(*args, None, 0)
    out = ctypes.create_string_buffer(max(need, 1))
    rc = fn(*args, out, max(need, 1))
    if rc != 0:
        raise NzcbError(11, "json encoding failed")
    return out.value.decode()


def vk_from_zkey(zkey) -> bytes:
    """Binary verification key (include/nzcb.h NZCB_VK_BYTES) of a zkey: bytes, a path, or
    a (pointer, length) library buffer (nzcb.plonk_setup_raw)."""
    out = _out(VK_BYTES)
    err = _Err()
    if isinstance(zkey, str):   # memory-mapped by the library (zkeys past 2 GiB)
        _check(load().nzcb_vk_from_zkey_file(zkey.encode(), out, ctypes.byref(err)), err)
        return bytes(out)
    if isinstance(zkey, tuple):
        ptr, size = ctypes.cast(zkey[0], POINTER(c_uint8)), zkey[1]
    else:
        ptr, size = _buf(zkey), len(zkey)
    _check(load().nzcb_vk_from_zkey(ptr, size, out, ctypes.byref(err)), err)
    return bytes(out)


def vk_to_json(vk: bytes) -> dict:
    """snarkjs verification_key.json object."""
    import json
    return json.loads(_json_text(load().nzcb_vk_to_json, _buf(vk)))


def _le(x) -> bytes:
    return int(x).to_bytes(32, "little")


def vk_from_json(obj: dict) -> bytes:
    """verification_key.json (snarkjs layout) -> binary verification key."""
    def g1(p):
        return bytes(64) if str(p[2]) == "0" else _le(p[0]) + _le(p[1])

    out = int(obj["nPublic"]).to_bytes(4, "little") + int(obj["power"]).to_bytes(4, "little")
    out += _le(obj["k1"]) + _le(obj["k2"])
    out += b"".join(g1(obj[k]) for k in VK_POINTS)
    (x0, x1), (y0, y1) = obj["X_2"][0], obj["X_2"][1]
    out += _le(x0) + _le(x1) + _le(y0) + _le(y1) + _le(obj["w"])
    return out


def proof_from_json(obj: dict) -> bytes:
    """snarkjs proof object -> NZCB_PROOF_BYTES."""
    def g1(p):
        return bytes(64) if str(p[2]) == "0" else _le(p[0]) + _le(p[1])

    return b"".join(g1(obj[k]) for k in PROOF_POINTS) + b"".join(_le(obj[k]) for k in PROOF_EVALS)


def verify(vk: bytes, proof: bytes, public: bytes, transcript_public: bool = True) -> bool:
    """Pairing verification of a binary proof; public = nPublic x 32-byte LE."""
    valid = c_int(0)
    err = _Err()
    _check(load().nzcb_verify(_buf(vk), _buf(proof), _buf(public), len(public) // 32, int(transcript_public),
                              ctypes.byref(valid), ctypes.byref(err)), err)
    return bool(valid.value)


def verify_batch(vk: bytes, proofs, publics, transcript_public: bool = True, device: int = 0,
                 seed: bytes | None = None) -> list:
    """nzcb.verify for many proofs of one key (include/nzcb.h nzcb_verify_batch): one pairing
    check for the batch, the G1 scalar multiplications on GPU `device` (VERIFY_HOST: on the
    host). proofs: binary proofs; publics: per proof nPublic x 32-byte LE. `seed` (32 bytes)
    fixes the random weights, for reproducible tests only. Returns one bool per proof."""
    count = len(proofs)
    if len(publics) != count or any(len(p) != PROOF_BYTES for p in proofs):
        raise ValueError("verify_batch: one public-signal buffer per proof of PROOF_BYTES bytes")
    if seed is not None and len(seed) != 32:
        raise ValueError("verify_batch: the seed is 32 bytes")
    n_public = len(publics[0]) // 32 if count else 0
    if any(len(p) != 32 * n_public for p in publics):
        raise ValueError("verify_batch: every item has the same number of public signals")
    valid = (c_int * max(count, 1))()
    err = _Err()
    _check(load().nzcb_verify_batch(_buf(vk), _buf(b"".join(proofs)), _buf(b"".join(publics)), 32 * n_public,
                                    n_public, count, int(transcript_public), device,
                                    _buf(seed) if seed else None, valid, ctypes.byref(err)), err)
    return [bool(valid[i]) for i in range(count)]


def proof_to_calldata(proof: bytes, public: bytes) -> str:
    """snarkjs `zkey export soliditycalldata` text for a PLONK proof."""
    return _json_text(load().nzcb_proof_to_calldata, _buf(proof), _buf(public), len(public) // 32)


def vk_to_solidity(vk: bytes, contract_name: str = "PlonkVerifier", transcript_public: bool = True) -> str:
    """snarkjs `zkey export solidityverifier`: the Solidity PLONK verifier of a binary
    verification key (include/nzcb.h nzcb_vk_to_solidity)."""
    fn = load().nzcb_vk_to_solidity
    name = contract_name.encode()
    need = fn(_buf(vk), name, int(transcript_public), None, 0)
    if need < 0:
        raise NzcbError(1, f"solidity verifier: bad verification key or contract name {contract_name!r}")
    out = ctypes.create_string_buffer(need)
    if fn(_buf(vk), name, int(transcript_public), out, need) != 0:
        raise NzcbError(11, "solidity verifier: rendering failed")
    return out.value.decode()


class plonk:
    """snarkjs-compatible entry points (``snarkjs.plonk.prove`` / ``verify`` [EXT])."""

    @staticmethod
    def verify(vk_verifier: dict, publicSignals, proof: dict, transcript_public: bool = True) -> bool:
        """snarkjs.plonk.verify(vkey, publicSignals, proof) on the JSON objects."""
        pub = b"".join(_le(x) for x in publicSignals)
        return verify(vk_from_json(vk_verifier), proof_from_json(proof), pub, transcript_public)

    @staticmethod
    def verify_batch(vk_verifier: dict, publicSignalsArray, proofArray, transcript_public: bool = True,
                     device: int = 0) -> list:
        """plonk.verify for many proofs of one key on the JSON objects: one bool per proof."""
        pubs = [b"".join(_le(x) for x in ps) for ps in publicSignalsArray]
        return verify_batch(vk_from_json(vk_verifier), [proof_from_json(p) for p in proofArray], pubs,
                            transcript_public, device)

    @staticmethod
    def prove(zkeyFileName, witnessFileName, logger=None, device: int = 0, blinding: bytes | None = None):
        ctx = ProverContext(zkeyFileName, device=device, logger=logger)
        try:
            if blinding is None:
                blinding = random_blinding()
            return ctx.prove(witnessFileName, blinding)
        finally:
            ctx.close()


def random_blinding() -> bytes:
    """11 uniform Fr scalars (snarkjs ``Fr.random()``), 32-byte LE each."""
    import secrets
    r = 21888242871839275222246405745257275088548364400416034343698204186575808495617
    return b"".join((secrets.randbelow(r)).to_bytes(32, "little") for _ in range(11))


SYNTH_FREE_PUBLIC = 1


def _synth_raw(power, n_public, n_inputs, seed, n_constraints, tau, device, free_public):
    lib = load()
    zp = POINTER(c_uint8)()
    wp = POINTER(c_uint8)()
    zl = c_size_t()
    wl = c_size_t()
    err = _Err()
    taub = _buf(int(tau).to_bytes(32, "little"))
    flags = SYNTH_FREE_PUBLIC if free_public else 0
    _check(lib.nzcb_synth_setup_ex(power, n_public, n_inputs, seed, n_constraints, flags, taub, device,
                                   ctypes.byref(zp), ctypes.byref(zl), ctypes.byref(wp), ctypes.byref(wl),
                                   ctypes.byref(err)), err)
    return zp, zl.value, wp, wl.value


def synth_context(power: int, n_public: int = 3, n_inputs: int = 8, seed: int = 0x6E7A6362,
                  n_constraints: int = 0, tau: int = 0x6E7A6362746175, device: int = 0, free_public: bool = False):
    """Build the synthetic circuit's zkey on `device` and upload it straight into a
    ProverContext without copying the (multi-GB) zkey through Python. Returns (ctx, wtns bytes).
    free_public: public signals on their public-input gate only (NZCB_SYNTH_FREE_PUBLIC)."""
    lib = load()
    zp, zl, wp, wl = _synth_raw(power, n_public, n_inputs, seed, n_constraints, tau, device, free_public)
    try:
        ctx = ProverContext(None, device=device, _raw=(zp, zl))
        wtns = _take(wp, wl)
    finally:
        lib.nzcb_free(ctypes.cast(zp, c_void_p))
        lib.nzcb_free(ctypes.cast(wp, c_void_p))
    return ctx, wtns


def synth_setup(power: int, n_public: int = 3, n_inputs: int = 8, seed: int = 0x6E7A6362,
                n_constraints: int = 0, tau: int = 0x6E7A6362746175, device: int = 0, free_public: bool = False):
    """Seeded synthetic circuit + zkey built on the GPU (``nzcb_synth_setup_ex``). Returns (zkey, wtns) bytes."""
    lib = load()
    zp, zl, wp, wl = _synth_raw(power, n_public, n_inputs, seed, n_constraints, tau, device, free_public)
    try:
        zkey = _take(zp, zl)
        wtns = _take(wp, wl)
    finally:
        lib.nzcb_free(ctypes.cast(zp, c_void_p))
        lib.nzcb_free(ctypes.cast(wp, c_void_p))
    return zkey, wtns


def plonk_setup(r1cs: bytes, ptau: bytes, device: int = 0) -> bytes:
    """snarkjs ``plonk setup <r1cs> <ptau> <zkey>`` (snarkjs 0.4.12 plonk_setup.js, run at
    /root/reference/Makefile:55,60): returns the PLONK zkey bytes. The NTTs and the
    commitments run on `device`; raises NzcbError as snarkjs throws (curve mismatch,
    "circuit too big for this power of tau ceremony", "Variable not used")."""
    ptr, size = plonk_setup_raw(r1cs, ptau, device)
    try:
        return _take(ptr, size)
    finally:
        load().nzcb_free(ptr)


def plonk_setup_raw(r1cs: bytes, ptau: bytes, device: int = 0):
    """plonk_setup returning the library-owned zkey buffer (pointer, length) without a
    host copy (a 2^21 zkey is about 3.9 GB); release with nzcb.free_ptr."""
    lib = load()
    zp = POINTER(c_uint8)()
    zl = c_size_t()
    err = _Err()
    _check(lib.nzcb_plonk_setup(bytes(r1cs), len(r1cs), bytes(ptau), len(ptau), device, ctypes.byref(zp),
                                ctypes.byref(zl), ctypes.byref(err)), err)
    return ctypes.cast(zp, c_void_p).value, zl.value


def free_ptr(ptr: int):
    load().nzcb_free(ptr)


def _take(ptr, size: int) -> bytes:
    """bytes of a library buffer (ctypes.string_at takes an int size, < 2 GiB)."""
    addr = ctypes.cast(ptr, c_void_p).value if not isinstance(ptr, int) else ptr
    return bytes((c_uint8 * size).from_address(addr)) if size else b""


def _finding_dict(f: KeyFinding) -> dict:
    return {"status": KEY_STATUS_NAMES[f.status], "pairing_checks": f.pairing_checks, "index": f.index,
            "n_bad": f.n_bad, "checked": f.checked}


def _host_view(data):
    """(pointer, length, keep-alive) of key material in host memory; bytes and bytearrays are not
    copied (a zkey can be several GB)."""
    if isinstance(data, bytearray):
        keep = (c_uint8 * len(data)).from_buffer(data)
        return ctypes.cast(keep, c_void_p), len(data), keep
    if not isinstance(data, bytes):
        data = bytes(data)
    return ctypes.cast(ctypes.c_char_p(data), c_void_p), len(data), data


def ptau_check(ptau_or_path, count: int = 0, device: int = 0, seed: bytes | None = None) -> dict:
    """Examine a powers-of-tau file (bytes, or a path, which is memory-mapped) on GPU `device`
    (KEY_HOST: on the host) before a setup uses it (include/nzcb.h nzcb_ptau_check): every tauG1
    point on the curve, P_0 the generator, and P_i = tau P_(i-1) against the file's [tau]G2 by
    one pairing check under random weights. count = 0 checks every point the header promises,
    otherwise the first `count` (a circuit of domain 2^p uses 2^p + 6). Returns the finding:
    status ("OK", "G2", "RANGE", "CURVE", "GENERATOR", "SEQUENCE"), index, n_bad, checked,
    pairing_checks. A malformed file raises NzcbError. seed: 32 bytes, for reproducible tests only."""
    if seed is not None and len(seed) != 32:
        raise ValueError("ptau_check: the seed is 32 bytes")
    f = KeyFinding()
    err = _Err()
    sd = _buf(seed) if seed else None
    if isinstance(ptau_or_path, (str, os.PathLike)):
        rc = load().nzcb_ptau_check_file(os.fsencode(ptau_or_path), count, device, sd, ctypes.byref(f),
                                         ctypes.byref(err))
    else:
        ptr, n, keep = _host_view(ptau_or_path)
        rc = load().nzcb_ptau_check(ptr, n, count, device, sd, ctypes.byref(f), ctypes.byref(err))
        del keep
    _check(rc, err)
    return _finding_dict(f)


def zkey_check(zkey_or_path, device: int = 0, seed: bytes | None = None) -> dict:
    """Examine a PLONK zkey (bytes, or a path, which is memory-mapped) on GPU `device` (KEY_HOST:
    on the host) before a context loads it (include/nzcb.h nzcb_zkey_check). Returns
    {"ok": bool, "header": finding of k1, k2 (COSETS), "srs": finding of the key's PTau against
    X_2, "parts": {"Qm": finding, ..., "S3": ..., "L0": ...}}; a part's status is "OK",
    "NONCANONICAL", "LAGRANGE", "EVALS" or "COMMIT" and carries commit_checked. Whether the key
    belongs to your circuit is not examined: that needs the r1cs."""
    if seed is not None and len(seed) != 32:
        raise ValueError("zkey_check: the seed is 32 bytes")
    lib = load()
    ok = c_int(0)
    hdr = (KeyFinding * 2)()
    n_parts = c_uint32(0)
    err = _Err()
    sd = _buf(seed) if seed else None
    cap = 64
    while True:
        parts = (KeyFinding * cap)()
        if isinstance(zkey_or_path, (str, os.PathLike)):
            rc = lib.nzcb_zkey_check_file(os.fsencode(zkey_or_path), device, sd, ctypes.byref(ok), hdr, parts, cap,
                                          ctypes.byref(n_parts), ctypes.byref(err))
        else:
            ptr, n, keep = _host_view(zkey_or_path)
            rc = lib.nzcb_zkey_check(ptr, n, device, sd, ctypes.byref(ok), hdr, parts, cap, ctypes.byref(n_parts),
                                     ctypes.byref(err))
            del keep
        _check(rc, err)
        if n_parts.value <= cap:
            break
        cap = n_parts.value
    out = {}
    for k in range(n_parts.value):
        d = _finding_dict(parts[k])
        d["commit_checked"] = bool(d.pop("pairing_checks"))
        out[KEY_PARTS[k] if k < 8 else f"L{k - 8}"] = d
    return {"ok": bool(ok.value), "header": _finding_dict(hdr[0]), "srs": _finding_dict(hdr[1]), "parts": out}


def ptau_synth(power: int, tau: int, device: int = 0) -> bytes:
    """Powers-of-tau file (snarkjs layout, sections 1-3) for a trapdoor tau, built on the
    GPU (include/nzcb.h nzcb_ptau_synth)."""
    lib = load()
    pp = POINTER(c_uint8)()
    pl = c_size_t()
    err = _Err()
    _check(lib.nzcb_ptau_synth(power, _buf(int(tau).to_bytes(32, "little")), device, ctypes.byref(pp),
                               ctypes.byref(pl), ctypes.byref(err)), err)
    try:
        return _take(pp, pl.value)
    finally:
        lib.nzcb_free(pp)


def _take_ptau(lib, pp, pl) -> bytes:
    try:
        return _take(pp, pl.value)
    finally:
        lib.nzcb_free(pp)


def _is_path(x) -> bool:
    return isinstance(x, (str, os.PathLike))


def ptau_new(power: int, out_path=None):
    """snarkjs ``powersoftau new bn128 <power>``: a powers-of-tau file (sections 1-7) whose every
    point is its group's generator and that holds no contribution (include/nzcb.h nzcb_ptau_new;
    host only). Returns the bytes, or writes `out_path` and returns it."""
    lib = load()
    err = _Err()
    if out_path is not None:
        _check(lib.nzcb_ptau_new_file(power, os.fsencode(out_path), ctypes.byref(err)), err)
        return out_path
    pp, pl = POINTER(c_uint8)(), c_size_t()
    _check(lib.nzcb_ptau_new(power, ctypes.byref(pp), ctypes.byref(pl), ctypes.byref(err)), err)
    return _take_ptau(lib, pp, pl)


def ptau_contribute(ptau_or_path, out_path=None, secrets=None, entropy=None, device: int = 0):
    """Multiply your own secret into a powers-of-tau file on GPU `device` (PTAU_HOST: on the host):
    tauG1[i], tauG2[i] by tau^i, alphaTauG1[i] by alpha tau^i, betaTauG1[i] by beta tau^i, betaG2
    by beta (include/nzcb.h nzcb_ptau_contribute). secrets = None draws tau, alpha and beta from
    the OS CSPRNG, mixed with the optional `entropy` (str or bytes); a (tau, alpha, beta) tuple of
    integers in [1, r) is FOR REPRODUCIBLE TESTS ONLY. Every input point is tested first; a bad one
    raises NzcbError FORMAT naming its section and index. NO contribution record is written:
    ``snarkjs powersoftau verify`` does not accept the output. The input is bytes, or a path
    (memory-mapped when `out_path` is given). Returns the bytes, or writes `out_path` and returns it."""
    lib = load()
    err = _Err()
    sec = None
    if secrets is not None:
        if len(secrets) != 3:
            raise ValueError("ptau_contribute: secrets are (tau, alpha, beta)")
        if any(not 0 <= int(s) < 1 << 256 for s in secrets):
            raise NzcbError(1, "ptau: a secret is zero or not below r")
        sec = _buf(b"".join(int(s).to_bytes(32, "little") for s in secrets))
    ent = entropy.encode() if isinstance(entropy, str) else bytes(entropy or b"")
    if _is_path(ptau_or_path) and out_path is not None:
        _check(lib.nzcb_ptau_contribute_file(os.fsencode(ptau_or_path), os.fsencode(out_path), sec, ent, len(ent),
                                             device, ctypes.byref(err)), err)
        return out_path
    if _is_path(ptau_or_path):
        with open(ptau_or_path, "rb") as f:
            ptau_or_path = f.read()
    ptr, n, keep = _host_view(ptau_or_path)
    pp, pl = POINTER(c_uint8)(), c_size_t()
    rc = lib.nzcb_ptau_contribute(ptr, n, sec, ent, len(ent), device, ctypes.byref(pp), ctypes.byref(pl),
                                  ctypes.byref(err))
    del keep
    _check(rc, err)
    out = _take_ptau(lib, pp, pl)
    if out_path is None:
        return out
    with open(out_path, "wb") as f:
        f.write(out)
    return out_path


def ptau_prepare_phase2(ptau_or_path, out_path=None, device: int = 0):
    """snarkjs ``powersoftau prepare phase2``: sections 1-7 of the input and the Lagrange sections
    12-15 that snarkjs's setups read, computed by elliptic-curve inverse transforms on GPU `device`
    (PTAU_HOST: on the host; include/nzcb.h nzcb_ptau_prepare_phase2). Input and result as for
    ptau_contribute."""
    lib = load()
    err = _Err()
    if _is_path(ptau_or_path) and out_path is not None:
        _check(lib.nzcb_ptau_prepare_phase2_file(os.fsencode(ptau_or_path), os.fsencode(out_path), device,
                                                 ctypes.byref(err)), err)
        return out_path
    if _is_path(ptau_or_path):
        with open(ptau_or_path, "rb") as f:
            ptau_or_path = f.read()
    ptr, n, keep = _host_view(ptau_or_path)
    pp, pl = POINTER(c_uint8)(), c_size_t()
    rc = lib.nzcb_ptau_prepare_phase2(ptr, n, device, ctypes.byref(pp), ctypes.byref(pl), ctypes.byref(err))
    del keep
    _check(rc, err)
    out = _take_ptau(lib, pp, pl)
    if out_path is None:
        return out
    with open(out_path, "wb") as f:
        f.write(out)
    return out_path


def ptau_batch_top(level: int) -> int:
    """Tests: the highest level ptau_prepare_phase2 transforms together with the levels below it
    on the device (nzcb_debug_ptau_batch_top; < 0 restores the library's constant). Returns the
    previous value."""
    return load().nzcb_debug_ptau_batch_top(level)


def ptau_timings() -> list:
    """Milliseconds of this thread's last ptau_contribute or ptau_prepare_phase2: the kernels (HIP
    events), the call (nzcb_debug_ptau_timings)."""
    ms = (c_double * 2)()
    k = load().nzcb_debug_ptau_timings(ms, 2)
    return list(ms[:k])


def _read_if_path(x):
    if _is_path(x):
        with open(x, "rb") as f:
            return f.read()
    return x


def groth16_setup(r1cs_or_path, ptau_or_path, out_path=None, device: int = 0):
    """snarkjs ``groth16 setup <r1cs> <ptau> <zkey>``: the Groth16 proving key of a circuit from a
    powers-of-tau file that ptau_prepare_phase2 prepared, every key point a sparse sum of
    coefficients times Lagrange points computed on GPU `device` (GROTH16_HOST: on the host;
    include/nzcb.h nzcb_groth16_setup, where the file layout is specified). A FRESH KEY HAS
    delta = gamma = 1: anyone can forge proofs under it until groth16_contribute has run. NO
    circuit hash and NO contribution records are written, so ``snarkjs zkey verify`` does not
    accept the key, and parity with snarkjs's bytes is unpinned. The inputs are bytes or paths
    (memory-mapped when both are paths and `out_path` is given). Returns the bytes, or writes
    `out_path` and returns it."""
    lib = load()
    err = _Err()
    if _is_path(r1cs_or_path) and _is_path(ptau_or_path) and out_path is not None:
        _check(lib.nzcb_groth16_setup_file(os.fsencode(r1cs_or_path), os.fsencode(ptau_or_path),
                                           os.fsencode(out_path), device, ctypes.byref(err)), err)
        return out_path
    rp, rn, keep_r = _host_view(_read_if_path(r1cs_or_path))
    pp_, pn, keep_p = _host_view(_read_if_path(ptau_or_path))
    zp, zl = POINTER(c_uint8)(), c_size_t()
    rc = lib.nzcb_groth16_setup(rp, rn, pp_, pn, device, ctypes.byref(zp), ctypes.byref(zl), ctypes.byref(err))
    del keep_r, keep_p
    _check(rc, err)
    out = _take_ptau(lib, zp, zl)
    if out_path is None:
        return out
    with open(out_path, "wb") as f:
        f.write(out)
    return out_path


def groth16_contribute(zkey_or_path, out_path=None, secret=None, entropy=None, device: int = 0):
    """snarkjs ``zkey contribute``: multiply your own secret d into a Groth16 key on GPU `device`
    (GROTH16_HOST: on the host): delta1 and delta2 by d, C and H by 1/d; everything else is copied
    (include/nzcb.h nzcb_groth16_contribute). secret = None draws d from the OS CSPRNG, mixed with
    the optional `entropy` (str or bytes); an integer in [1, r) is FOR REPRODUCIBLE TESTS ONLY.
    The points of C and H and the two deltas are tested first; a bad one raises NzcbError FORMAT
    naming its section and index. NO contribution record is written: ``snarkjs zkey verify`` does
    not accept the output. The input is bytes, or a path (memory-mapped when `out_path` is given).
    Returns the bytes, or writes `out_path` and returns it."""
    lib = load()
    err = _Err()
    sec = None
    if secret is not None:
        if not 0 <= int(secret) < 1 << 256:
            raise NzcbError(1, "zkey: a secret is zero or not below r")
        sec = _buf(int(secret).to_bytes(32, "little"))
    ent = entropy.encode() if isinstance(entropy, str) else bytes(entropy or b"")
    if _is_path(zkey_or_path) and out_path is not None:
        _check(lib.nzcb_groth16_contribute_file(os.fsencode(zkey_or_path), os.fsencode(out_path), sec, ent, len(ent),
                                                device, ctypes.byref(err)), err)
        return out_path
    ptr, n, keep = _host_view(_read_if_path(zkey_or_path))
    zp, zl = POINTER(c_uint8)(), c_size_t()
    rc = lib.nzcb_groth16_contribute(ptr, n, sec, ent, len(ent), device, ctypes.byref(zp), ctypes.byref(zl),
                                     ctypes.byref(err))
    del keep
    _check(rc, err)
    out = _take_ptau(lib, zp, zl)
    if out_path is None:
        return out
    with open(out_path, "wb") as f:
        f.write(out)
    return out_path


def groth16_vk(zkey_or_path) -> dict:
    """snarkjs ``zkey export verificationkey`` for a Groth16 key (bytes, or a path, which is
    memory-mapped): protocol, curve, nPublic, vk_alpha_1, vk_beta_2, vk_gamma_2, vk_delta_2, IC
    (include/nzcb.h nzcb_groth16_vk_to_json). snarkjs's vk_alphabeta_12 is left out."""
    lib = load()
    if _is_path(zkey_or_path):
        def call(out, cap):
            return lib.nzcb_groth16_vk_to_json_file(os.fsencode(zkey_or_path), out, cap)
    else:
        ptr, n, keep = _host_view(zkey_or_path)

        def call(out, cap):
            return lib.nzcb_groth16_vk_to_json(ptr, n, out, cap)
    out = ctypes.create_string_buffer(256)
    rc = call(out, 256)
    if rc < 0:
        out = ctypes.create_string_buffer(-rc)
        rc = call(out, -rc)
    if rc != 0:
        raise NzcbError(rc, out.value.decode(errors="replace"))
    return json.loads(out.value.decode())


def groth16_rows(points: bytes, row_off, idx, coefs, g2: bool = False, device: int = 0) -> list:
    """Tests: the kernel family of groth16_setup on bare arrays (nzcb_engine_groth16_rows). points:
    LEM affine points back to back (64 B each, 128 B with g2); row r is the sum over t in
    [row_off[r], row_off[r + 1]) of coefs[t] * points[idx[t]], coefs integers in [0, r). Returns
    one LEM affine point per row (zero bytes: the point at infinity). On a GPU the points are
    uploaded first, as the entry point reads them from device memory."""
    lib = load()
    w = 128 if g2 else 64
    n_points, n_rows, n_terms = len(points) // w, len(row_off) - 1, len(idx)
    ro = (ctypes.c_uint64 * (n_rows + 1))(*row_off)
    ix = (c_uint32 * max(n_terms, 1))(*idx)
    cf = _buf(b"".join(int(c).to_bytes(32, "little") for c in coefs))
    out = _out(w * n_rows)
    err = _Err()
    if device == GROTH16_HOST:
        src = _buf(points)
        rc = lib.nzcb_engine_groth16_rows(device, int(g2), ctypes.cast(src, c_void_p), n_points, ro, n_rows, ix, cf,
                                          out, ctypes.byref(err))
    else:
        d_pts = lib.nzcb_dev_alloc_on(device, max(len(points), 4))
        if not d_pts:
            raise NzcbError(10, "hipMalloc failed")
        try:
            if points:
                h2d(d_pts, points)
            rc = lib.nzcb_engine_groth16_rows(device, int(g2), d_pts, n_points, ro, n_rows, ix, cf, out,
                                              ctypes.byref(err))
        finally:
            lib.nzcb_dev_free(d_pts)
    _check(rc, err)
    return [bytes(out[w * i:w * i + w]) for i in range(n_rows)]


def groth16_schedule(chunk: int, fan_in: int) -> tuple:
    """Tests: the longest chunk of a row one lane sums and the fan-in of the folds that follow, for
    the calls after this one (nzcb_debug_groth16_schedule; <= 0 restores the library's constant).
    Returns the previous (chunk, fan_in). The bytes of a key do not depend on them."""
    pc, pf = c_int(), c_int()
    rc = load().nzcb_debug_groth16_schedule(chunk, fan_in, ctypes.byref(pc), ctypes.byref(pf))
    if rc != 0:
        raise NzcbError(rc, "groth16: chunk length in 1..1024 and fan-in in 2..1024")
    return pc.value, pf.value


GROTH16_TIMING_NAMES = ("kernels_ms", "call_ms", "rows_g1_ms", "rows_g2_ms", "tests_ms", "scale_ms", "plan_ms",
                        "terms_A", "terms_B1", "terms_B2", "terms_K", "chunks_g1", "chunks_g2")


def groth16_timings() -> dict:
    """This thread's last groth16_setup, groth16_contribute or groth16_rows: kernel milliseconds
    (HIP events) by step, the call's wall time, and the term and chunk counts
    (nzcb_debug_groth16_timings)."""
    v = (c_double * len(GROTH16_TIMING_NAMES))()
    k = load().nzcb_debug_groth16_timings(v, len(GROTH16_TIMING_NAMES))
    return dict(zip(GROTH16_TIMING_NAMES[:k], v[:k]))


def synth_setup_raw(power: int, n_public: int = 3, n_inputs: int = 8, seed: int = 0x6E7A6362,
                    n_constraints: int = 0, tau: int = 0x6E7A6362746175, device: int = 0, free_public: bool = False):
    """Like synth_setup but returns library-owned host buffers (zkey_ptr, zkey_len, wtns_ptr, wtns_len)
    without copying them into Python; release with free_raw()."""
    zp, zl, wp, wl = _synth_raw(power, n_public, n_inputs, seed, n_constraints, tau, device, free_public)
    return (ctypes.cast(zp, c_void_p).value, zl, ctypes.cast(wp, c_void_p).value, wl)


def free_raw(raw):
    lib = load()
    lib.nzcb_free(raw[0])
    lib.nzcb_free(raw[2])
