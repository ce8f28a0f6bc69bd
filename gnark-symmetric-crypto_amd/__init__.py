"""gnark-symmetric-crypto_amd — MI355X-native Groth16 prover behind the reference's libprove C-ABI.

This package is only the Python-side loader of ``libprove.so`` (built from ``csrc/`` by ``csrc/Makefile``)
plus thin helpers that call it exactly the way a foreign-function host (node.js / Go cgo) would:
``GoSlice`` arguments by value, ``struct Prove_return`` results released with ``Free``
(reference: libraries/prover/libprove.go:17-47).  There is no Python or CPU implementation of the prover
here: if the shared library or a GPU is missing, calls fail loudly.
"""
import ctypes as C
import json
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libprove.so")
VERIFY_LIB_PATH = os.path.join(_HERE, "libverify.so")
CSRC = os.path.join(_HERE, "csrc")

CHACHA20, AES_128, AES_256 = 0, 1, 2                       # prove_impl.go:15-19
ALGORITHM_NAMES = {0: "chacha20", 1: "aes-128-ctr", 2: "aes-256-ctr"}   # prove_impl.go:21-25

EXPORTS = ["enforce_binding", "InitAlgorithm", "Free", "Prove", "ProveBatch", "gsc_prove_raw", "gsc_setup",
           "gsc_set_deterministic_randomness", "gsc_debug_prove", "gsc_debug_vector", "gsc_describe", "gsc_last_stage_ms", "gsc_last_dominant_kernel", "gsc_last_kernel_clock", "gsc_debug_field_ops", "gsc_debug_limb_ops", "gsc_debug_curve_ops", "gsc_debug_decode_points", "gsc_debug_tower_ops", "gsc_debug_compute_h", "gsc_debug_compute_d", "gsc_debug_z_sum", "gsc_debug_quot_fold_dft", "gsc_debug_secret_residue", "gsc_debug_secret_scan", "gsc_debug_wipe", "gsc_debug_clock_trace", "gsc_debug_glv_split",
           "gsc_verify_init", "gsc_verify_raw", "VerifyBatch", "gsc_debug_pairing",
           "gsc_verify_raw_batched", "gsc_verify_all", "VerifyAll", "gsc_debug_verify_randomizers",
           "gsc_verify_json", "gsc_verify_last_path", "gsc_debug_verify_path", "gsc_debug_pairing_few",
           "gsc_verify_claims", "VerifyClaims",
           "gsc_prove_check_init", "gsc_prove_check_stats", "gsc_debug_prove_corrupt",
           "gsc_release_algorithm", "gsc_replace_algorithm", "gsc_memory_info", "gsc_key_generation",
           "gsc_setup_contribute", "gsc_setup_verify_contribution", "gsc_debug_scale_points",
           "gsc_pedersen_verify", "gsc_setup_contribute_sigma", "gsc_setup_verify_sigma_contribution", "gsc_setup_verify_from_srs",
           "gsc_srs_verify", "gsc_debug_srs_generate", "gsc_debug_group_idft", "gsc_debug_column_sums", "gsc_setup_from_srs", "gsc_debug_msm", "gsc_debug_solve", "gsc_debug_assemble", "gsc_debug_quotient", "gsc_debug_verify_g1",
           "gsc_srs_initial", "gsc_srs_contribute", "gsc_srs_verify_contribution", "gsc_debug_scale_powers"]


class GoSlice(C.Structure):
    _fields_ = [("data", C.c_void_p), ("len", C.c_longlong), ("cap", C.c_longlong)]


class DebugMsmArgs(C.Structure):      # struct gsc_debug_msm_args of include/libprove.h
    _fields_ = [("group", C.c_int32), ("nbases", C.c_uint32),
                ("points", C.c_char_p), ("kind", C.c_char_p), ("rowlen", C.c_void_p), ("rows", C.c_void_p),
                ("n_rows", C.c_uint32), ("zero_row", C.c_uint32),
                ("c", C.c_int32), ("cv", C.c_int32), ("mont", C.c_int32),
                ("batch", C.c_uint32), ("nproofs", C.c_uint32), ("per_flat", C.c_uint32), ("per_win", C.c_uint32), ("digit_bases", C.c_uint32),
                ("digit_rows", C.c_void_p), ("scalars_be", C.c_char_p),
                ("plane", C.c_char_p), ("plane_rows", C.c_uint32), ("plane_stride", C.c_uint32),
                ("out", C.c_void_p), ("out_inf", C.c_void_p),
                ("flat_digits", C.c_void_p), ("flat_digits_cap", C.c_size_t), ("win_digits", C.c_void_p), ("win_digits_cap", C.c_size_t),
                ("gok", C.c_void_p), ("gok_cap", C.c_size_t), ("group_ok", C.c_void_p), ("group_ok_cap", C.c_size_t),
                ("info", C.c_void_p)]


class DebugSolveArgs(C.Structure):      # struct gsc_debug_solve_args of include/libprove.h
    _fields_ = [("n_public", C.c_uint32), ("n_secret", C.c_uint32), ("n_internal", C.c_uint32), ("n_constraints", C.c_uint32),
                ("calldata", C.c_void_p), ("n_calldata", C.c_uint32),
                ("blueprint", C.c_void_p), ("constraint_off", C.c_void_p), ("wire_off", C.c_void_p), ("n_instr", C.c_uint32),
                ("bp_kind", C.c_char_p), ("bp_entries", C.c_void_p), ("bp_entries_len", C.c_void_p), ("n_blueprints", C.c_uint32),
                ("coeff", C.c_void_p), ("n_coeff", C.c_uint32),
                ("has_commitment", C.c_int32), ("commit_wire", C.c_uint32), ("commit_private", C.c_void_p), ("n_commit_private", C.c_uint32),
                ("in_W", C.c_char_p), ("mask", C.c_char_p), ("commit", C.c_char_p),
                ("batch", C.c_uint32), ("nproofs", C.c_uint32), ("workgroups", C.c_uint32), ("mode", C.c_int32),
                ("class_w", C.c_char_p), ("class_a", C.c_char_p), ("class_b", C.c_char_p), ("class_c", C.c_char_p),
                ("fill", C.c_uint32),
                ("W", C.c_void_p), ("W_cap", C.c_size_t), ("A", C.c_void_p), ("A_cap", C.c_size_t), ("B", C.c_void_p), ("B_cap", C.c_size_t), ("C", C.c_void_p), ("C_cap", C.c_size_t),
                ("status", C.c_void_p), ("flag", C.c_void_p), ("info", C.c_void_p), ("why", C.c_void_p)]


_ASSEMBLE_SETS = ("a", "b1", "k", "z", "b2", "c", "d", "pok")


class DebugAssembleArgs(C.Structure):      # struct gsc_debug_assemble_args of include/libprove.h
    _fields_ = [("batch", C.c_uint32), ("nproofs", C.c_uint32), ("n_wires", C.c_uint32), ("fill", C.c_uint32)] + \
               [(s + part, C.c_char_p) for s in _ASSEMBLE_SETS for part in ("_pts", "_inf", "_lam")] + \
               [("rs", C.c_char_p), ("mask", C.c_char_p), ("glv_in", C.c_char_p)] + \
               [(n, C.c_void_p) for n in ("out", "flags", "tmp", "tmp_inf", "cpts", "commit", "W", "mask_out", "glv")]


class DebugVerifyG1Args(C.Structure):      # struct gsc_debug_verify_g1_args of include/libprove.h
    _fields_ = [("algorithm", C.c_uint32), ("path", C.c_uint32), ("fill", C.c_uint32), ("vk", C.c_char_p), ("vk_len", C.c_size_t),
                ("n", C.c_size_t), ("proofs", C.c_char_p), ("lens", C.c_void_p), ("signals", C.c_char_p), ("rnd", C.c_void_p),
                ("np", C.c_size_t), ("ends", C.c_void_p), ("key_status", C.c_void_p), ("key_status_cap", C.c_size_t)] + \
               [(n, C.c_void_p) for n in ("table", "ctable", "ok", "g1", "g2", "okv", "fixed", "flag", "pfixed", "prho", "pflag")]


class DebugQuotientArgs(C.Structure):      # struct gsc_debug_quotient_args of include/libprove.h
    _fields_ = [("algorithm", C.c_uint32), ("plain", C.c_int32), ("c", C.c_int32),
                ("mats_be", C.c_void_p), ("m", C.c_size_t), ("planes", C.c_void_p),
                ("ncols", C.c_size_t), ("live", C.c_size_t), ("out", C.c_void_p), ("cap", C.c_size_t)]


class ProveReturn(C.Structure):
    _fields_ = [("r0", C.c_void_p), ("r1", C.c_longlong)]


def build(jobs=8):
    """Compile csrc/ into libprove.so for gfx950 (hipcc cross-compiles without a GPU)."""
    subprocess.check_call(["make", "-C", CSRC, "-j%d" % jobs], stdout=subprocess.DEVNULL)
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libprove.so is not built: run gnark-symmetric-crypto_amd.build() (make -C %s)" % CSRC)
        L = C.CDLL(LIB_PATH)
        L.InitAlgorithm.restype = C.c_ubyte
        L.InitAlgorithm.argtypes = [C.c_ubyte, GoSlice, GoSlice]
        L.Free.argtypes = [C.c_void_p]
        L.Prove.restype = ProveReturn
        L.Prove.argtypes = [GoSlice]
        L.ProveBatch.restype = ProveReturn
        L.ProveBatch.argtypes = [GoSlice]
        L.gsc_prove_raw.restype = C.c_longlong
        L.gsc_prove_raw.argtypes = [C.c_ubyte, C.c_char_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
        L.gsc_setup.restype = C.c_int
        L.gsc_setup.argtypes = [GoSlice, C.c_char_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
        L.gsc_set_deterministic_randomness.restype = C.c_int
        L.gsc_set_deterministic_randomness.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p]
        L.gsc_debug_prove.restype = C.c_longlong
        L.gsc_debug_prove.argtypes = [GoSlice]
        L.gsc_debug_vector.restype = C.c_longlong
        L.gsc_debug_vector.argtypes = [C.c_int, C.c_void_p, C.c_size_t]
        L.gsc_describe.restype = C.c_size_t
        L.gsc_describe.argtypes = [C.c_ubyte, C.c_char_p, C.c_size_t]
        L.gsc_last_stage_ms.argtypes = [C.c_ubyte, C.POINTER(C.c_float)]
        L.gsc_last_dominant_kernel.restype = C.c_int
        L.gsc_last_dominant_kernel.argtypes = [C.c_ubyte, C.c_char_p, C.c_size_t, C.POINTER(C.c_float), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
        L.gsc_last_kernel_clock.restype = C.c_int
        L.gsc_last_kernel_clock.argtypes = [C.c_ubyte, C.POINTER(C.c_float), C.POINTER(C.c_int)]
        L.gsc_debug_field_ops.restype = C.c_int
        L.gsc_debug_field_ops.argtypes = [C.c_int, C.c_int, C.c_char_p, C.c_char_p, C.c_void_p, C.c_size_t, C.c_int]
        L.gsc_debug_limb_ops.restype = C.c_int
        L.gsc_debug_limb_ops.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        L.gsc_debug_tower_ops.restype = C.c_int
        L.gsc_debug_tower_ops.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.gsc_debug_curve_ops.restype = C.c_int
        L.gsc_debug_curve_ops.argtypes = [C.c_int, C.c_int, C.c_char_p, C.c_char_p, C.c_char_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p]
        L.gsc_verify_init.restype = C.c_int
        L.gsc_verify_init.argtypes = [C.c_ubyte, GoSlice]
        L.gsc_verify_raw.restype = C.c_longlong
        L.gsc_verify_raw.argtypes = [C.c_ubyte, C.c_char_p, C.c_void_p, C.c_char_p, C.c_size_t, C.c_void_p]
        L.VerifyBatch.restype = ProveReturn
        L.VerifyBatch.argtypes = [GoSlice]
        L.gsc_debug_pairing.restype = C.c_longlong
        L.gsc_debug_pairing.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t, C.c_void_p]
        L.gsc_verify_raw_batched.restype = C.c_longlong
        L.gsc_verify_raw_batched.argtypes = [C.c_ubyte, C.c_char_p, C.c_void_p, C.c_char_p, C.c_size_t, C.c_void_p]
        L.gsc_verify_all.restype = C.c_int
        L.gsc_verify_all.argtypes = [C.c_ubyte, C.c_char_p, C.c_void_p, C.c_char_p, C.c_size_t]
        L.VerifyAll.restype = C.c_ubyte
        L.VerifyAll.argtypes = [GoSlice]
        L.gsc_debug_verify_randomizers.restype = C.c_int
        L.gsc_debug_verify_randomizers.argtypes = [C.c_char_p, C.c_int]
        L.gsc_verify_json.restype = C.c_ubyte
        L.gsc_verify_json.argtypes = [GoSlice]
        L.gsc_verify_last_path.restype = C.c_int
        L.gsc_verify_last_path.argtypes = [C.c_ubyte]
        L.gsc_debug_verify_path.restype = C.c_int
        L.gsc_debug_verify_path.argtypes = [C.c_int]
        L.gsc_debug_pairing_few.restype = C.c_longlong
        L.gsc_debug_pairing_few.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t, C.c_void_p]
        L.gsc_verify_claims.restype = C.c_longlong
        L.gsc_verify_claims.argtypes = [C.c_ubyte, C.c_char_p, C.c_void_p, C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
        L.VerifyClaims.restype = ProveReturn
        L.VerifyClaims.argtypes = [GoSlice]
        L.gsc_prove_check_init.restype = C.c_int
        L.gsc_prove_check_init.argtypes = [C.c_ubyte, GoSlice]
        L.gsc_prove_check_stats.restype = C.c_int
        L.gsc_prove_check_stats.argtypes = [C.c_ubyte, C.POINTER(C.c_uint64)]
        L.gsc_debug_prove_corrupt.restype = C.c_int
        L.gsc_debug_prove_corrupt.argtypes = [C.c_ubyte, C.c_uint32, C.c_int, C.c_int]
        L.gsc_release_algorithm.restype = C.c_ubyte
        L.gsc_release_algorithm.argtypes = [C.c_ubyte]
        L.gsc_replace_algorithm.restype = C.c_int
        L.gsc_replace_algorithm.argtypes = [C.c_ubyte, GoSlice, GoSlice, GoSlice]
        L.gsc_memory_info.restype = C.c_int
        L.gsc_memory_info.argtypes = [C.c_int, C.POINTER(C.c_uint64)]
        L.gsc_key_generation.restype = C.c_uint64
        L.gsc_key_generation.argtypes = [C.c_ubyte]
        L.gsc_setup_contribute.restype = C.c_int
        L.gsc_setup_contribute.argtypes = [GoSlice, GoSlice, C.c_char_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_void_p]
        L.gsc_setup_verify_contribution.restype = C.c_int
        L.gsc_setup_verify_contribution.argtypes = [GoSlice, GoSlice, GoSlice, GoSlice, C.c_char_p]
        L.gsc_debug_scale_points.restype = C.c_int
        L.gsc_debug_scale_points.argtypes = [C.c_int, C.c_char_p, C.c_char_p, C.c_size_t, C.c_char_p, C.c_void_p, C.c_void_p]
        L.gsc_pedersen_verify.restype = C.c_int
        L.gsc_pedersen_verify.argtypes = [GoSlice, GoSlice]
        L.gsc_setup_contribute_sigma.restype = C.c_int
        L.gsc_setup_contribute_sigma.argtypes = [GoSlice, GoSlice, C.c_char_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_void_p]
        L.gsc_setup_verify_sigma_contribution.restype = C.c_int
        L.gsc_setup_verify_sigma_contribution.argtypes = [GoSlice, GoSlice, GoSlice, GoSlice, C.c_char_p]
        L.gsc_setup_verify_from_srs.restype = C.c_int
        L.gsc_setup_verify_from_srs.argtypes = [GoSlice, GoSlice, GoSlice, GoSlice]
        L.gsc_srs_verify.restype = C.c_int
        L.gsc_srs_verify.argtypes = [GoSlice]
        L.gsc_debug_srs_generate.restype = C.c_int
        L.gsc_debug_srs_generate.argtypes = [C.c_int, C.c_char_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
        L.gsc_srs_initial.restype = C.c_int
        L.gsc_srs_initial.argtypes = [C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
        L.gsc_srs_contribute.restype = C.c_int
        L.gsc_srs_contribute.argtypes = [GoSlice, C.c_char_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_void_p]
        L.gsc_srs_verify_contribution.restype = C.c_int
        L.gsc_srs_verify_contribution.argtypes = [GoSlice, GoSlice, C.c_char_p]
        L.gsc_debug_scale_powers.restype = C.c_int
        L.gsc_debug_scale_powers.argtypes = [C.c_int, C.c_char_p, C.c_char_p, C.c_size_t, C.c_char_p, C.c_char_p, C.c_uint64, C.c_void_p, C.c_void_p]
        L.gsc_setup_from_srs.restype = C.c_int
        L.gsc_setup_from_srs.argtypes = [GoSlice, GoSlice, C.c_char_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
        L.gsc_debug_group_idft.restype = C.c_int
        L.gsc_debug_group_idft.argtypes = [C.c_int, C.c_int, C.c_char_p, C.c_void_p, C.c_void_p]
        L.gsc_debug_msm.restype = C.c_int
        L.gsc_debug_msm.argtypes = [C.POINTER(DebugMsmArgs)]
        L.gsc_debug_solve.restype = C.c_int
        L.gsc_debug_solve.argtypes = [C.POINTER(DebugSolveArgs)]
        L.gsc_debug_verify_g1.restype = C.c_int
        L.gsc_debug_verify_g1.argtypes = [C.POINTER(DebugVerifyG1Args)]
        L.gsc_debug_assemble.restype = C.c_int
        L.gsc_debug_assemble.argtypes = [C.POINTER(DebugAssembleArgs)]
        L.gsc_debug_quotient.restype = C.c_longlong
        L.gsc_debug_quotient.argtypes = [C.POINTER(DebugQuotientArgs)]
        L.gsc_debug_column_sums.restype = C.c_int
        L.gsc_debug_column_sums.argtypes = [C.c_int, C.c_uint32, C.c_char_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_char_p, C.c_void_p, C.c_void_p]
        L.enforce_binding()
        _lib = L
    return _lib


def _slice(b: bytes):
    buf = C.create_string_buffer(b, len(b))
    return GoSlice(C.cast(buf, C.c_void_p), len(b), len(b)), buf


def init_algorithm(algorithm_id: int, proving_key: bytes, r1cs: bytes) -> bool:
    """InitAlgorithm(algorithmID, provingKey, r1cs) — libprove.go:20-23."""
    s1, k1 = _slice(proving_key)
    s2, k2 = _slice(r1cs)
    return bool(lib().InitAlgorithm(algorithm_id, s1, s2))


def release_algorithm(algorithm_id: int) -> bool:
    """gsc_release_algorithm: takes the algorithm out, waits for the calls in flight and frees the engine with all its device memory.
    False: it was not initialised."""
    return bool(lib().gsc_release_algorithm(algorithm_id))


def replace_algorithm(algorithm_id: int, proving_key: bytes, r1cs: bytes, verifying_key: bytes = b"") -> int:
    """gsc_replace_algorithm: a new engine from (proving_key, r1cs) built beside the serving one, swapped in, the old one drained and freed.
    1 swapped; 0 refused (a line on stdout; the old key keeps serving); -1 the algorithm is not initialised.  verifying_key: the self-check of
    the new engine is on under it (b"": off, or as GSC_PROVE_CHECK says)."""
    s1, k1 = _slice(proving_key)
    s2, k2 = _slice(r1cs)
    s3, k3 = _slice(verifying_key) if verifying_key else (GoSlice(None, 0, 0), None)
    return int(lib().gsc_replace_algorithm(algorithm_id, s1, s2, s3))


def memory_info(device: int = 0):
    """gsc_memory_info: {"free", "total", "provers", "verifiers"} in bytes for one device; None for a device that does not exist."""
    out = (C.c_uint64 * 4)()
    if lib().gsc_memory_info(device, out) != 0:
        return None
    return dict(zip(("free", "total", "provers", "verifiers"), (int(v) for v in out)))


def key_generation(algorithm_id: int) -> int:
    """gsc_key_generation: 0 not initialised, 1 after InitAlgorithm, +1 per successful replace_algorithm."""
    return int(lib().gsc_key_generation(algorithm_id))


def key_id(algorithm_id: int):
    """The key= field of gsc_describe (first 16 hex digits of SHA-256 of the proving key's bytes); None when not initialised."""
    d = describe(algorithm_id)
    return d.split(" key=")[1].split()[0] if " key=" in d else None


def _take(ret: ProveReturn) -> bytes:
    if not ret.r0:
        return b""
    out = C.string_at(ret.r0, ret.r1)
    lib().Free(ret.r0)
    return out


def prove(params) -> bytes:
    """Prove(params) — libprove.go:30-47.  params: bytes/str JSON or a dict.  Returns the raw JSON bytes."""
    if isinstance(params, dict):
        params = json.dumps(params)
    if isinstance(params, str):
        params = params.encode()
    s, keep = _slice(params)
    return _take(lib().Prove(s))


def prove_batch(params_list) -> list:
    """ProveBatch (addition): list of dicts -> list of decoded JSON results."""
    s, keep = _slice(json.dumps(params_list).encode())
    return json.loads(_take(lib().ProveBatch(s)))


def setup(r1cs: bytes, seed: bytes = None):
    """gsc_setup: Groth16 Setup for an R1CS file -> (pk bytes, vk bytes) in gnark's layouts.  seed (32 bytes) makes TEST keys and
    needs the test hooks; None = CSPRNG toxic waste."""
    s, keep = _slice(r1cs)
    pk, vk, npk, nvk = C.c_void_p(), C.c_void_p(), C.c_size_t(), C.c_size_t()
    if lib().gsc_setup(s, seed, C.byref(pk), C.byref(npk), C.byref(vk), C.byref(nvk)) != 0:
        raise RuntimeError("gsc_setup failed (see stdout)")
    out = C.string_at(pk.value, npk.value), C.string_at(vk.value, nvk.value)
    lib().Free(pk); lib().Free(vk)
    return out


def prove_batch_bytes(params_json: bytes) -> bytes:
    """ProveBatch on an already encoded JSON array; returns the raw JSON bytes (bench.py keeps JSON work off the timed path)."""
    s, keep = _slice(params_json)
    return _take(lib().ProveBatch(s))


CONTRIBUTION_BYTES = 224


def setup_contribute(pk: bytes, vk: bytes, seed: bytes = None):
    """gsc_setup_contribute: one contribution to the second phase of the key ceremony (include/libprove.h) -> (pk', vk', record).  seed
    (32 bytes) fixes the secrets and needs the test hooks; None = the OS CSPRNG.  Raises RuntimeError with the return code (-1 seed without
    hooks, -2 refused keys, -3 device error; the reason is on stdout)."""
    s1, k1 = _slice(pk)
    s2, k2 = _slice(vk)
    p, v, np_, nv = C.c_void_p(), C.c_void_p(), C.c_size_t(), C.c_size_t()
    rec = C.create_string_buffer(CONTRIBUTION_BYTES)
    rc = lib().gsc_setup_contribute(s1, s2, seed, C.byref(p), C.byref(np_), C.byref(v), C.byref(nv), rec)
    if rc != 0:
        raise RuntimeError("gsc_setup_contribute failed: %d (see stdout)" % rc)
    out = C.string_at(p.value, np_.value), C.string_at(v.value, nv.value), rec.raw
    lib().Free(p); lib().Free(v)
    return out


def setup_verify_contribution(pk_prev: bytes, vk_prev: bytes, pk_next: bytes, vk_next: bytes, record: bytes) -> bool:
    """gsc_setup_verify_contribution: is (pk_next, vk_next) a contribution to (pk_prev, vk_prev) that `record` proves?  A refusal names its
    rule on stdout.  Raises RuntimeError on a device error."""
    if len(record) != CONTRIBUTION_BYTES:
        return False
    keep = [_slice(b) for b in (pk_prev, vk_prev, pk_next, vk_next)]
    rc = lib().gsc_setup_verify_contribution(keep[0][0], keep[1][0], keep[2][0], keep[3][0], record)
    if rc < 0:
        raise RuntimeError("gsc_setup_verify_contribution: device error (%d)" % rc)
    return rc == 1


SIGMA_CONTRIBUTION_BYTES = 224


def pedersen_verify(pk: bytes, vk: bytes) -> bool:
    """gsc_pedersen_verify: does the pair's one commitment key hold the Pedersen relation e(BasisExpSigma_j, G) e(Basis_j, GSigmaNeg) = 1?  A
    refusal names its rule on stdout (a pair without a commitment key: rule 1).  Raises RuntimeError on a device error."""
    s1, k1 = _slice(pk)
    s2, k2 = _slice(vk)
    rc = lib().gsc_pedersen_verify(s1, s2)
    if rc < 0:
        raise RuntimeError("gsc_pedersen_verify: device error (%d)" % rc)
    return rc == 1


def setup_contribute_sigma(pk: bytes, vk: bytes, seed: bytes = None):
    """gsc_setup_contribute_sigma: one contribution to the Pedersen sigma of a key pair with a commitment (include/libprove.h) -> (pk', vk',
    record).  seed (32 bytes) fixes the secrets and needs the test hooks; None = the OS CSPRNG.  Raises RuntimeError with the return code
    (-1 seed without hooks, -2 refused keys, -3 device error; the reason is on stdout)."""
    s1, k1 = _slice(pk)
    s2, k2 = _slice(vk)
    p, v, np_, nv = C.c_void_p(), C.c_void_p(), C.c_size_t(), C.c_size_t()
    rec = C.create_string_buffer(SIGMA_CONTRIBUTION_BYTES)
    rc = lib().gsc_setup_contribute_sigma(s1, s2, seed, C.byref(p), C.byref(np_), C.byref(v), C.byref(nv), rec)
    if rc != 0:
        raise RuntimeError("gsc_setup_contribute_sigma failed: %d (see stdout)" % rc)
    out = C.string_at(p.value, np_.value), C.string_at(v.value, nv.value), rec.raw
    lib().Free(p); lib().Free(v)
    return out


def setup_verify_sigma_contribution(pk_prev: bytes, vk_prev: bytes, pk_next: bytes, vk_next: bytes, record: bytes) -> bool:
    """gsc_setup_verify_sigma_contribution: is (pk_next, vk_next) a sigma contribution to (pk_prev, vk_prev) that `record` proves?  prev's own
    Pedersen relation is not re-checked: a chain starts from a pair that passed pedersen_verify or setup_verify_from_srs.  A refusal names its
    rule on stdout.  Raises RuntimeError on a device error."""
    if len(record) != SIGMA_CONTRIBUTION_BYTES:
        return False
    keep = [_slice(b) for b in (pk_prev, vk_prev, pk_next, vk_next)]
    rc = lib().gsc_setup_verify_sigma_contribution(keep[0][0], keep[1][0], keep[2][0], keep[3][0], record)
    if rc < 0:
        raise RuntimeError("gsc_setup_verify_sigma_contribution: device error (%d)" % rc)
    return rc == 1


def setup_verify_from_srs(r1cs: bytes, srs: bytes, pk: bytes, vk: bytes) -> bool:
    """gsc_setup_verify_from_srs: is (pk, vk) what setup_from_srs makes of (r1cs, srs) — byte for byte outside the commitment key's sigma and g,
    which every run draws afresh, and with the Pedersen relation on those?  A refusal names its rule on stdout.  Raises RuntimeError with the
    return code (-2 refused r1cs / file / L too small, -3 device error)."""
    keep = [_slice(b) for b in (r1cs, srs, pk, vk)]
    rc = lib().gsc_setup_verify_from_srs(keep[0][0], keep[1][0], keep[2][0], keep[3][0])
    if rc < 0:
        raise RuntimeError("gsc_setup_verify_from_srs failed: %d (see stdout)" % rc)
    return rc == 1


def debug_scale_points(group: int, pts: bytes, inf: bytes, scalar: int):
    """TEST HOOK: scalar * P for raw big-endian points (64 B in G1, 128 B in G2) through k_scale_points -> (points, infinity flags)."""
    w = 64 if group == 0 else 128
    n = len(inf)
    assert len(pts) == w * n
    out, oinf = C.create_string_buffer(max(1, w * n)), C.create_string_buffer(max(1, n))
    if lib().gsc_debug_scale_points(group, pts, inf, n, int(scalar).to_bytes(32, "big"), out, oinf) != 0:
        raise RuntimeError("gsc_debug_scale_points failed (see stdout)")
    return out.raw[:w * n], oinf.raw[:n]


def srs_verify(srs: bytes) -> bool:
    """gsc_srs_verify: is `srs` a well-formed powers file (include/libprove.h: this project's own format) whose elements are the powers they
    claim to be?  A refusal names its rule on stdout.  Raises RuntimeError on a device error."""
    s, keep = _slice(srs)
    rc = lib().gsc_srs_verify(s)
    if rc < 0:
        raise RuntimeError("gsc_srs_verify: device error (%d)" % rc)
    return rc == 1


SRS_CONTRIBUTION_BYTES = 544


def srs_initial(L: int) -> bytes:
    """gsc_srs_initial: the ceremony's starting powers file for N = 2^L (tau = alpha = beta = 1: every element a generator).  Host only and
    deterministic.  Raises ValueError outside 1 <= L <= 24."""
    p, n = C.c_void_p(), C.c_size_t()
    if lib().gsc_srs_initial(L, C.byref(p), C.byref(n)) != 0:
        raise ValueError("gsc_srs_initial: L outside [1, 24]")
    out = C.string_at(p.value, n.value)
    lib().Free(p)
    return out


def srs_contribute(srs: bytes, seed: bytes = None):
    """gsc_srs_contribute: one contribution to a powers file (include/libprove.h) -> (srs', record).  seed (32 bytes) fixes the secrets and
    needs the test hooks; None = the OS CSPRNG.  Raises RuntimeError with the return code (-1 seed without hooks, -2 refused file, -3 device
    error; the reason is on stdout)."""
    s, keep = _slice(srs)
    p, n = C.c_void_p(), C.c_size_t()
    rec = C.create_string_buffer(SRS_CONTRIBUTION_BYTES)
    rc = lib().gsc_srs_contribute(s, seed, C.byref(p), C.byref(n), rec)
    if rc != 0:
        raise RuntimeError("gsc_srs_contribute failed: %d (see stdout)" % rc)
    out = C.string_at(p.value, n.value), rec.raw
    lib().Free(p)
    return out


def srs_verify_contribution(prev: bytes, nxt: bytes, record: bytes) -> bool:
    """gsc_srs_verify_contribution: is `nxt` a contribution to `prev` that `record` proves, and a powers file?  `prev` is not checked in full: a
    chain is verified link by link from srs_initial(L).  A refusal names its rule on stdout.  Raises RuntimeError on a device error."""
    if len(record) != SRS_CONTRIBUTION_BYTES:
        return False
    s1, k1 = _slice(prev)
    s2, k2 = _slice(nxt)
    rc = lib().gsc_srs_verify_contribution(s1, s2, record)
    if rc < 0:
        raise RuntimeError("gsc_srs_verify_contribution: device error (%d)" % rc)
    return rc == 1


def debug_scale_powers(group: int, pts: bytes, inf: bytes, x: int, m: int, first: int = 0):
    """TEST HOOK: m * x^(first + i) * P_i for raw big-endian points (64 B in G1, 128 B in G2) through k_fr_powers and the per-point ladder ->
    (points, infinity flags)."""
    w = 64 if group == 0 else 128
    n = len(inf)
    assert len(pts) == w * n
    out, oinf = C.create_string_buffer(max(1, w * n)), C.create_string_buffer(max(1, n))
    if lib().gsc_debug_scale_powers(group, pts, inf, n, int(x).to_bytes(32, "big"), int(m).to_bytes(32, "big"), first, out, oinf) != 0:
        raise RuntimeError("gsc_debug_scale_powers failed (see stdout)")
    return out.raw[:w * n], oinf.raw[:n]


def setup_from_srs(r1cs: bytes, srs: bytes, seed: bytes = None):
    """gsc_setup_from_srs: Groth16 Setup from a powers file -> (pk, vk) with delta = gamma = 1: FORGEABLE until at least one
    setup_contribute.  seed (32 bytes) chooses gamma, delta, sigma, g as gsc_setup's seeded Setup does and needs the test hooks.  Raises
    RuntimeError with the return code (-1 seed without hooks, -2 refused r1cs / file / L too small, -3 device error; the reason is on stdout)."""
    s1, k1 = _slice(r1cs)
    s2, k2 = _slice(srs)
    pk, vk, npk, nvk = C.c_void_p(), C.c_void_p(), C.c_size_t(), C.c_size_t()
    rc = lib().gsc_setup_from_srs(s1, s2, seed, C.byref(pk), C.byref(npk), C.byref(vk), C.byref(nvk))
    if rc != 0:
        raise RuntimeError("gsc_setup_from_srs failed: %d (see stdout)" % rc)
    out = C.string_at(pk.value, npk.value), C.string_at(vk.value, nvk.value)
    lib().Free(pk); lib().Free(vk)
    return out


def debug_srs_generate(L: int, seed: bytes) -> bytes:
    """TEST HOOK: the powers file with N = 2^L for the tau, alpha, beta that gsc_setup derives from `seed` (32 bytes)."""
    assert len(seed) == 32
    p, n = C.c_void_p(), C.c_size_t()
    if lib().gsc_debug_srs_generate(L, seed, C.byref(p), C.byref(n)) != 0:
        raise RuntimeError("gsc_debug_srs_generate failed (see stdout)")
    out = C.string_at(p.value, n.value)
    lib().Free(p)
    return out


def debug_group_idft(group: int, L: int, pts: bytes):
    """TEST HOOK: out[j] = (1/n) sum_k w^(-jk) pts[k] over n = 2^L raw points (64 B in G1, 128 B in G2) -> (points, infinity flags)."""
    w, n = (64 if group == 0 else 128), 1 << L
    assert len(pts) == w * n
    out, oinf = C.create_string_buffer(w * n), C.create_string_buffer(n)
    if lib().gsc_debug_group_idft(group, L, pts, out, oinf) != 0:
        raise RuntimeError("gsc_debug_group_idft failed (see stdout)")
    return out.raw[:w * n], oinf.raw[:n]


def debug_column_sums(group: int, rows: bytes, columns, coeffs):
    """TEST HOOK: the column-sum kernels on a caller's matrix.  rows: raw points; columns: one list of (row, coefficient id) per column;
    coeffs: integers below r -> (points, infinity flags), one per column."""
    w = 64 if group == 0 else 128
    assert len(rows) % w == 0
    start, trow, tco = [0], [], []
    for col in columns:
        for r, c in col:
            trow.append(r); tco.append(c)
        start.append(len(trow))
    u32 = lambda v: (C.c_uint32 * max(1, len(v)))(*v)
    a_start, a_row, a_co = u32(start), u32(trow), u32(tco)
    cbe = b"".join(int(c).to_bytes(32, "big") for c in coeffs)
    n = len(columns)
    out, oinf = C.create_string_buffer(max(1, w * n)), C.create_string_buffer(max(1, n))
    if lib().gsc_debug_column_sums(group, len(rows) // w, rows, n, a_start, a_row, a_co, len(coeffs), cbe, out, oinf) != 0:
        raise RuntimeError("gsc_debug_column_sums failed (see stdout)")
    return out.raw[:w * n], oinf.raw[:n]


def debug_msm(group: int, points: bytes, kind, rowlen, rows, scalars, n_rows: int, zero_row: int, c: int, cv: int = 0, mont: int = 1, batch: int = 64,
              nproofs: int = 0, per_flat: int = 0, per_win: int = 0, digit_rows=None, plane: bytes = None, plane_rows: int = 0, plane_stride: int = 0):
    """TEST HOOK: the MSM kernels on a caller's bases (raw points; kind 0 bit / 1 narrow of rowlen entries / 2 wide; scalar row per base) and
    scalars (n_rows x batch integers below r, row-major); see gsc_debug_msm in include/libprove.h.  digit_rows: the rows the windowed digits
    are laid out for when that is more than the wide bases.  -> dict: out (canonical little-endian coordinates per column), inf, flat_digits,
    win_digits, gok, group_ok (bytes as the kernels store them) and info (64 integers)."""
    w = 64 if group == 0 else 128
    n = len(kind)
    assert len(points) == w * n and len(rowlen) == n and len(rows) == n and len(scalars) == n_rows * batch
    u32 = lambda v: (C.c_uint32 * max(1, len(v)))(*v)
    a_len, a_rows, a_drows = u32(rowlen), u32(rows), u32(digit_rows or [])
    sbe = b"".join(int(v).to_bytes(32, "big") for v in scalars)
    ncols = nproofs or batch
    nwide = sum(1 for k in kind if k == 2)
    # capacities from upper bounds: at most 9 window octets per wide base (cv = 4: 65 windows), 65 windows at c = 4, two words per digit octet at c = 17
    flat_cap = 16 * batch * ((n + 7) // 8 + 1 + 9 * nwide)
    win_cap = 16 * batch * 65 * ((max(nwide, len(digit_rows or [])) + 7) // 8) * (2 if c > 16 else 1)
    gok_cap, gr_cap = 32 * ((n + 7) // 8) + 1, (n + 7) // 8 + 1
    out, oinf = C.create_string_buffer(w * ncols), C.create_string_buffer(ncols)
    fd, wd, gk, gr = C.create_string_buffer(flat_cap), C.create_string_buffer(max(1, win_cap)), C.create_string_buffer(gok_cap), C.create_string_buffer(gr_cap)
    info = (C.c_uint32 * 64)()
    vp = lambda b: C.cast(b, C.c_void_p)
    args = DebugMsmArgs(group, n, points, bytes(kind), vp(a_len), vp(a_rows), n_rows, zero_row, c, cv, mont, batch, nproofs, per_flat, per_win,
                        len(digit_rows or []), vp(a_drows) if digit_rows else None, sbe, plane, plane_rows, plane_stride, vp(out), vp(oinf),
                        vp(fd), flat_cap, vp(wd), max(1, win_cap), vp(gk), gok_cap, vp(gr), gr_cap, vp(info))
    if lib().gsc_debug_msm(C.byref(args)) != 0:
        raise RuntimeError("gsc_debug_msm failed (see stdout)")
    info = list(info)
    return {"out": out.raw[:w * ncols], "inf": oinf.raw[:ncols], "flat_digits": fd.raw[:info[48]], "win_digits": wd.raw[:info[49]],
            "gok": gk.raw[:info[50]], "group_ok": gr.raw[:info[51]], "info": info}


def debug_solve(desc: dict, in_W: bytes, batch: int = 64, nproofs: int = 0, workgroups: int = 0, mode: int = 0, mask: bytes = None, commit: bytes = None,
                classes=None, fill: int = 0xA5, caps=None):
    """TEST HOOK: the witness solver kernels on a caller's constraint system; see gsc_debug_solve in include/libprove.h.  desc: the R1CS fields
    (n_public, n_secret, n_internal, n_constraints, calldata, blueprint, constraint_off, wire_off, bp_kind, bp_entries (one list per blueprint),
    coeff (Montgomery integers), has_commitment, commit_wire, commit_private); in_W / mask / commit: 32 little-endian bytes per Montgomery value,
    [wire][column]; classes: (class_w, class_a, class_b, class_c) for mode 1; caps: byte capacities of (W, A, B, C) when not the exact need.
    -> dict: rc, W, A, B, C (bytes as stored), status, flag, info (32 integers), why."""
    nw, nc = desc["n_public"] + desc["n_secret"] + desc["n_internal"], desc["n_constraints"]
    u32 = lambda v: (C.c_uint32 * max(1, len(v)))(*v)
    vp = lambda b: C.cast(b, C.c_void_p)
    cd, bp, co, wo = u32(desc["calldata"]), u32(desc["blueprint"]), u32(desc["constraint_off"]), u32(desc["wire_off"])
    ents = u32([w for e in desc["bp_entries"] for w in e]); elen = u32([len(e) for e in desc["bp_entries"]])
    coeff = b"".join(int(v).to_bytes(32, "little") for v in desc["coeff"])
    cbuf = C.create_string_buffer(coeff, max(1, len(coeff)))
    cpriv = u32(desc.get("commit_private") or [])
    assert len(in_W) == 32 * batch * (desc["n_public"] + desc["n_secret"])
    need = [32 * batch * nw] + [32 * batch * nc] * 3
    caps = list(caps or need)
    bufs = [C.create_string_buffer(max(1, c)) for c in caps]
    status, flag, info, why = (C.c_uint32 * batch)(), (C.c_uint32 * 1)(), (C.c_uint32 * 32)(), C.create_string_buffer(128)
    cls = [bytes(c) for c in classes] if classes else [None] * 4
    args = DebugSolveArgs(desc["n_public"], desc["n_secret"], desc["n_internal"], nc, vp(cd), len(desc["calldata"]), vp(bp), vp(co), vp(wo), len(desc["blueprint"]),
                          bytes(desc["bp_kind"]), vp(ents), vp(elen), len(desc["bp_kind"]), vp(cbuf), len(desc["coeff"]),
                          1 if desc.get("has_commitment") else 0, desc.get("commit_wire", 0), vp(cpriv), len(desc.get("commit_private") or []),
                          in_W, mask, commit, batch, nproofs, workgroups, mode, cls[0], cls[1], cls[2], cls[3], fill,
                          vp(bufs[0]), caps[0], vp(bufs[1]), caps[1], vp(bufs[2]), caps[2], vp(bufs[3]), caps[3], vp(status), vp(flag), vp(info), vp(why))
    rc = lib().gsc_debug_solve(C.byref(args))
    return {"rc": rc, "W": bufs[0].raw[:need[0]], "A": bufs[1].raw[:need[1]], "B": bufs[2].raw[:need[2]], "C": bufs[3].raw[:need[3]],
            "status": list(status), "flag": flag[0], "info": list(info), "why": why.value.decode("utf-8", "replace")}


def debug_assemble(batch: int, sets: dict, rs: bytes, nproofs: int = 0, mask: bytes = None, n_wires: int = 3, fill: int = 0xA5, glv_in: bytes = None):
    """TEST HOOK: the proof assembly kernels on a caller's sums; see gsc_debug_assemble in include/libprove.h.  sets: "a", "b1", "k", "z", "b2" and
    optionally "c", "d", "pok" -> (points, infinity bytes, scales) as the header lays them out; rs: batch x 64 bytes (r, s little-endian);
    mask: batch x 32 bytes little-endian; glv_in: 2 x nproofs records of 44 bytes the latency kernel gets instead of glv_split's.  -> dict: rc, out, flags, tmp, tmp_inf, cpts, commit, W, mask_out, glv (bytes as stored; None where
    the part did not run)."""
    bufs = {"out": 256 * batch, "flags": batch, "tmp": 128 * batch, "tmp_inf": 2 * batch, "W": 128 * batch}
    if sets.get("d") is not None:
        bufs.update(cpts=128 * batch, commit=32 * batch)
    if mask is not None:
        bufs["mask_out"] = 32 * batch
    if nproofs:
        bufs["glv"] = 88 * nproofs
    bufs = {k: C.create_string_buffer(max(1, v)) for k, v in bufs.items()}
    args = DebugAssembleArgs(batch=batch, nproofs=nproofs, n_wires=n_wires, fill=fill, rs=rs, mask=mask, glv_in=glv_in)
    for name in _ASSEMBLE_SETS:
        if sets.get(name) is not None:
            for part, b in zip(("_pts", "_inf", "_lam"), sets[name]):
                setattr(args, name + part, b)
    for k, b in bufs.items():
        setattr(args, k, C.cast(b, C.c_void_p))
    rc = lib().gsc_debug_assemble(C.byref(args))
    res = {k: None for k in ("out", "flags", "tmp", "tmp_inf", "cpts", "commit", "W", "mask_out", "glv")}
    res.update({k: b.raw for k, b in bufs.items()})
    res["rc"] = rc
    return res


def debug_verify_g1(algorithm_id: int, vk: bytes, proofs: bytes, lens, signals: bytes, rnd, ends=(), path: int = 1, fill: int = 0xA5):
    """TEST HOOK: the verifier's G1 stage on a caller's key, proofs and randomizers; see gsc_debug_verify_g1 in include/libprove.h.  proofs: 196-byte
    slots; rnd: n x 8 words (rho, t); ends: the part ends of the claim-wise check, or none.  -> dict: rc and, when rc == 0, the outputs as bytes
    (prho: a list of 5-word tuples), each filled with `fill` before the call."""
    n, np = len(lens), len(ends)
    assert len(proofs) >= 196 * n and len(signals) >= 144 * n and len(rnd) == 8 * n
    sizes = {"key_status": 2048, "table": 144 * 256 * 65, "ctable": 32 * 256 * 65, "ok": n, "g1": 6 * 65 * n, "g2": 129 * n, "okv": n, "fixed": 5 * 65, "flag": 1,
             "pfixed": 5 * 65 * np, "prho": 20 * np, "pflag": np}
    bufs = {k: C.create_string_buffer(bytes([fill]) * max(1, v), max(1, v)) for k, v in sizes.items()}
    lens_arr, rnd_arr, ends_arr = (C.c_uint32 * max(n, 1))(*lens), (C.c_uint32 * max(8 * n, 1))(*rnd), (C.c_uint64 * max(np, 1))(*ends)
    args = DebugVerifyG1Args(algorithm=algorithm_id, path=path, fill=fill, vk=bytes(vk), vk_len=len(vk), n=n, proofs=bytes(proofs), lens=C.cast(lens_arr, C.c_void_p),
                             signals=bytes(signals), rnd=C.cast(rnd_arr, C.c_void_p), np=np, ends=C.cast(ends_arr, C.c_void_p) if np else None, key_status_cap=sizes["key_status"])
    for k, b in bufs.items():
        setattr(args, k, C.cast(b, C.c_void_p))
    res = {"rc": lib().gsc_debug_verify_g1(C.byref(args))}
    res.update({k: b.raw[:sizes[k]] for k, b in bufs.items()})
    res["prho"] = [tuple(int.from_bytes(res["prho"][20 * p + 4 * c:20 * p + 4 * c + 4], "little") for c in range(5)) for p in range(np)]
    return res


def prove_raw(cipher: int, records: bytes, n: int):
    """Binary batch path: n records of 112 B {key[32], nonce[12], counter u32 LE, input[64]}.
    Returns (n_ok, proofs[n][196], lens[n], ciphertexts[n][64])."""
    proofs = C.create_string_buffer(196 * n)
    lens = (C.c_uint32 * n)()
    cts = C.create_string_buffer(64 * n)
    ok = lib().gsc_prove_raw(cipher, records, n, proofs, lens, cts)
    return ok, proofs.raw, list(lens), cts.raw


def raw_buffers(n: int):
    """Reusable output buffers for prove_raw_into: (proofs[n][196], lens[n] u32, ciphertexts[n][64])."""
    return C.create_string_buffer(196 * n), (C.c_uint32 * n)(), C.create_string_buffer(64 * n)


def prove_raw_into(cipher: int, records: bytes, n: int, proofs, lens, cts) -> int:
    """prove_raw without per-call allocations and copies: fills caller-owned buffers (raw_buffers), returns the number of proofs produced."""
    return lib().gsc_prove_raw(cipher, records, n, proofs, lens, cts)


def set_deterministic_randomness(r=None, s=None, mask=0):
    """TEST HOOK: fix (r, s, mask) as integers; None restores the CSPRNG.  Needs GSC_ENABLE_TEST_HOOKS=1 in the environment
    before the library is loaded."""
    if r is None:
        rc = lib().gsc_set_deterministic_randomness(None, None, None)
    else:
        rc = lib().gsc_set_deterministic_randomness(int(r).to_bytes(32, "big"), int(s).to_bytes(32, "big"), int(mask).to_bytes(32, "big"))
    if rc != 0:
        raise RuntimeError("test hooks are disabled: set GSC_ENABLE_TEST_HOOKS=1 before loading libprove.so")


def debug_prove(params: dict):
    """TEST HOOK: run one proof and return the device pipeline's intermediate vectors as lists of ints.
    W/A/B/C come back in Montgomery form and are converted here with Python integers."""
    r_mod = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
    rinv = pow(1 << 256, -1, r_mod)
    s, keep = _slice(json.dumps(params).encode())
    if lib().gsc_debug_prove(s) != 0:
        raise RuntimeError("debug prove failed")
    out = {}
    for which, name, mont in ((0, "W", True), (1, "A", True), (2, "B", True), (3, "C", True), (4, "h", False)):
        n = lib().gsc_debug_vector(which, None, 0)
        buf = C.create_string_buffer(32 * n)
        lib().gsc_debug_vector(which, buf, 32 * n)
        vals = [int.from_bytes(buf.raw[32 * i:32 * i + 32], "little") for i in range(n)]
        if mont:
            vals = [v * rinv % r_mod for v in vals]
        out[name] = vals
    return out


def describe(algorithm_id: int) -> str:
    buf = C.create_string_buffer(4096)
    lib().gsc_describe(algorithm_id, buf, 4096)
    return buf.value.decode()


def last_stage_ms(algorithm_id: int):
    arr = (C.c_float * 4)()
    if lib().gsc_last_stage_ms(algorithm_id, arr) != 0:
        return None
    return dict(zip(("witness", "quotient", "msm", "assembly"), list(arr)))


def last_dominant_kernel(algorithm_id: int):
    """(kernel name, milliseconds, statements proved, padded columns, Z bases per proof) of the dominant kernel in the batch that
    finished last: the Z-table MSM for batch calls, the resident witness solver for calls on the latency path."""
    name = C.create_string_buffer(96)
    ms, st, cols, nb = C.c_float(0), C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    if lib().gsc_last_dominant_kernel(algorithm_id, name, 96, C.byref(ms), C.byref(st), C.byref(cols), C.byref(nb)) != 0:
        return None
    return name.value.decode(), float(ms.value), st.value, cols.value, nb.value


def debug_secret_residue(algorithm_id: int) -> int:
    """TEST HOOK: bytes of a finished call's secrets still non-zero in device memory (0 expected; -1: hooks disabled / error)."""
    lib().gsc_debug_secret_residue.restype = C.c_longlong
    lib().gsc_debug_secret_residue.argtypes = [C.c_ubyte]
    return int(lib().gsc_debug_secret_residue(algorithm_id))


def debug_secret_scan(algorithm_id: int):
    """TEST HOOK: (bytes off the idle image over every secret region of every lane, {"lane<i>.<name>": bytes} of the regions that are not clean,
    {"registered": bytes, "allocated": bytes, "public": [names]}); the total is -1 with the hooks disabled / on error."""
    buf = C.create_string_buffer(16384)
    lib().gsc_debug_secret_scan.restype = C.c_longlong
    lib().gsc_debug_secret_scan.argtypes = [C.c_ubyte, C.c_char_p, C.c_size_t]
    total = int(lib().gsc_debug_secret_scan(algorithm_id, buf, 16384))
    dirty, info = {}, {}
    for word in buf.value.decode().split():
        k, v = word.split("=", 1)
        if k.startswith("lane"):
            dirty[k] = int(v)
        else:
            info[k] = v.split(",") if k == "public" else int(v)
    return total, dirty, info


def debug_wipe(nbytes: int, fill: int, descs, cls: bytes = b"", windows=(), want_buffer: bool = True):
    """TEST HOOK: k_wipe on a device buffer of nbytes bytes filled with `fill`.  descs / windows: (offset, rows, pitch, width[, image]) tuples.
    Returns (the buffer afterwards as bytes or None, [bytes off the idle image per window] by k_scan_idle, device ms of the wipe); raises on error."""
    def pack(items):
        flat = []
        for it in items:
            it = tuple(it)
            flat += list(it) + [0] * (5 - len(it))
        return (C.c_uint64 * max(1, len(flat)))(*flat)
    descs, windows = list(descs), list(windows)
    out = (C.c_ubyte * nbytes)() if want_buffer else None
    counts = (C.c_uint64 * max(1, len(windows)))()
    ms = C.c_float(0)
    f = lib().gsc_debug_wipe
    f.restype = C.c_int
    f.argtypes = [C.c_uint64, C.c_int, C.c_void_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_float)]
    rc = f(nbytes, fill, pack(descs), len(descs), cls if cls else None, len(cls), out, pack(windows), len(windows), counts, C.byref(ms))
    if rc != 0:
        raise RuntimeError("gsc_debug_wipe failed")
    return (bytes(out) if want_buffer else None), [int(counts[i]) for i in range(len(windows))], float(ms.value)


def debug_clock_trace(n: int, interval_us: int):
    """TEST HOOK: [(seconds since the first sample, shader clock in MHz over the interval before it)] from a resident one-wave sampler; blocks
    for n x interval_us microseconds — run it in a thread beside the calls to be observed."""
    buf = (C.c_ulonglong * (2 * n))()
    lib().gsc_debug_clock_trace.restype = C.c_int
    lib().gsc_debug_clock_trace.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(C.c_ulonglong)]
    if lib().gsc_debug_clock_trace(n, interval_us, buf) != 0:
        raise RuntimeError("gsc_debug_clock_trace failed")
    v = list(buf)
    return [((v[2 * i] - v[0]) / 1e8, 100.0 * (v[2 * i + 1] - v[2 * i - 1]) / max(1, v[2 * i] - v[2 * i - 2])) for i in range(1, n)]


def last_kernel_clock(algorithm_id: int):
    """(shader clock in MHz during the last batch's Z-table kernel — 0.0 when not measured —, digit windows of the Z set)."""
    mhz, nwin = C.c_float(0), C.c_int(0)
    if lib().gsc_last_kernel_clock(algorithm_id, C.byref(mhz), C.byref(nwin)) != 0:
        return None
    return float(mhz.value), int(nwin.value)


def last_msm_z_kernel(algorithm_id: int):
    """(milliseconds, columns in the launch, bases per proof) of the dominant kernel in the last batch (older tools)."""
    k = last_dominant_kernel(algorithm_id)
    return (k[1], k[3], k[4]) if k else None


def served(algorithm_id: int):
    """[(calls, statements)] per engine replica (GSC_DEVICES), parsed from gsc_describe."""
    d = describe(algorithm_id)
    tail = d.split("served(calls/statements)=")[1].split()[0]
    return [tuple(int(x) for x in part.split("/")) for part in tail.split(",")]


def debug_field_ops(field: int, op: int, a, b, chain=1):
    """TEST HOOK: a, b lists of ints (canonical residues) -> list of ints computed by the device's radix-2^29 field code."""
    n = len(a)
    out = C.create_string_buffer(32 * n)
    rc = lib().gsc_debug_field_ops(field, op, b"".join(int(x).to_bytes(32, "little") for x in a), b"".join(int(x).to_bytes(32, "little") for x in b), out, n, chain)
    if rc:
        raise RuntimeError("gsc_debug_field_ops failed")
    return [int.from_bytes(out.raw[32 * i:32 * i + 32], "little") for i in range(n)]


def debug_limb_ops(field: int, op: int, a, b=None, c=None, d=None):
    """TEST HOOK: a (b, c, d): lists of 9-tuples of raw int32 limbs -> list of 9-tuples computed by the device's radix-2^29 code on
    exactly these limbs.  op: 0 mul, 1 sqr, 2 fmms, 3 norm, 4 freeze, 5 freeze_near."""
    n = len(a)
    arrs = [None if v is None else (C.c_int32 * (9 * n))(*[l for e in v for l in e]) for v in (a, b, c, d)]
    out = (C.c_int32 * (9 * n))()
    if lib().gsc_debug_limb_ops(field, op, arrs[0], arrs[1], arrs[2], arrs[3], out, n):
        raise RuntimeError("gsc_debug_limb_ops failed")
    return [tuple(out[9 * i:9 * i + 9]) for i in range(n)]


def debug_curve_ops(group: int, op: int, pts: bytes, inf: bytes, lam: bytes, n: int, k: int):
    """TEST HOOK: the device's XYZZ group law on packed canonical affine points (layout: include/libprove.h gsc_debug_curve_ops)
    -> (packed affine results, flag bytes)."""
    w = 64 if group == 0 else 128
    assert len(pts) == w * n * k and len(inf) == n * k and len(lam) == w * n
    out = C.create_string_buffer(w * n)
    flags = C.create_string_buffer(n)
    if lib().gsc_debug_curve_ops(group, op, pts, inf, lam, n, k, out, flags):
        raise RuntimeError("gsc_debug_curve_ops failed")
    return out.raw, flags.raw


def debug_decode_points(group: int, encoded: bytes, n: int):
    """TEST HOOK: the key-point decode of InitAlgorithm (host walk + kernels; G2 with the subgroup test) on n encoded elements, each
    compressed or raw -> (canonical big-endian X | Y bytes, 64 per G1 and 128 per G2 point, status bytes: 0 ok, 1 refused, 2 infinity).
    Raises RuntimeError when the library returns -1 (a slice that ends inside an element, bytes left over, hooks off)."""
    L = lib()
    L.gsc_debug_decode_points.restype = C.c_int
    L.gsc_debug_decode_points.argtypes = [C.c_int, C.c_char_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p]
    w = 64 if group == 0 else 128
    out, st = C.create_string_buffer(max(1, w * n)), C.create_string_buffer(max(1, n))
    if L.gsc_debug_decode_points(group, bytes(encoded), len(encoded), n, out, st):
        raise RuntimeError("gsc_debug_decode_points failed")
    return out.raw[:w * n], st.raw[:n]


def tower_words(path: int, op: int):
    """(int32 words one element of gsc_debug_tower_ops reads, words it writes); the table of include/libprove.h"""
    if not (0 <= op < 30 if path == 0 else path == 1 and 16 <= op <= 25):
        raise RuntimeError("gsc_debug_tower_ops: path %d has no op %d" % (path, op))
    win = {0: 9, 11: 9, 13: 9, 1: 20, 2: 36, 3: 36, 6: 36, 28: 36, 29: 36, 8: 27, 10: 19, 16: 216, 18: 162, 26: 54, 27: 90}.get(op, 108 if op >= 16 else 18)
    wout = {0: 9, 1: 9, 11: 9, 13: 9, 15: 0, 25: 0, 26: 108, 27: 108, 28: 72, 29: 5508}.get(op, (144 if path == 1 else 108) if op >= 16 else 18)
    return win, wout


def debug_tower_ops(path: int, op: int, rows):
    """TEST HOOK: rows: one flat tuple of raw int32 words per element (layout: include/libprove.h gsc_debug_tower_ops) -> (list of flat
    tuples of the words the device wrote, list of flags).  path 0: verify_dev.hpp per thread; path 1: verify_few_dev.hpp per 8-lane group."""
    win, wout = tower_words(path, op)
    n = len(rows)
    assert all(len(r) == win for r in rows)
    src = (C.c_int32 * max(1, win * n))(*[w for r in rows for w in r])
    out = (C.c_int32 * max(1, wout * n))()
    flags = C.create_string_buffer(max(1, n))
    if lib().gsc_debug_tower_ops(path, op, src, n, out, flags):
        raise RuntimeError("gsc_debug_tower_ops failed")
    flat = list(out)
    return [tuple(flat[wout * i:wout * (i + 1)]) for i in range(n)], list(flags.raw[:n])


def debug_glv_split(k: int):
    """TEST HOOK (host arithmetic, no GPU): k -> (k1, k2) with k = k1 + k2 * lambda (mod r), the split of csrc/glv.hpp."""
    L = lib()
    L.gsc_debug_glv_split.restype = C.c_int
    L.gsc_debug_glv_split.argtypes = [C.c_char_p, C.c_void_p]
    out = C.create_string_buffer(44)
    if L.gsc_debug_glv_split(int(k).to_bytes(32, "little"), out) != 0:
        raise RuntimeError("gsc_debug_glv_split failed")
    k1 = int.from_bytes(out.raw[:20], "little"); k2 = int.from_bytes(out.raw[20:40], "little"); neg = out.raw[40]
    return (-k1 if neg & 1 else k1), (-k2 if neg & 2 else k2)


def debug_compute_h(algorithm_id: int, abc_be: bytes, m: int) -> bytes:
    """TEST HOOK: computeH on 64 columns of caller-supplied a|b|c ([m][64] big-endian each) -> [domain][64] little-endian rows in
    bit-reversed order (raw bytes)."""
    L = lib()
    L.gsc_debug_compute_h.restype = C.c_longlong
    L.gsc_debug_compute_h.argtypes = [C.c_ubyte, C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t]
    n = L.gsc_debug_compute_h(algorithm_id, None, 0, None, 0)
    if n <= 0:
        raise RuntimeError("algorithm not initialised")
    assert len(abc_be) == 3 * m * 64 * 32
    out = C.create_string_buffer(n * 64 * 32)
    if L.gsc_debug_compute_h(algorithm_id, abc_be, m, out, len(out)) != n:
        raise RuntimeError("gsc_debug_compute_h failed")
    return out.raw


def debug_compute_d(algorithm_id: int, ab_be: bytes, m: int) -> bytes:
    """TEST HOOK: the evaluation-form quotient kernels on 64 columns of caller-supplied a|b ([m][64] big-endian each) ->
    [domain][64] little-endian rows, row i = A(zeta w^i) B(zeta w^i) 2^261 mod r (raw bytes)."""
    L = lib()
    L.gsc_debug_compute_d.restype = C.c_longlong
    L.gsc_debug_compute_d.argtypes = [C.c_ubyte, C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t]
    n = L.gsc_debug_compute_d(algorithm_id, None, 0, None, 0)
    if n <= 0:
        raise RuntimeError("algorithm not initialised")
    assert len(ab_be) == 2 * m * 64 * 32
    out = C.create_string_buffer(n * 64 * 32)
    if L.gsc_debug_compute_d(algorithm_id, ab_be, m, out, len(out)) != n:
        raise RuntimeError("gsc_debug_compute_d failed")
    return out.raw


def debug_quotient(algorithm_id: int, ab_be, m: int, planes=None, plain: int = 0, ncols: int = 0, live: int = 0, c: int = 0) -> bytes:
    """TEST HOOK: the evaluation-form quotient kernels on the routes of a batch call; see gsc_debug_quotient in include/libprove.h.  ab_be: a | b,
    [m][64] big-endian each, m up to the domain size n; planes: None or the int8 planes of a | b, [n][64] each (bytes, or anything with the buffer
    protocol).  Returns the raw output: [n][64] little-endian d for c = 0, the digit buffer for c > 0."""
    L = lib()
    n = L.gsc_debug_quotient(C.byref(DebugQuotientArgs(algorithm=algorithm_id)))
    if n <= 0:
        raise RuntimeError("algorithm not initialised")
    ab_be = memoryview(ab_be).cast("B")
    assert len(ab_be) == 2 * m * 64 * 32
    def held(view):      # a ctypes array over the caller's bytes (copied only when they are read-only); m = 0 has none: one spare byte to point at
        return C.create_string_buffer(1) if not len(view) else (C.c_char * len(view)).from_buffer_copy(view) if view.readonly else (C.c_char * len(view)).from_buffer(view)
    keep = [held(ab_be)]
    if planes is not None:
        planes = memoryview(planes).cast("B")
        assert len(planes) == 2 * n * 64
        keep.append(held(planes))
    nwin = 0
    if c:
        nwin = (254 + c - 1) // c
        if (0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001 >> (c * (nwin - 1))) + 1 > (1 << (c - 1)) - 1:      # msm_windows (csrc/kernels.hpp): the top window absorbs the last carry
            nwin += 1
    out = C.create_string_buffer(nwin * (n // 8) * 64 * (32 if c > 16 else 16) if c else n * 64 * 32)
    args = DebugQuotientArgs(algorithm=algorithm_id, plain=plain, c=c, mats_be=C.addressof(keep[0]), m=m,
                             planes=C.addressof(keep[1]) if planes is not None else None, ncols=ncols, live=live, out=C.addressof(out), cap=len(out))
    if L.gsc_debug_quotient(C.byref(args)) != n:
        raise RuntimeError("gsc_debug_quotient failed (see stdout)")
    return out.raw


def debug_z_sum(algorithm_id: int, abc_be: bytes, m: int):
    """TEST HOOK: the evaluation-form quotient sum of 64 columns of caller-supplied a|b|c ([m][64] big-endian each, c = a b) through the
    batch kernels and the engine's own Z sets -> (64 x 64 B big-endian X | Y, 64 infinity flags)."""
    L = lib()
    L.gsc_debug_z_sum.restype = C.c_int
    L.gsc_debug_z_sum.argtypes = [C.c_ubyte, C.c_char_p, C.c_size_t, C.c_void_p, C.c_void_p]
    assert len(abc_be) == 3 * m * 64 * 32
    out, flags = C.create_string_buffer(64 * 64), C.create_string_buffer(64)
    if L.gsc_debug_z_sum(algorithm_id, abc_be, m, out, flags) != 0:
        raise RuntimeError("gsc_debug_z_sum failed")
    return out.raw, flags.raw


def debug_quot_fold_dft(L: int, m: int, perm, u_be: bytes, u_inf: bytes, v_be: bytes, v_inf: bytes):
    """TEST HOOK: the fold of the redundant quotient bases by three group transforms on caller-supplied bases (no InitAlgorithm).  n = 2^L;
    perm: n table positions -> coset indices, or None for the identity; u_be (m) and v_be (n, table order): 64 B big-endian X | Y per point with
    infinity flags -> (U' bytes, U' flags, V' bytes, V' flags) for m and m - 1 points.  Raises RuntimeError when the library returns -1."""
    lb = lib()
    n = 1 << L
    lb.gsc_debug_quot_fold_dft.restype = C.c_int
    lb.gsc_debug_quot_fold_dft.argtypes = [C.c_int, C.c_uint32, C.c_void_p] + [C.c_char_p] * 4 + [C.c_void_p] * 4
    assert len(u_be) == 64 * m and len(u_inf) == m and len(v_be) == 64 * n and len(v_inf) == n and (perm is None or len(perm) == n)
    pm = (C.c_uint32 * n)(*perm) if perm is not None else None
    u2, f2, v2, g2 = C.create_string_buffer(64 * m), C.create_string_buffer(m), C.create_string_buffer(64 * max(m - 1, 1)), C.create_string_buffer(max(m - 1, 1))
    if lb.gsc_debug_quot_fold_dft(L, m, pm, u_be, u_inf, v_be, v_inf, u2, f2, v2, g2) != 0:
        raise RuntimeError("gsc_debug_quot_fold_dft failed")
    return u2.raw, f2.raw, v2.raw[:64 * (m - 1)], g2.raw[:m - 1]


# ---- GPU verifier in libprove.so (k_verify.hip): verdicts identical to libverify's Verify ----
def verify_init(algorithm_id: int, verifying_key: bytes) -> bool:
    """gsc_verify_init: load a verifying key (InitVerifier's bytes) for the GPU verifier."""
    s, keep = _slice(verifying_key)
    return bool(lib().gsc_verify_init(algorithm_id, s))


def verify_raw(algorithm_id: int, proofs: bytes, lens, signals: bytes, n: int = None):
    """gsc_verify_raw: n proofs in 196-byte slots (prove_raw's layout), their lengths, n x 144 signal bytes -> list of 0/1 verdicts.
    Raises RuntimeError when no key is loaded (-1) or on a device error (-2)."""
    n = len(lens) if n is None else n
    assert len(proofs) >= 196 * n and len(signals) >= 144 * n
    lens_arr = (C.c_uint32 * max(n, 1))(*lens[:n])
    out = C.create_string_buffer(max(n, 1))
    rc = lib().gsc_verify_raw(algorithm_id, bytes(proofs), lens_arr, bytes(signals), n, out)
    if rc < 0:
        raise RuntimeError("gsc_verify_raw failed (%d): %s" % (rc, "no key loaded" if rc == -1 else "device error"))
    return list(out.raw[:n])


def verify_batch(items) -> list:
    """VerifyBatch: list of Verify inputs (dicts; bytes values become arrays) -> list of bools."""
    enc = [{k: (list(v) if isinstance(v, (bytes, bytearray)) else v) for k, v in it.items()} if isinstance(it, dict) else it for it in items]
    s, keep = _slice(json.dumps(enc).encode())
    return json.loads(_take(lib().VerifyBatch(s)))


def verify_batch_bytes(params_json: bytes) -> bytes:
    """VerifyBatch on already encoded JSON; returns the raw JSON bytes."""
    s, keep = _slice(params_json)
    return _take(lib().VerifyBatch(s))


def verify_raw_batched(algorithm_id: int, proofs: bytes, lens, signals: bytes, n: int = None):
    """gsc_verify_raw_batched: verify_raw's arguments and verdicts, one final exponentiation per chunk when every proof holds.
    Raises RuntimeError when no key is loaded (-1) or on a device error (-2)."""
    n = len(lens) if n is None else n
    assert len(proofs) >= 196 * n and len(signals) >= 144 * n
    lens_arr = (C.c_uint32 * max(n, 1))(*lens[:n])
    out = C.create_string_buffer(max(n, 1))
    rc = lib().gsc_verify_raw_batched(algorithm_id, bytes(proofs), lens_arr, bytes(signals), n, out)
    if rc < 0:
        raise RuntimeError("gsc_verify_raw_batched failed (%d): %s" % (rc, "no key loaded" if rc == -1 else "device error"))
    return list(out.raw[:n])


def verify_all(algorithm_id: int, proofs: bytes, lens, signals: bytes, n: int = None) -> int:
    """gsc_verify_all: 1 iff every item verifies, 0 otherwise, -1 no key loaded, -2 device error."""
    n = len(lens) if n is None else n
    assert len(proofs) >= 196 * n and len(signals) >= 144 * n
    lens_arr = (C.c_uint32 * max(n, 1))(*lens[:n])
    return lib().gsc_verify_all(algorithm_id, bytes(proofs), lens_arr, bytes(signals), n)


def verify_all_json(items) -> bool:
    """VerifyAll: a list of Verify inputs (dicts; bytes values become arrays), or already encoded JSON bytes / str -> bool."""
    if isinstance(items, str):
        items = items.encode()
    if not isinstance(items, (bytes, bytearray)):
        items = json.dumps([{k: (list(v) if isinstance(v, (bytes, bytearray)) else v) for k, v in it.items()} if isinstance(it, dict) else it
                            for it in items]).encode()
    s, keep = _slice(bytes(items))
    return bool(lib().VerifyAll(s))


def verify_claims(algorithm_id: int, proofs: bytes, lens, signals: bytes, ends):
    """gsc_verify_claims: verify_raw's items cut into claims, claim j = items [ends[j-1], ends[j]) -> list of 0/1 verdicts, one per claim,
    each from a batched check of its own.  Raises RuntimeError when no key is loaded (-1), on a device error (-2) or when ends is not
    non-decreasing up to the number of items (-3)."""
    n, m = len(lens), len(ends)
    assert len(proofs) >= 196 * n and len(signals) >= 144 * n
    lens_arr = (C.c_uint32 * max(n, 1))(*lens)
    ends_arr = (C.c_uint64 * max(m, 1))(*ends)
    out = C.create_string_buffer(max(m, 1))
    rc = lib().gsc_verify_claims(algorithm_id, bytes(proofs), lens_arr, bytes(signals), n, ends_arr, m, out)
    if rc < 0:
        raise RuntimeError("gsc_verify_claims failed (%d): %s" % (rc, {-1: "no key loaded", -2: "device error"}.get(rc, "bad claim ends")))
    return list(out.raw[:m])


def verify_claims_json(claims):
    """VerifyClaims: a list of claims, each a list of Verify inputs (dicts; bytes values become arrays), or already encoded JSON
    bytes / str -> the decoded result: a list of bools, one per claim (top-level errors: VerifyBatch's shapes)."""
    if isinstance(claims, str):
        claims = claims.encode()
    if not isinstance(claims, (bytes, bytearray)):
        enc = lambda it: {k: (list(v) if isinstance(v, (bytes, bytearray)) else v) for k, v in it.items()} if isinstance(it, dict) else it
        claims = json.dumps([[enc(it) for it in cl] if isinstance(cl, list) else cl for cl in claims]).encode()
    s, keep = _slice(bytes(claims))
    return json.loads(_take(lib().VerifyClaims(s)))


def debug_verify_randomizers(seed: bytes = None, all_ones: bool = False) -> int:
    """TEST HOOK: randomizers of the batched check from a 32-byte seed, or all 1 (the naive sum); no arguments: the OS CSPRNG.
    Returns 0, -1 when test hooks are disabled."""
    assert seed is None or len(seed) == 32
    return lib().gsc_debug_verify_randomizers(None if seed is None else bytes(seed), 1 if all_ones else 0)


def verify_json(params) -> bool:
    """gsc_verify_json: Verify's input (bytes/str JSON, or a dict whose bytes values become arrays) answered on the GPU."""
    if isinstance(params, dict):
        params = json.dumps({k: (list(v) if isinstance(v, (bytes, bytearray)) else v) for k, v in params.items()})
    s, keep = _slice(params.encode() if isinstance(params, str) else bytes(params))
    return bool(lib().gsc_verify_json(s))


def verify_last_path(algorithm_id: int) -> int:
    """gsc_verify_last_path: 1 the last verifier call on this key ran one thread per proof, 2 the few-proof groups, 0 none yet, -1 no key."""
    return lib().gsc_verify_last_path(algorithm_id)


def debug_verify_path(mode: int) -> int:
    """TEST HOOK: route every later verifier call: 0 automatic, 1 one thread per proof, 2 the few-proof groups.  -1 when hooks are off."""
    return lib().gsc_debug_verify_path(mode)


def debug_pairing(g1_points, g2_points, few: bool = False):
    """TEST HOOK: reduced pairings on the device (few: by the few-proof kernels).  g1_points: [(x, y)] ints (None = infinity),
    g2_points: [((x0, x1), (y0, y1))] -> list of 12-tuples of ints, element 2i + j = component j (of 1, u) of the w^i coefficient."""
    n = len(g1_points)
    b1 = b"".join(bytes(64) if P is None else P[0].to_bytes(32, "big") + P[1].to_bytes(32, "big") for P in g1_points)
    b2 = b"".join(bytes(128) if Q is None else Q[0][1].to_bytes(32, "big") + Q[0][0].to_bytes(32, "big") + Q[1][1].to_bytes(32, "big") + Q[1][0].to_bytes(32, "big") for Q in g2_points)
    out = C.create_string_buffer(384 * max(n, 1))
    if (lib().gsc_debug_pairing_few if few else lib().gsc_debug_pairing)(b1, b2, n, out) != n:
        raise RuntimeError("gsc_debug_pairing failed (test hooks off?)")
    return [tuple(int.from_bytes(out.raw[384 * i + 32 * c:384 * i + 32 * c + 32], "big") for c in range(12)) for i in range(n)]


# ---- the prover's self-check ----
def prove_check_init(algorithm_id: int, verifying_key: bytes = b"") -> int:
    """gsc_prove_check_init: from now on every chunk of the algorithm is verified on the device under this key (gnark VerifyingKey.WriteTo
    bytes) before its proofs are released.  1 on; 0 key refused (the state stays as it was); -1 algorithm not initialised.  Empty bytes: off (1)."""
    if not verifying_key:
        return lib().gsc_prove_check_init(algorithm_id, GoSlice(None, 0, 0))
    s, keep = _slice(verifying_key)
    return lib().gsc_prove_check_init(algorithm_id, s)


def prove_check_stats(algorithm_id: int):
    """gsc_prove_check_stats: (chunks checked, proofs checked, proofs refused by the check, chunks that needed the proof-by-proof pass); all 0
    while the check is off; None when the algorithm is not initialised."""
    out = (C.c_uint64 * 4)()
    if lib().gsc_prove_check_stats(algorithm_id, out) != 0:
        return None
    return tuple(int(v) for v in out)


PROOF_POINTS = {"A": 0, "B": 1, "C": 2, "D": 3, "PoK": 4}


def debug_prove_corrupt(algorithm_id: int, index: int, which, mode: int = 0) -> int:
    """TEST HOOK: arms a one-shot change to statement `index` of the algorithm's next chunk, on the device in front of the self-check and the
    download.  which: "A", "B", "C", "D", "PoK" (or 0..4); mode 0: the same point of statement (index + 1) mod n, mode 1: bit 0 of its y
    flipped.  Returns 0, -1 when hooks are off / the algorithm is not initialised / the proofs have no such point."""
    return lib().gsc_debug_prove_corrupt(algorithm_id, index, PROOF_POINTS.get(which, which), mode)


# ---- libverify (CPU-side, libraries/verifier/libverify.go:14-17) ----
_vlib = None


def verify_lib():
    global _vlib
    if _vlib is None:
        if not os.path.exists(VERIFY_LIB_PATH):
            raise RuntimeError("libverify.so is not built: make -C %s" % CSRC)
        L = C.CDLL(VERIFY_LIB_PATH)
        L.Verify.restype = C.c_ubyte
        L.Verify.argtypes = [GoSlice]
        L.InitVerifier.restype = C.c_ubyte
        L.InitVerifier.argtypes = [C.c_ubyte, GoSlice]
        _vlib = L
    return _vlib


def init_verifier(algorithm_id: int, verifying_key: bytes) -> bool:
    s, keep = _slice(verifying_key)
    return bool(verify_lib().InitVerifier(algorithm_id, s))


def verify(params) -> bool:
    """Verify(params) — libverify.go:14-17.  params: bytes/str JSON or a dict with cipher / proof / publicSignals."""
    if isinstance(params, dict):
        params = json.dumps({k: (list(v) if isinstance(v, (bytes, bytearray)) else v) for k, v in params.items()})
    if isinstance(params, str):
        params = params.encode()
    s, keep = _slice(params)
    return bool(verify_lib().Verify(s))
