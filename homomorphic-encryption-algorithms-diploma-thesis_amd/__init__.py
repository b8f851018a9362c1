"""hecdna — MI355X-native CKKS homomorphic linear-algebra engine (Python plumbing).

The product is the C-ABI in ``include/hecdna.h`` implemented by ``libhecdna.so`` (HIP kernels for
gfx950, built in-tree by ``make`` in this directory).  This module is a thin ctypes binding of that
C-ABI used by the tests, ``bench.py`` and ``__graft_entry__.py``; it mirrors the reference's
operator surface (``he::operators`` / ``he::linalg``, see cpp/ for the C++ façade) but adds no
computation of its own.  Loading fails loudly when the shared library is missing: there is no CPU
fallback.

Data layout (SEAL layout): ciphertext u64[size][level][N] (NTT form), key u64[L][2][K][N].
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HECDNA_LIB") or os.path.join(_HERE, "libhecdna.so")  # override: experiments
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "hecdna.h")

_lib = None
u64p = C.POINTER(C.c_uint64)


HEC_OK, HEC_EINVAL, HEC_ELOGIC, HEC_EDEVICE = 0, 1, 2, 3  # include/hecdna.h status codes


class HecError(Exception):
    """Mirrors SEAL's exception classes: code 1 = invalid_argument, 2 = logic_error, 3 = device."""

    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


class InvalidArgument(HecError, ValueError):
    pass


class LogicError(HecError, RuntimeError):
    pass


def build(jobs: int = 8):
    subprocess.check_call(["make", "-s", "-C", _HERE, f"-j{jobs}"])


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: build the HIP engine first (make -C {_HERE})")
        L = C.CDLL(LIB_PATH)
        L.hec_last_error.restype = C.c_char_p
        vp = C.c_void_p
        sig = {
            "hec_context_create": [C.c_uint64, u64p, C.c_uint64, C.c_int, C.POINTER(vp)],
            "hec_context_destroy": [vp],
            "hec_context_set_stream": [vp, vp],
            "hec_context_synchronize": [vp],
            "hec_context_set_option": [vp, C.c_char_p, C.c_int64],
            "hec_ciphertext_create": [vp, C.POINTER(vp)],
            "hec_ciphertext_destroy": [vp],
            "hec_ciphertext_upload": [vp, u64p, C.c_uint64, C.c_uint64, C.c_double],
            "hec_ciphertext_download": [vp, u64p],
            "hec_ciphertext_info": [vp, u64p, u64p, C.POINTER(C.c_double)],
            "hec_ciphertext_copy": [vp, vp],
            "hec_ciphertext_export_device": [vp, vp],
            "hec_ciphertext_import_device": [vp, vp, C.c_uint64, C.c_uint64, C.c_double],
            "hec_ciphertext_reduce": [vp, vp],
            "hec_ciphertext_fill_uniform": [vp, C.c_uint64, C.c_uint64, C.c_double, C.c_uint64],
            "hec_plaintext_create": [vp, C.POINTER(vp)],
            "hec_plaintext_destroy": [vp],
            "hec_plaintext_upload": [vp, u64p, C.c_uint64, C.c_double],
            "hec_kswitch_key_upload": [vp, u64p, C.POINTER(vp)],
            "hec_kswitch_key_fill_uniform": [vp, C.c_uint64, C.POINTER(vp)],
            "hec_kswitch_key_destroy": [vp],
            "hec_kswitch_key_download": [vp, u64p],
            "hec_galois_keys_download": [vp, C.c_uint32, u64p],
            "hec_galois_keys_create": [vp, C.POINTER(vp)],
            "hec_galois_keys_add": [vp, C.c_uint32, u64p],
            "hec_galois_keys_add_uniform": [vp, C.c_uint32, C.c_uint64],
            "hec_galois_keys_destroy": [vp],
            "hec_negate_inplace": [vp, vp],
            "hec_add_inplace": [vp, vp, vp],
            "hec_sub_inplace": [vp, vp, vp],
            "hec_add_plain_inplace": [vp, vp, vp],
            "hec_sub_plain_inplace": [vp, vp, vp],
            "hec_multiply_inplace": [vp, vp, vp],
            "hec_multiply_plain_inplace": [vp, vp, vp],
            "hec_square_inplace": [vp, vp],
            "hec_relinearize_inplace": [vp, vp, vp],
            "hec_rescale_to_next_inplace": [vp, vp],
            "hec_mod_switch_to_next_inplace": [vp, vp],
            "hec_rotate_vector_inplace": [vp, vp, C.c_int, vp],
            "hec_apply_galois_inplace": [vp, vp, C.c_uint32, vp],
            "hec_matmul_diag_col": [vp, vp, C.c_uint64, vp, C.c_uint64, vp, vp, vp],
            "hec_matmul_diagpt_col": [vp, vp, C.c_uint64, vp, C.c_uint64, vp, vp],
            "hec_bsgs_plan": [C.c_uint64, C.c_uint64, C.POINTER(C.c_int), C.c_uint64, u64p, u64p],
            "hec_matmul_diagpt_col_bsgs": [vp, vp, C.c_uint64, C.c_uint64, vp, C.c_uint64, vp, vp],
            "hec_matmul_diag_col_bsgs": [vp, vp, C.c_uint64, C.c_uint64, vp, C.c_uint64, vp, vp, vp],
            "hec_plaintext_fill_uniform": [vp, C.c_uint64, C.c_double, C.c_uint64],
            "hec_plaintext_download": [vp, u64p],
            "hec_plaintext_info": [vp, u64p, C.POINTER(C.c_double)],
            "hec_encode": [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_uint64, C.c_uint64, C.c_double,
                           C.c_uint64, vp],
            "hec_encode_scalar": [vp, C.c_double, C.c_double, C.c_uint64, vp],
            "hec_matmul_diag_col_partial": [vp, vp, C.c_uint64, C.c_uint64, C.c_uint64, vp, C.c_uint64, vp, vp],
            "hec_matmul_diag_col_partial_set": [vp, vp, C.c_uint64, vp, C.c_uint64, vp, C.c_uint64, vp, vp],
            "hec_matmul_finish": [vp, vp, C.c_uint64, vp, vp],
            "hec_matmul_col_colT": [vp, vp, C.c_uint64, vp, C.c_uint64, vp, vp, vp],
            "hec_colcolT_bsgs_plan": [C.c_uint64, C.c_uint64, C.c_int, C.POINTER(C.c_int), C.c_uint64, u64p, u64p],
            "hec_matmul_col_colT_bsgs": [vp, vp, C.c_uint64, vp, C.c_uint64, C.c_uint64, C.c_int, vp, vp, vp],
            "hec_matrix_matmul": [vp, vp, C.c_uint64, C.c_uint64, C.c_int, vp, C.c_uint64, C.c_uint64, C.c_int,
                                  vp, vp],
            "hec_ntt_forward": [vp, vp, C.c_uint64, C.c_uint64, C.c_uint64],
            "hec_ntt_inverse": [vp, vp, C.c_uint64, C.c_uint64, C.c_uint64],
            "hec_dyadic_multiply": [vp, vp, vp, vp, C.c_uint64, C.c_uint64, C.c_uint64],
            "hec_device_alloc": [vp, C.c_uint64, C.POINTER(vp)],
            "hec_device_free": [vp, vp],
            "hec_memcpy_h2d": [vp, vp, vp, C.c_uint64],
            "hec_memcpy_d2h": [vp, vp, vp, C.c_uint64],
            "hec_time_ntt_forward": [vp, vp, C.c_uint64, C.c_uint64, C.c_int, C.POINTER(C.c_double)],
            "hec_profile_enable": [vp, C.c_int],
            "hec_profile_read": [vp, C.c_char_p, C.POINTER(C.c_double), u64p],
            "hec_profile_read_ex": [vp, C.c_char_p, C.POINTER(C.c_double), u64p, C.POINTER(C.c_double), u64p],
            "hec_profile_classes": [vp, C.c_char_p, C.c_uint64],
            "hec_plan_diagonal_shards": [C.c_uint64, C.c_uint64, C.c_int, C.POINTER(C.c_uint32), C.c_uint64,
                                         C.POINTER(C.c_int32)],
            "hec_comm_unique_id": [vp],
            "hec_comm_init": [vp, C.c_int, C.c_int, vp],
            "hec_comm_init_ops": [vp, C.c_int, C.c_int, vp],
            "hec_shard_agree": [vp, C.c_int, C.c_int, C.c_char_p, C.POINTER(C.c_double), C.c_uint64, C.c_char_p,
                                C.c_uint64],
            "hec_context_comm": [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)],
            "hec_matmul_diag_col_sharded": [vp, vp, C.c_uint64, vp, C.c_uint64, vp, vp, vp],
            "hec_create_coeff_modulus": [C.c_uint64, C.POINTER(C.c_int), C.c_uint64, u64p],
            "hec_seal_blake2b": [vp, C.c_uint64, C.c_uint64, vp],
            "hec_seal_parms_id": [C.c_uint64, u64p, C.c_uint64, u64p],
            "hec_seal_ciphertext_load": [vp, C.c_uint64, u64p, u64p, u64p, C.POINTER(C.c_double), u64p, u64p,
                                         C.c_uint64, u64p],
            "hec_seal_ciphertext_load_ex": [vp, C.c_uint64, u64p, C.c_uint64, u64p, u64p, u64p,
                                            C.POINTER(C.c_double), u64p, u64p, C.c_uint64, u64p],
            "hec_seal_blake2xb": [vp, C.c_uint64, vp, C.c_uint64, C.c_uint64, vp],
            "hec_seal_shake256": [vp, C.c_uint64, C.c_uint64, vp],
            "hec_seal_ciphertext_save": [u64p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_double, u64p, C.c_int, vp,
                                         C.c_uint64, u64p],
            "hec_seal_parms_load": [vp, C.c_uint64, u64p, u64p, C.c_uint64, u64p, u64p],
            "hec_seal_parms_save": [C.c_uint64, u64p, C.c_uint64, C.c_int, vp, C.c_uint64, u64p],
            "hec_seal_kswitch_keys_load": [vp, C.c_uint64, C.c_uint64, u64p, u64p, C.c_uint64, u64p, u64p],
            "hec_seal_kswitch_keys_save": [C.c_uint64, u64p, C.c_uint64, C.POINTER(u64p), u64p, C.c_uint64, C.c_int,
                                           vp, C.c_uint64, u64p],
            "hec_seal_kswitch_keys_foreach": [vp, C.c_uint64, KEYLIST_VISIT, vp, u64p, u64p],
            "hec_seal_kswitch_keys_load_ex": [vp, C.c_uint64, C.c_uint64, C.c_uint64, u64p, u64p, C.c_uint64, u64p,
                                              u64p],
            "hec_seal_kswitch_keys_foreach_ex": [vp, C.c_uint64, C.c_uint64, KEYLIST_VISIT, vp, u64p, u64p],
            "hec_ciphertext_load_seal": [vp, vp, C.c_uint64, u64p],
            "hec_ciphertext_save_seal": [vp, C.c_int, vp, C.c_uint64, u64p],
            "hec_kswitch_key_load_seal": [vp, vp, C.c_uint64, C.POINTER(vp), u64p],
            "hec_galois_keys_load_seal": [vp, vp, C.c_uint64, u64p],
            "hec_galois_keys_load_seal_ex": [vp, vp, C.c_uint64, C.c_uint64, u64p],
            "hec_fft_twiddles": [C.c_uint64, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)],
            "hec_bfft_diagonal": [C.c_int, C.c_uint64, C.c_uint64, C.c_int, C.POINTER(C.c_double),
                                  C.POINTER(C.c_double)],
            "hec_fft": [vp, vp, C.c_uint64, C.c_int, vp],
            "hec_secret_key_upload": [vp, u64p, C.POINTER(vp)],
            "hec_secret_key_download": [vp, u64p],
            "hec_secret_key_destroy": [vp],
            "hec_decrypt": [vp, vp, vp, C.c_uint64, vp],
            "hec_decode": [vp, vp, C.c_uint64, C.c_uint64, C.POINTER(C.c_double), C.POINTER(C.c_double)],
            "hec_decrypt_decode": [vp, vp, vp, C.c_uint64, C.c_uint64, C.POINTER(C.c_double),
                                   C.POINTER(C.c_double)],
            "hec_bfft": [vp, vp, C.c_uint64, C.c_uint64, C.c_int, vp, vp],
            "hec_math_plan": [u64p, C.c_uint64, C.c_int, C.c_double, C.c_uint64, C.c_uint64, C.c_double, u64p,
                              C.POINTER(C.c_double)],
            "hec_math_signed_inv": [vp, vp, C.c_uint64, C.c_double, C.c_uint64, vp, vp],
            "hec_math_inv_sqrt_twice": [vp, vp, C.c_uint64, C.c_double, C.c_uint64, vp, vp],
            "hec_math_sqrt": [vp, vp, C.c_uint64, C.c_double, C.c_uint64, vp, vp],
            "hec_math_abs": [vp, vp, C.c_uint64, C.c_double, C.c_uint64, vp, vp],
            "hec_math_poly_plan": [u64p, C.c_uint64, C.POINTER(C.c_double), C.c_uint64, C.c_uint64, C.c_uint64,
                                   C.c_double, u64p, C.POINTER(C.c_double), u64p, u64p, u64p],
            "hec_math_poly": [vp, vp, C.c_uint64, C.POINTER(C.c_double), C.c_uint64, C.c_uint64, vp, vp],
            "hec_drop_chain_levels": [vp, vp, C.c_uint64, C.c_uint64],
            "hec_multiply_relin_rescale_many": [vp, vp, vp, C.c_uint64, vp, vp],
            "hec_sum_elems_many": [vp, vp, C.c_uint64, C.c_uint64, vp, vp],
            "hec_sum_elems_plan": [C.c_uint64, C.POINTER(C.c_int), C.c_uint64, u64p],
            "hec_keygen_secret": [vp, u64p, C.POINTER(vp)],
            "hec_keygen_public": [vp, vp, u64p, C.POINTER(vp)],
            "hec_public_key_upload": [vp, u64p, C.POINTER(vp)],
            "hec_public_key_download": [vp, u64p],
            "hec_public_key_destroy": [vp],
            "hec_keygen_relin": [vp, vp, u64p, C.POINTER(vp)],
            "hec_keygen_galois": [vp, vp, C.POINTER(C.c_uint32), C.c_uint64, u64p],
            "hec_encrypt_symmetric": [vp, vp, vp, C.c_uint64, u64p, vp, u64p],
            "hec_encrypt": [vp, vp, vp, C.c_uint64, u64p, vp],
            "hec_seal_ciphertext_save_seeded": [u64p, C.c_uint64, C.c_uint64, C.c_double, u64p, u64p, C.c_int, vp,
                                                C.c_uint64, u64p],
        }
        for name, args in sig.items():
            fn = getattr(L, name)
            fn.argtypes = args
            fn.restype = C.c_int
        L.hec_galois_elt_from_step.argtypes = [vp, C.c_int]
        L.hec_galois_elt_from_step.restype = C.c_uint32
        L.hec_default_galois_elts.argtypes = [vp, C.POINTER(C.c_uint32)]
        L.hec_default_galois_elts.restype = C.c_uint64
        L.hec_galois_keys_has.argtypes = [vp, C.c_uint32]
        L.hec_galois_keys_has.restype = C.c_int
        L.hec_profile_classes.restype = C.c_uint64
        L.hec_seal_last_error.restype = C.c_char_p
        L.hec_seal_kswitch_keys_default_limit.restype = C.c_uint64
        L.hec_galois_keys_load_seal_default_lists.argtypes = [vp]
        L.hec_galois_keys_load_seal_default_lists.restype = C.c_uint64
        _lib = L
    return _lib


def _check(rc):
    if rc != 0:
        msg = lib().hec_last_error().decode()
        if rc == 1:
            raise InvalidArgument(rc, msg)
        if rc == 2:
            raise LogicError(rc, msg)
        raise HecError(rc, msg)


def _p(a: np.ndarray):
    assert a.dtype == np.uint64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(u64p)


def exported_symbols():
    """Names declared in include/hecdna.h (for the C-ABI export test)."""
    import re
    txt = open(HEADER_PATH).read()
    return sorted(set(re.findall(r"\b(hec_[A-Za-z0-9_]+)\s*\(", txt)))


def plan_diagonal_shards(N, n, world, key_elts):
    """hec_plan_diagonal_shards (host only): per rank the sorted diagonals it owns."""
    keys = (C.c_uint32 * max(1, len(key_elts)))(*key_elts)
    out = (C.c_int32 * n)()
    _check(lib().hec_plan_diagonal_shards(N, n, world, keys, len(key_elts), out))
    plan = [[] for _ in range(world)]
    for j in range(n):
        plan[out[j]].append(j)
    return plan


def comm_unique_id() -> bytes:
    buf = C.create_string_buffer(128)
    _check(lib().hec_comm_unique_id(buf))
    return buf.raw


COMM_F64_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_uint64, C.c_int)
COMM_U64_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, u64p, C.c_uint64)
REDUCE_MIN, REDUCE_MAX = 0, 1


class CommOps(C.Structure):
    """include/hecdna.h hec_comm_ops"""
    _fields_ = [("user", C.c_void_p), ("allreduce_f64", COMM_F64_FN), ("allreduce_u64_sum", COMM_U64_FN)]


class HostComm:
    """hec_comm_ops over torch.distributed (a backend with MIN / MAX / SUM on CPU tensors: gloo): the sharded
    matvec's collectives on the host, for hec_comm_init_ops and hec_shard_agree.  Keeps the ctypes callbacks alive."""

    def __init__(self, group=None):
        import torch
        import torch.distributed as dist

        def f64(_user, buf, count, op):
            try:
                if count:
                    t = torch.from_numpy(np.ctypeslib.as_array(buf, shape=(count,)))
                    dist.all_reduce(t, op=dist.ReduceOp.MIN if op == REDUCE_MIN else dist.ReduceOp.MAX, group=group)
                return 0
            except Exception:  # noqa: BLE001 - reported to the engine as a failed collective
                return 1

        def u64(_user, buf, count):
            try:
                if count:  # residues < 2^60, world <= 8: the int64 sum is exact and non-negative
                    t = torch.from_numpy(np.ctypeslib.as_array(buf, shape=(count,)).view(np.int64))
                    dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
                return 0
            except Exception:  # noqa: BLE001
                return 1

        self._f64, self._u64 = COMM_F64_FN(f64), COMM_U64_FN(u64)
        self.ops = CommOps(None, self._f64, self._u64)


def shard_agree(comm: HostComm, rank: int, status: int, reason: str, scales) -> tuple[int, str]:
    """hec_shard_agree (host only): the sharded matvec's agreement step -> (agreed status, message)."""
    sc = np.ascontiguousarray(scales, dtype=np.float64)
    msg = C.create_string_buffer(512)
    rc = lib().hec_shard_agree(C.byref(comm.ops), rank, status, reason.encode(),
                               sc.ctypes.data_as(C.POINTER(C.c_double)), len(sc), msg, 512)
    return rc, msg.value.decode()


# ------------------------------------------------------------------ SEAL wire format (host side)
COMPR_NONE, COMPR_ZLIB, COMPR_ZSTD = 0, 1, 2


def _seal_check(rc):
    if rc != 0:
        msg = lib().hec_seal_last_error().decode()
        raise (InvalidArgument if rc == 1 else LogicError)(rc, msg)


def _bytes_in(b: bytes):
    return C.c_char_p(b), len(b)


def _sized_out(fn):
    """Call fn(out, cap, written) twice: size query, then into a buffer of that size."""
    n = C.c_uint64()
    _seal_check(fn(None, 0, C.byref(n)))
    buf = C.create_string_buffer(n.value)
    _seal_check(fn(buf, n.value, C.byref(n)))
    return buf.raw[: n.value]


def seal_blake2b(data: bytes, outlen=64) -> bytes:
    out = C.create_string_buffer(outlen)
    _seal_check(lib().hec_seal_blake2b(C.c_char_p(data), len(data), outlen, out))
    return out.raw


def seal_parms_id(N, moduli):
    m = np.ascontiguousarray(np.array(moduli, dtype=np.uint64))
    out = np.zeros(4, dtype=np.uint64)
    _seal_check(lib().hec_seal_parms_id(N, _p(m), len(m), _p(out)))
    return out


def seal_ciphertext_save(data: np.ndarray, scale: float, moduli, compr=COMPR_ZSTD) -> bytes:
    """Ciphertext::save of u64[size][level][N] (parms_id of its level from moduli)."""
    d = np.ascontiguousarray(data, dtype=np.uint64)
    m = np.ascontiguousarray(np.array(moduli, dtype=np.uint64))
    size, level, N = d.shape
    return _sized_out(lambda o, c, w: lib().hec_seal_ciphertext_save(_p(d), size, level, N, scale, _p(m), compr, o, c, w))


def _seed_words(seed):
    """A 64-byte prng_seed_type as 8 words (bytes, or 8 integers); None stays None (the library draws entropy)."""
    if seed is None:
        return None
    a = (np.frombuffer(bytes(seed), dtype=np.uint64) if isinstance(seed, (bytes, bytearray))
         else np.array(seed, dtype=np.uint64)).copy()
    if a.shape != (8,):
        raise InvalidArgument(HEC_EINVAL, "a seed is 64 bytes")
    return a


def seal_ciphertext_save_seeded(c0: np.ndarray, scale: float, moduli, prng_seed, compr=COMPR_ZSTD) -> bytes:
    """Serializable<Ciphertext>::save of encrypt_symmetric(plain): c0 u64[level][N] and the seed of c1
    (hec_seal_ciphertext_save_seeded; prng_seed = Context.encrypt_symmetric's public seed)."""
    d = np.ascontiguousarray(c0, dtype=np.uint64)
    m = np.ascontiguousarray(np.array(moduli, dtype=np.uint64))
    sd = _seed_words(prng_seed)
    level, N = d.shape
    return _sized_out(lambda o, c, w: lib().hec_seal_ciphertext_save_seeded(_p(d), level, N, scale, _p(m), _p(sd),
                                                                              compr, o, c, w))


def seal_blake2xb(data: bytes, key: bytes, outlen: int) -> bytes:
    """BLAKE2Xb XOF output (SEAL's Blake2xbPRNG core)."""
    out = C.create_string_buffer(outlen)
    _seal_check(lib().hec_seal_blake2xb(C.c_char_p(data), len(data), C.c_char_p(key), len(key), outlen, out))
    return out.raw


def seal_shake256(data: bytes, outlen: int) -> bytes:
    """SHAKE256 XOF output (SEAL's Shake256PRNG core)."""
    out = C.create_string_buffer(outlen)
    _seal_check(lib().hec_seal_shake256(C.c_char_p(data), len(data), outlen, out))
    return out.raw


def seal_ciphertext_load(b: bytes, moduli=None):
    """-> (data u64[size][level][N], scale, parms_id, bytes consumed).  With the context's data-level moduli a
    seeded ciphertext (encrypt_symmetric(...).save) is expanded as Ciphertext::expand_seed does."""
    size, level, N, used = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
    scale = C.c_double()
    pid = np.zeros(4, dtype=np.uint64)
    m = None if moduli is None else np.ascontiguousarray(np.array(moduli, dtype=np.uint64))
    mp, mc = (None, 0) if m is None else (_p(m), len(m))
    src, n = _bytes_in(b)
    _seal_check(lib().hec_seal_ciphertext_load_ex(src, n, mp, mc, C.byref(size), C.byref(level), C.byref(N),
                                                  C.byref(scale), _p(pid), None, 0, C.byref(used)))
    d = np.zeros((size.value, level.value, N.value), dtype=np.uint64)
    _seal_check(lib().hec_seal_ciphertext_load_ex(src, n, mp, mc, None, None, None, None, None, _p(d), d.size, None))
    return d, scale.value, pid, used.value


def seal_parms_save(N, moduli, compr=COMPR_NONE) -> bytes:
    m = np.ascontiguousarray(np.array(moduli, dtype=np.uint64))
    return _sized_out(lambda o, c, w: lib().hec_seal_parms_save(N, _p(m), len(m), compr, o, c, w))


def seal_parms_load(b: bytes):
    """EncryptionParameters::load -> (N, moduli, bytes consumed)"""
    N, k, used = C.c_uint64(), C.c_uint64(), C.c_uint64()
    src, n = _bytes_in(b)
    out = np.zeros(64, dtype=np.uint64)
    _seal_check(lib().hec_seal_parms_load(src, n, C.byref(N), _p(out), 64, C.byref(k), C.byref(used)))
    return N.value, [int(x) for x in out[: k.value]], used.value


def seal_kswitch_keys_save(N, moduli, key_lists, compr=COMPR_NONE) -> bytes:
    """KSwitchKeys::save: key_lists[i] = u64[L][2][K][N] or None (an empty list)."""
    m = np.ascontiguousarray(np.array(moduli, dtype=np.uint64))
    keep = [None if k is None else np.ascontiguousarray(k, dtype=np.uint64) for k in key_lists]
    ptrs = (u64p * max(1, len(keep)))(*[(_p(k) if k is not None else u64p()) for k in keep])
    digits = np.array([0 if k is None else k.shape[0] for k in keep] or [0], dtype=np.uint64)
    return _sized_out(lambda o, c, w: lib().hec_seal_kswitch_keys_save(N, _p(m), len(m), ptrs, _p(digits), len(keep),
                                                                     compr, o, c, w))


KEYLIST_VISIT = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint64, u64p, C.c_uint64)


def seal_kswitch_keys_lists(b: bytes, max_bytes=0, visit_status=0):
    """hec_seal_kswitch_keys_foreach[_ex]: every non-empty key list in one pass -> ({index: u64 words}, list count,
    bytes consumed).  max_bytes bounds the decompressed object (0: the library's default); a non-zero visit_status
    is what the visitor returns for the first list (the walk stops with that status)."""
    got = {}

    def visit(_user, index, words, nwords):
        got[int(index)] = np.ctypeslib.as_array(words, shape=(int(nwords),)).copy()
        return visit_status
    cb = KEYLIST_VISIT(visit)
    lists, used = C.c_uint64(), C.c_uint64()
    src, n = _bytes_in(b)
    rc = lib().hec_seal_kswitch_keys_foreach_ex(src, n, max_bytes, cb, None, C.byref(lists), C.byref(used))
    if rc != 0 and rc == visit_status:
        raise HecError(rc, lib().hec_seal_last_error().decode())
    _seal_check(rc)
    return got, lists.value, used.value


def seal_kswitch_keys_load(b: bytes, index, max_bytes=0):
    """key list `index` as u64 words (u64[L][2][K][N] flattened), and the object's list count"""
    lists, words, used = C.c_uint64(), C.c_uint64(), C.c_uint64()
    src, n = _bytes_in(b)
    _seal_check(lib().hec_seal_kswitch_keys_load_ex(src, n, index, max_bytes, C.byref(lists), None, 0, C.byref(words),
                                                    C.byref(used)))
    out = np.zeros(words.value, dtype=np.uint64)
    _seal_check(lib().hec_seal_kswitch_keys_load_ex(src, n, index, max_bytes, None, _p(out), out.size, None, None))
    return out, lists.value, used.value


def fft_twiddles(m, inverse=False) -> np.ndarray:
    """hec_fft_twiddles (host only): the m / 2 complex doubles pow(exp(-+2 pi i / m), k) as the reference's
    he::fft computes them (libstdc++'s exp and pow), the values hec_fft encodes for block size m."""
    re, im = np.empty(max(int(m) // 2, 1)), np.empty(max(int(m) // 2, 1))
    dp = C.POINTER(C.c_double)
    if lib().hec_fft_twiddles(int(m), int(bool(inverse)), re.ctypes.data_as(dp), im.ctypes.data_as(dp)) != 0:
        raise InvalidArgument(1, "m must be a power of two >= 2")
    return np.array([complex(a, b) for a, b in zip(re, im)])  # keeps a -0.0 imaginary part


def bfft_diagonal(d, k, n, inverse=False) -> np.ndarray:
    """hec_bfft_diagonal (host only): the n complex values of diagonal d (0, 1, 2) of the in-slot FFT's stage k = 2^i
    before tiling over slot_count (reference he_fft.cpp:89-153)."""
    re, im = np.empty(max(int(n), 1)), np.empty(max(int(n), 1))
    dp = C.POINTER(C.c_double)
    if lib().hec_bfft_diagonal(int(d), int(k), int(n), int(bool(inverse)), re.ctypes.data_as(dp),
                               im.ctypes.data_as(dp)) != 0:
        raise InvalidArgument(1, "bfft_diagonal: d in {0, 1, 2} (d = 2 needs k > 2), k <= n powers of two")
    return np.array([complex(a, b) for a, b in zip(re, im)])


MATH_SIGNED_INV, MATH_INV_SQRT_TWICE, MATH_SQRT, MATH_ABS = 0, 1, 2, 3


def math_plan(moduli, fn, a, iters, level, scale):
    """hec_math_plan (host only): the (level, scale) that Context.signed_inv / inv_sqrt_twice / sqrt / abs (fn =
    MATH_*) return for inputs at (level, scale) on the key moduli `moduli`; raises InvalidArgument with the message of
    the first check the per-operation schedule would fail."""
    m = np.array([int(x) for x in moduli], dtype=np.uint64)
    lv, sc = C.c_uint64(), C.c_double()
    _check(lib().hec_math_plan(_p(m), len(m), int(fn), float(a), int(iters), int(level), float(scale), C.byref(lv),
                               C.byref(sc)))
    return lv.value, sc.value


def math_poly_plan(moduli, coeffs, level, scale, bs=None):
    """hec_math_poly_plan (host only): (level, scale, bs, products, leaves) of Context.poly for inputs at (level,
    scale) on the key moduli `moduli`: the result's level and scale, the block size used, the relinearised products
    (powers included) and the linear-combination stages; raises InvalidArgument with the message of the first check
    the schedule would fail."""
    m = np.array([int(x) for x in moduli], dtype=np.uint64)
    cf = np.ascontiguousarray(np.asarray(coeffs, dtype=np.float64).ravel())
    if cf.size < 1:
        raise InvalidArgument(1, "polynomial must not be constant")
    lv, sc, be, pr, le = C.c_uint64(), C.c_double(), C.c_uint64(), C.c_uint64(), C.c_uint64()
    _check(lib().hec_math_poly_plan(_p(m), len(m), cf.ctypes.data_as(C.POINTER(C.c_double)), cf.size - 1,
                                    int(bs or 0), int(level), float(scale), C.byref(lv), C.byref(sc), C.byref(be),
                                    C.byref(pr), C.byref(le)))
    return lv.value, sc.value, be.value, pr.value, le.value


def sum_elems_plan(dim, cap=None):
    """hec_sum_elems_plan (host only): the rotation steps Context.sum_elems issues for dim, in order, the ones whose
    result the schedule discards included (dim = 1 rotates once and keeps the input).  cap: the size of the buffer
    handed to the engine (default: as many as the plan holds); with a smaller one, (steps written, count) is
    returned."""
    n = C.c_uint64()
    _check(lib().hec_sum_elems_plan(int(dim), None, 0, C.byref(n)))
    if cap is None:
        buf = (C.c_int * max(1, n.value))()
        _check(lib().hec_sum_elems_plan(int(dim), buf, n.value, C.byref(n)))
        return list(buf[:n.value])
    buf = (C.c_int * (int(cap) + 1))(*([-1] * (int(cap) + 1)))  # one guard word behind the cap
    _check(lib().hec_sum_elems_plan(int(dim), buf, int(cap), C.byref(n)))
    if buf[int(cap)] != -1:
        raise RuntimeError("hec_sum_elems_plan wrote past its cap")
    return list(buf[:min(int(cap), n.value)]), n.value


def bsgs_plan(n, bs=None):
    """hec_bsgs_plan (host only): (bs_eff, steps) of Context.matmul_diagpt_col_bsgs for an n x n matrix: the baby
    steps 1 .. bs_eff - 1, then the giant steps g * bs_eff.  bs=None picks the smallest power of two >= sqrt(n).  A key
    set with exactly these steps' elements makes every rotation one key switch."""
    cnt, eff = C.c_uint64(), C.c_uint64()
    b = 0 if bs is None else int(bs)
    if bs is not None and b < 1:
        raise InvalidArgument(HEC_EINVAL, "bs must be positive")
    _check(lib().hec_bsgs_plan(int(n), b, None, 0, C.byref(cnt), C.byref(eff)))
    buf = (C.c_int * max(1, cnt.value))()
    _check(lib().hec_bsgs_plan(int(n), b, buf, cnt.value, C.byref(cnt), C.byref(eff)))
    return eff.value, list(buf[:cnt.value])


DIAG_NATURAL, DIAG_BSGS = 0, 1  # include/hecdna.h HEC_DIAG_NATURAL, HEC_DIAG_BSGS


def colcolT_bsgs_plan(p, bs=None, form=0):
    """hec_colcolT_bsgs_plan (host only): (bs_eff, steps) of Context.matmul_col_colT_bsgs for p output diagonals: the
    baby steps 1 .. bs_eff - 1, the negative giant steps -g * bs_eff and, for form 0 (natural-form outputs) only, the
    positive giant steps g * bs_eff.  bs=None picks the smallest power of two >= sqrt(p)."""
    cnt, eff = C.c_uint64(), C.c_uint64()
    b = 0 if bs is None else int(bs)
    if bs is not None and b < 1:
        raise InvalidArgument(HEC_EINVAL, "bs must be positive")
    _check(lib().hec_colcolT_bsgs_plan(int(p), b, int(form), None, 0, C.byref(cnt), C.byref(eff)))
    buf = (C.c_int * max(1, cnt.value))()
    _check(lib().hec_colcolT_bsgs_plan(int(p), b, int(form), buf, cnt.value, C.byref(cnt), C.byref(eff)))
    return eff.value, list(buf[:cnt.value])


def bsgs_diagonals(diag_values, bs=None):
    """The BSGS form of n diagonals given as [n][slots] slot vectors (row j: diagonal j over all slots): row j rotated
    right by (j // bs_eff) * bs_eff slots, the vectors Context.matmul_diagpt_col_bsgs expects encoded."""
    d = np.asarray(diag_values)
    if d.ndim != 2:
        raise InvalidArgument(HEC_EINVAL, "diag_values must be [n][slots]")
    eff, _ = bsgs_plan(d.shape[0], bs)
    return np.stack([np.roll(d[j], (j // eff) * eff) for j in range(d.shape[0])])


def create_coeff_modulus(N, bits):
    out = np.zeros(len(bits), dtype=np.uint64)
    _check(lib().hec_create_coeff_modulus(N, (C.c_int * len(bits))(*bits), len(bits), _p(out)))
    return [int(x) for x in out]


class Context:
    """seal::SEALContext + seal::Evaluator on one GPU (one per process/device)."""

    def __init__(self, N, coeff_modulus, device=0):
        self.N = int(N)
        self.moduli = [int(x) for x in coeff_modulus]
        self.K = len(self.moduli)
        self.L = self.K - 1
        self.device = int(device)
        m = np.array(self.moduli, dtype=np.uint64)
        h = C.c_void_p()
        _check(lib().hec_context_create(self.N, _p(m), self.K, int(device), C.byref(h)))
        self.h = h

    def close(self):
        if self.h:
            lib().hec_context_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream_ptr):
        _check(lib().hec_context_set_stream(self.h, C.c_void_p(stream_ptr) if stream_ptr else None))

    def synchronize(self):
        _check(lib().hec_context_synchronize(self.h))

    def set_option(self, name: str, value: int):
        """hec_context_set_option: an engine knob (lanes, poison, lane_serial, hoist, ...) on the context and its
        batch lanes; every setting computes the same bits."""
        _check(lib().hec_context_set_option(self.h, name.encode(), int(value)))

    def elt_from_step(self, step):
        e = lib().hec_galois_elt_from_step(self.h, int(step))
        if e == 0:
            _check(1)
        return int(e)

    def default_galois_elts(self):
        n = lib().hec_default_galois_elts(self.h, None)
        out = (C.c_uint32 * n)()
        lib().hec_default_galois_elts(self.h, out)
        return list(out)

    # -------------------------------------------------------------- objects
    def ciphertext(self, data=None, scale=1.0):
        ct = Ciphertext(self)
        if data is not None:
            ct.upload(data, scale)
        return ct

    def plaintext(self, data, scale):
        return Plaintext(self, data, scale)

    def encode(self, values, scale, level=None):
        """seal::CKKSEncoder::encode on the GPU (hec_encode): `values` is one slot vector or a 2-D array of
        `count` vectors (real or complex, at most N/2 slots each) -> list of NTT-form Plaintexts (a single
        Plaintext for a 1-D input)."""
        v = np.asarray(values)
        single = v.ndim == 1
        v = v.reshape(1, -1) if single else v
        level = level or (self.K - 1)
        re = np.ascontiguousarray(v.real, dtype=np.float64)
        im = np.ascontiguousarray(v.imag, dtype=np.float64) if np.iscomplexobj(v) else None
        pts = [Plaintext(self, None, scale) for _ in range(v.shape[0])]
        arr = (C.c_void_p * len(pts))(*[p.h.value for p in pts])
        dp = C.POINTER(C.c_double)
        _check(lib().hec_encode(self.h, re.ctypes.data_as(dp), im.ctypes.data_as(dp) if im is not None else None,
                                v.shape[1], v.shape[0], float(scale), level, arr))
        return pts[0] if single else pts

    def encode_scalar(self, value, scale, level=None):
        """seal::CKKSEncoder::encode(double value, parms_id, scale, pt) (hec_encode_scalar): the constant plaintext
        he::util::drop_chain_levels and he::math multiply by (he_util.h:33)"""
        level = level or (self.K - 1)
        pt = Plaintext(self, None, scale)
        _check(lib().hec_encode_scalar(self.h, float(value), float(scale), level, pt.h))
        return pt

    def secret_key(self, data):
        """seal::SecretKey on the device (hec_secret_key_upload): data u64[K][N], NTT form at the key level"""
        return SecretKey(self, data)

    # -------------------------------------------------------------- KeyGenerator / Encryptor
    # seed: 64 bytes (or 8 words) that make the call's output a pure function of its arguments; None draws them
    # from the operating system.  A seed must never be reused across calls.
    @staticmethod
    def _seed(seed):
        a = _seed_words(seed)
        return (None if a is None else _p(a)), a

    def keygen_secret(self, seed=None):
        """KeyGenerator::secret_key() on the GPU (hec_keygen_secret)"""
        sp, _keep = self._seed(seed)
        h = C.c_void_p()
        _check(lib().hec_keygen_secret(self.h, sp, C.byref(h)))
        return SecretKey(self, None, handle=h)

    def keygen_public(self, sk, seed=None):
        """KeyGenerator::create_public_key (hec_keygen_public)"""
        sp, _keep = self._seed(seed)
        h = C.c_void_p()
        _check(lib().hec_keygen_public(self.h, sk.h, sp, C.byref(h)))
        return PublicKey(self, None, handle=h)

    def public_key(self, data):
        """seal::PublicKey on the device (hec_public_key_upload): data u64[2][K][N]"""
        return PublicKey(self, data)

    def keygen_relin(self, sk, seed=None):
        """KeyGenerator::create_relin_keys (hec_keygen_relin)"""
        sp, _keep = self._seed(seed)
        h = C.c_void_p()
        _check(lib().hec_keygen_relin(self.h, sk.h, sp, C.byref(h)))
        return KSwitchKey(self, handle=h)

    def keygen_galois(self, sk, elts=None, seed=None, gk=None):
        """KeyGenerator::create_galois_keys (hec_keygen_galois): the keys of `elts` (None: the default set) added to
        gk (a new GaloisKeys when None)"""
        sp, _keep = self._seed(seed)
        gk = gk or GaloisKeys(self)
        e = list(elts or [])
        arr = (C.c_uint32 * max(1, len(e)))(*e)
        _check(lib().hec_keygen_galois(gk.h, sk.h, arr, len(e), sp))
        return gk

    def encrypt_symmetric(self, sk, pts, seed=None, out=None, public_seeds=False):
        """Encryptor::encrypt_symmetric for a batch (hec_encrypt_symmetric; levels may differ).  public_seeds=True
        also returns u64[count][8], the seed of every c1 (for seal_ciphertext_save_seeded)."""
        single = isinstance(pts, Plaintext)
        pts = [pts] if single else list(pts)
        out = ([out] if single and out is not None else out) or [Ciphertext(self) for _ in pts]
        sp, _keep = self._seed(seed)
        ps = np.zeros((len(pts), 8), dtype=np.uint64) if public_seeds else None
        _check(lib().hec_encrypt_symmetric(self.h, sk.h, (C.c_void_p * max(1, len(pts)))(*[p.h.value for p in pts]),
                                           len(pts), sp, self._arr(out) if out else None,
                                           _p(ps) if ps is not None and ps.size else None))
        res = out[0] if single else out
        return (res, ps) if public_seeds else res

    def encrypt(self, pk, pts, seed=None, out=None):
        """Encryptor::encrypt with a public key for a batch (hec_encrypt)"""
        single = isinstance(pts, Plaintext)
        pts = [pts] if single else list(pts)
        out = ([out] if single and out is not None else out) or [Ciphertext(self) for _ in pts]
        sp, _keep = self._seed(seed)
        _check(lib().hec_encrypt(self.h, pk.h, (C.c_void_p * max(1, len(pts)))(*[p.h.value for p in pts]), len(pts),
                                 sp, self._arr(out) if out else None))
        return out[0] if single else out

    def _decoded(self, fn, handles, n_values, real):
        nv = self.N // 2 if n_values is None else int(n_values)
        re = np.zeros((len(handles), nv), dtype=np.float64)
        im = None if real else np.zeros((len(handles), nv), dtype=np.float64)
        arr = (C.c_void_p * max(1, len(handles)))(*handles)
        dp = C.POINTER(C.c_double)
        _check(fn(arr, len(handles), nv, re.ctypes.data_as(dp), im.ctypes.data_as(dp) if im is not None else None))
        if real:
            return re
        out = np.empty(re.shape, dtype=np.complex128)
        out.real, out.imag = re, im
        return out

    def decrypt(self, sk, cts):
        """seal::Decryptor::decrypt for a batch (hec_decrypt; sizes and levels may differ): one NTT-form Plaintext
        per ciphertext, with its level and scale (a single Plaintext for a single Ciphertext)."""
        single = isinstance(cts, Ciphertext)
        cts = [cts] if single else list(cts)
        pts = [Plaintext(self, None, 1.0) for _ in cts]
        _check(lib().hec_decrypt(self.h, sk.h, (C.c_void_p * max(1, len(cts)))(*[c.h.value for c in cts]), len(cts),
                                 (C.c_void_p * max(1, len(pts)))(*[p.h.value for p in pts])))
        return pts[0] if single else pts

    def decode(self, pts, n_values=None, real=False):
        """seal::CKKSEncoder::decode for a batch (hec_decode): the first n_values (default N/2) slots of every
        plaintext as a complex128 array [count][n_values] (float64 with real=True, SEAL's vector<double> overload);
        one row for a single Plaintext."""
        single = isinstance(pts, Plaintext)
        pts = [pts] if single else list(pts)
        out = self._decoded(lambda *a: lib().hec_decode(self.h, *a), [p.h.value for p in pts], n_values, real)
        return out[0] if single else out

    def decrypt_decode(self, sk, cts, n_values=None, real=False):
        """decrypt + decode in one pass with no Plaintext objects in between (hec_decrypt_decode): the doubles of
        decode(decrypt(sk, cts))."""
        single = isinstance(cts, Ciphertext)
        cts = [cts] if single else list(cts)
        out = self._decoded(lambda *a: lib().hec_decrypt_decode(self.h, sk.h, *a), [c.h.value for c in cts],
                            n_values, real)
        return out[0] if single else out

    def relin_key(self, data=None, seed=None):
        return KSwitchKey(self, data, seed)

    def galois_keys(self, keys: dict | None = None, uniform_elts=None, seed=0):
        g = GaloisKeys(self)
        for e, d in (keys or {}).items():
            g.add(e, d)
        for i, e in enumerate(uniform_elts or []):
            g.add_uniform(e, seed + 7919 * i)
        return g

    # -------------------------------------------------------------- evaluator (in place)
    def negate(self, a):
        _check(lib().hec_negate_inplace(self.h, a.h)); return a

    def add(self, a, b):
        _check(lib().hec_add_inplace(self.h, a.h, b.h)); return a

    def sub(self, a, b):
        _check(lib().hec_sub_inplace(self.h, a.h, b.h)); return a

    def add_plain(self, a, p):
        _check(lib().hec_add_plain_inplace(self.h, a.h, p.h)); return a

    def sub_plain(self, a, p):
        _check(lib().hec_sub_plain_inplace(self.h, a.h, p.h)); return a

    def multiply(self, a, b):
        _check(lib().hec_multiply_inplace(self.h, a.h, b.h)); return a

    def multiply_plain(self, a, p):
        _check(lib().hec_multiply_plain_inplace(self.h, a.h, p.h)); return a

    def square(self, a):
        _check(lib().hec_square_inplace(self.h, a.h)); return a

    def relinearize(self, a, rk):
        _check(lib().hec_relinearize_inplace(self.h, a.h, rk.h)); return a

    def rescale_to_next(self, a):
        _check(lib().hec_rescale_to_next_inplace(self.h, a.h)); return a

    def mod_switch_to_next(self, a):
        _check(lib().hec_mod_switch_to_next_inplace(self.h, a.h)); return a

    def rotate_vector(self, a, steps, gk):
        _check(lib().hec_rotate_vector_inplace(self.h, a.h, int(steps), gk.h)); return a

    def apply_galois(self, a, elt, gk):
        _check(lib().hec_apply_galois_inplace(self.h, a.h, int(elt), gk.h)); return a

    # -------------------------------------------------------------- linalg
    @staticmethod
    def _arr(cts):
        # None entries pass a null handle (diagonals a sharded rank does not hold; never dereferenced)
        return (C.c_void_p * len(cts))(*[(c.h if c is not None else None) for c in cts])

    def matmul_diag_col(self, diags, cols, rk, gk, out=None):
        out = out or [Ciphertext(self) for _ in cols]
        _check(lib().hec_matmul_diag_col(self.h, self._arr(diags), len(diags), self._arr(cols), len(cols), rk.h,
                                         gk.h, self._arr(out)))
        return out

    def comm_init(self, rank, world, unique_id: bytes | None = None):
        buf = C.create_string_buffer(unique_id, 128) if unique_id is not None else None
        _check(lib().hec_comm_init(self.h, rank, world, buf))

    def comm_init_ops(self, rank, world, comm: HostComm):
        """hec_comm_init_ops: the sharded matvec over the caller's host collectives (e.g. gloo)."""
        self._host_comm = comm  # the engine keeps the callbacks
        _check(lib().hec_comm_init_ops(self.h, rank, world, C.byref(comm.ops)))

    def matmul_diag_col_sharded(self, diags, cols, rk, gk, out=None):
        """hec_matmul_diag_col_sharded: every rank calls it; returns all p outputs on every rank."""
        out = out or [Ciphertext(self) for _ in cols]
        _check(lib().hec_matmul_diag_col_sharded(self.h, self._arr(diags), len(diags), self._arr(cols), len(cols),
                                                 rk.h, gk.h, self._arr(out)))
        return out

    def matmul_diagpt_col(self, pdiags, cols, gk, out=None):
        """ct x pt matvec: plaintext diagonals (multiply_plain), one rescale per output, no relin."""
        out = out or [Ciphertext(self) for _ in cols]
        _check(lib().hec_matmul_diagpt_col(self.h, self._arr(pdiags), len(pdiags), self._arr(cols), len(cols), gk.h,
                                           self._arr(out)))
        return out

    def matmul_diagpt_col_bsgs(self, pdiags, cols, gk, bs=None, out=None):
        """hec_matmul_diagpt_col_bsgs: the ct x pt matvec from (bs_eff - 1) + (ceil(n / bs_eff) - 1) rotations.  pdiags
        are the encodings of bsgs_diagonals(...) for the same bs.  Decrypts to matmul_diagpt_col's product; its
        ciphertext bits are those of the per-operation composition in the schedule's order, not the reference
        loop's (they coincide for bs >= n)."""
        out = out or [Ciphertext(self) for _ in cols]
        b = 0 if bs is None else int(bs)
        if bs is not None and b < 1:
            raise InvalidArgument(HEC_EINVAL, "bs must be positive")
        _check(lib().hec_matmul_diagpt_col_bsgs(self.h, self._arr(pdiags), len(pdiags), b, self._arr(cols), len(cols),
                                                gk.h, self._arr(out)))
        return out

    def matmul_diag_col_bsgs(self, diags, cols, rk, gk, bs=None, out=None):
        """hec_matmul_diag_col_bsgs: the ct x ct matvec from (bs_eff - 1) baby rotations, ceil(n / bs_eff)
        relinearisations and as many giant rotations less one.  diags encrypt the rows of bsgs_diagonals(...) for the
        same bs (or come from bsgs_rotate_diagonals).  Decrypts to matmul_diag_col's product; its ciphertext bits are
        those of the per-operation composition in the schedule's order, not the reference loop's (they coincide for
        bs >= n).  bs_eff is at most 512."""
        out = out or [Ciphertext(self) for _ in cols]
        b = 0 if bs is None else int(bs)
        if bs is not None and b < 1:
            raise InvalidArgument(HEC_EINVAL, "bs must be positive")
        _check(lib().hec_matmul_diag_col_bsgs(self.h, self._arr(diags), len(diags), b, self._arr(cols), len(cols),
                                              rk.h, gk.h, self._arr(out)))
        return out

    def bsgs_rotate_diagonals(self, diags, bs, gk):
        """The BSGS form of a matrix whose ciphertext diagonals arrive in natural form: copies of diags with diags[j]
        rotated right by (j // bs_eff) * bs_eff slots (rotate_vector by the negative step, so gk needs keys for the
        negative giant steps or their NAF chains).  Once per matrix, one rotation at a time; every rotation adds
        key-switch noise to its diagonal, which bsgs_diagonals before encryption does not."""
        eff, _ = bsgs_plan(len(diags), bs)
        out = [d.copy() for d in diags]
        for j, d in enumerate(out):
            if j // eff:
                self.rotate_vector(d, -(j // eff) * eff, gk)
        return out

    def matmul_diag_col_partial(self, diags, j_begin, j_end, cols, gk, out=None):
        out = out or [Ciphertext(self) for _ in cols]
        _check(lib().hec_matmul_diag_col_partial(self.h, self._arr(diags), len(diags), j_begin, j_end,
                                                 self._arr(cols), len(cols), gk.h, self._arr(out)))
        return out

    def matmul_diag_col_partial_set(self, diags, js, cols, gk, out=None):
        out = out or [Ciphertext(self) for _ in cols]
        idx = np.ascontiguousarray(js, dtype=np.uint64)
        _check(lib().hec_matmul_diag_col_partial_set(self.h, self._arr(diags), len(diags), _p(idx), len(idx),
                                                     self._arr(cols), len(cols), gk.h, self._arr(out)))
        return out

    def matmul_finish(self, accs, rk, out=None):
        out = out or [Ciphertext(self) for _ in accs]
        _check(lib().hec_matmul_finish(self.h, self._arr(accs), len(accs), rk.h, self._arr(out)))
        return out

    # -------------------------------------------------------------- he::fft
    def fft(self, cts, inverse=False, out=None):
        """hec_fft: he::fft::fft / ifft over the list of ciphertexts (a power of two of them)."""
        out = out or [Ciphertext(self) for _ in cts]
        _check(lib().hec_fft(self.h, self._arr(cts), len(cts), int(bool(inverse)), self._arr(out)))
        return out

    def bfft(self, cts, n, gk, inverse=False, out=None):
        """hec_bfft: he::fft::bfft / ibfft with block size n on every ciphertext of the list (or on one
        ciphertext, then one is returned)."""
        single = isinstance(cts, Ciphertext)
        cts = [cts] if single else list(cts)
        out = out or [Ciphertext(self) for _ in cts]
        _check(lib().hec_bfft(self.h, self._arr(cts), len(cts), int(n), int(bool(inverse)), gk.h, self._arr(out)))
        return out[0] if single else out

    # -------------------------------------------------------------- he::math
    def _math(self, fn, cts, a, iters, rk, out):
        single = isinstance(cts, Ciphertext)
        cts = [cts] if single else list(cts)
        if out is None:
            out = [Ciphertext(self) for _ in cts]
        elif isinstance(out, Ciphertext):
            out = [out]
        _check(fn(self.h, self._arr(cts), len(cts), float(a), int(iters), rk.h, self._arr(out)))
        return out[0] if single else out

    def signed_inv(self, cts, a, iters, rk, out=None):
        """hec_math_signed_inv: he::math::signed_inv on every ciphertext of the list (or on one, then one is
        returned), 1 / x from the guess a with |a x - 1| < 1."""
        return self._math(lib().hec_math_signed_inv, cts, a, iters, rk, out)

    def inv_sqrt_twice(self, cts, a, iters, rk, out=None):
        """hec_math_inv_sqrt_twice: he::math::inv_sqrt_twice, 1 / sqrt(2 x) from the guess a."""
        return self._math(lib().hec_math_inv_sqrt_twice, cts, a, iters, rk, out)

    def sqrt(self, cts, a, iters, rk, out=None):
        """hec_math_sqrt: he::math::sqrt."""
        return self._math(lib().hec_math_sqrt, cts, a, iters, rk, out)

    def abs(self, cts, a, iters, rk, out=None):
        """hec_math_abs: he::math::abs."""
        return self._math(lib().hec_math_abs, cts, a, iters, rk, out)

    def poly(self, cts, coeffs, rk, bs=None, out=None):
        """hec_math_poly: sum_j coeffs[j] x^j on every ciphertext of the list (or on one, then one is returned) by
        Paterson-Stockmeyer with block size bs (None: chosen from the degree).  The result keeps the input's scale."""
        single = isinstance(cts, Ciphertext)
        cts = [cts] if single else list(cts)
        if out is None:
            out = [Ciphertext(self) for _ in cts]
        elif isinstance(out, Ciphertext):
            out = [out]
        cf = np.ascontiguousarray(np.asarray(coeffs, dtype=np.float64).ravel())
        if cf.size < 1:
            raise InvalidArgument(1, "polynomial must not be constant")
        _check(lib().hec_math_poly(self.h, self._arr(cts), len(cts), cf.ctypes.data_as(C.POINTER(C.c_double)),
                                   cf.size - 1, int(bs or 0), rk.h, self._arr(out)))
        return out[0] if single else out

    def drop_chain_levels(self, cts, levels):
        """hec_drop_chain_levels: he::util::drop_chain_levels on the ciphertext(s), in place."""
        single = isinstance(cts, Ciphertext)
        lst = [cts] if single else list(cts)
        _check(lib().hec_drop_chain_levels(self.h, self._arr(lst), len(lst), int(levels)))
        return cts

    # -------------------------------------------------------------- he::linalg element-wise products and sums
    def _batch(self, cts, out):
        single = isinstance(cts, Ciphertext)
        cts = [cts] if single else list(cts)
        if out is None:
            out = [Ciphertext(self) for _ in cts]
        elif isinstance(out, Ciphertext):
            out = [out]
        return single, cts, out

    def multiply_relin_rescale(self, a, b, rk, out=None):
        """hec_multiply_relin_rescale_many: rescale_to_next(relinearize(a[i] * b[i], rk)) for every pair of the lists
        (or for one pair, then one ciphertext is returned); b is a, or equal handles, squares.  The entries may sit
        at different levels and scales."""
        single, la, out = self._batch(a, out)
        lb = la if b is a else ([b] if isinstance(b, Ciphertext) else list(b))
        if len(lb) != len(la):
            raise ValueError("a and b must have the same length")
        _check(lib().hec_multiply_relin_rescale_many(self.h, self._arr(la), self._arr(lb), len(la), rk.h,
                                                     self._arr(out)))
        return out[0] if single else out

    def sum_elems(self, cts, dim, gk, out=None):
        """hec_sum_elems_many: BatchedVector::sum_elems_inplace with this dim on every ciphertext of the list (or on
        one, then one is returned); gk must hold the key of every step of sum_elems_plan(dim)."""
        single, cts, out = self._batch(cts, out)
        _check(lib().hec_sum_elems_many(self.h, self._arr(cts), len(cts), int(dim), gk.h, self._arr(out)))
        return out[0] if single else out

    def reduce(self, ct):
        """Reduce every word of ct mod its prime (after a partial-sum exchange)."""
        _check(lib().hec_ciphertext_reduce(self.h, ct.h)); return ct

    def matmul_col_colT(self, A, B, p, rk, gk):
        out = [Ciphertext(self) for _ in range(p)]
        _check(lib().hec_matmul_col_colT(self.h, self._arr(A), len(A), self._arr(B), p, rk.h, gk.h,
                                         self._arr(out)))
        return out

    def matmul_col_colT_bsgs(self, A, B, p, rk, gk, bs=None, bsgs_form=False, out=None):
        """hec_matmul_col_colT_bsgs: matmul_col_colT's product from (bs_eff - 1) baby rotations of every B[j] and
        ceil(p / bs_eff) - 1 giant rotations of every A[j].  bsgs_form=False: the p diagonals in natural form, as
        matmul_col_colT gives them (one more rotation per output past the first block).  bsgs_form=True: diagonal i
        rotated right by (i // bs_eff) * bs_eff slots, what matmul_diag_col_bsgs takes for the same bs, with no
        rotation of the outputs at all.  Its ciphertext bits are those of the per-operation composition in the
        schedule's order, not matmul_col_colT's (they coincide for bs >= p)."""
        out = out or [Ciphertext(self) for _ in range(p)]
        b = 0 if bs is None else int(bs)
        if bs is not None and b < 1:
            raise InvalidArgument(HEC_EINVAL, "bs must be positive")
        form = bsgs_form if isinstance(bsgs_form, int) and not isinstance(bsgs_form, bool) else int(bool(bsgs_form))
        _check(lib().hec_matmul_col_colT_bsgs(self.h, self._arr(A), len(A), self._arr(B), int(p), b, form, rk.h, gk.h,
                                              self._arr(out)))
        return out

    def matrix_matmul(self, A, ar, ac, atr, B, br, bc, btr, rk):
        r1 = ac if atr else ar
        c2 = br if btr else bc
        out = [Ciphertext(self) for _ in range(r1 * c2)]
        _check(lib().hec_matrix_matmul(self.h, self._arr(A), ar, ac, int(atr), self._arr(B), br, bc, int(btr),
                                       rk.h, self._arr(out)))
        return out

    # -------------------------------------------------------------- primitives
    def ntt(self, host: np.ndarray, limb0=0, inverse=False):
        """host u64[npolys][nlimbs][N] -> transformed copy (device round trip)."""
        a = np.ascontiguousarray(host, dtype=np.uint64)
        npolys, nl = (a.shape[0], a.shape[1]) if a.ndim == 3 else (1, a.shape[0])
        buf = DeviceBuffer(self, a.nbytes)
        buf.upload(a)
        fn = lib().hec_ntt_inverse if inverse else lib().hec_ntt_forward
        _check(fn(self.h, buf.p, limb0, nl, npolys))
        return buf.download(a.shape)

    def ntt_device(self, buf, nl, npolys, limb0=0, inverse=False):
        """in place on device words u64[npolys][nl][N] (hec_ntt_forward / hec_ntt_inverse, stream ordered)"""
        fn = lib().hec_ntt_inverse if inverse else lib().hec_ntt_forward
        _check(fn(self.h, buf.p, limb0, nl, npolys))

    def dyadic_device(self, a, b, out, nl, npolys, limb0=0):
        """out = a (*) b on device words u64[npolys][nl][N] (hec_dyadic_multiply, stream ordered)"""
        _check(lib().hec_dyadic_multiply(self.h, a.p, b.p, out.p, limb0, nl, npolys))

    def dyadic_multiply(self, a: np.ndarray, b: np.ndarray, limb0=0):
        """a, b host u64[npolys][nlimbs][N] -> (a * b) mod q_(limb0 + limb) (device round trip)."""
        a = np.ascontiguousarray(a, dtype=np.uint64)
        b = np.ascontiguousarray(b, dtype=np.uint64)
        if a.shape != b.shape or a.ndim != 3:
            raise InvalidArgument(1, "operands must have the same shape u64[npolys][nlimbs][N]")
        bufs = [DeviceBuffer(self, a.nbytes) for _ in range(3)]
        bufs[0].upload(a)
        bufs[1].upload(b)
        _check(lib().hec_dyadic_multiply(self.h, bufs[0].p, bufs[1].p, bufs[2].p, limb0, a.shape[1], a.shape[0]))
        return bufs[2].download(a.shape)

    def profile(self, mode=1):
        """0 off, 1 synchronous per phase, 2 asynchronous event pairs (resolved by profile_read)."""
        _check(lib().hec_profile_enable(self.h, int(mode)))

    def profile_read(self, cls):
        ms = C.c_double()
        n = C.c_uint64()
        _check(lib().hec_profile_read(self.h, cls.encode(), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def profile_read_ex(self, cls):
        """(ms, scopes, algorithmic bytes, kernel launches) of one profile class."""
        ms, n, b, kl = C.c_double(), C.c_uint64(), C.c_double(), C.c_uint64()
        _check(lib().hec_profile_read_ex(self.h, cls.encode(), C.byref(ms), C.byref(n), C.byref(b), C.byref(kl)))
        return ms.value, n.value, b.value, kl.value

    def profile_classes(self):
        need = lib().hec_profile_classes(self.h, None, 0)
        buf = C.create_string_buffer(int(need))
        lib().hec_profile_classes(self.h, buf, need)
        return [x for x in buf.value.decode().split("\n") if x]


class DeviceBuffer:
    def __init__(self, ctx: Context, nbytes):
        self.ctx = ctx
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        _check(lib().hec_device_alloc(ctx.h, self.nbytes, C.byref(p)))
        self.p = p

    def upload(self, a):
        a = np.ascontiguousarray(a)
        _check(lib().hec_memcpy_h2d(self.ctx.h, self.p, a.ctypes.data_as(C.c_void_p), a.nbytes))

    def download(self, shape, dtype=np.uint64):
        out = np.empty(shape, dtype=dtype)
        _check(lib().hec_memcpy_d2h(self.ctx.h, out.ctypes.data_as(C.c_void_p), self.p, out.nbytes))
        return out

    def __del__(self):
        try:
            if self.p:
                lib().hec_device_free(self.ctx.h, self.p)
                self.p = None
        except Exception:
            pass


class _DeviceObject:
    """A device object of a context: its context, its C handle `h` and the name of the C call that destroys it.  The
    object may be finalised before or after its context, on any thread (hecdna.h)."""
    _destroy = None
    ctx = None
    h = None

    def __del__(self):
        try:
            if self.h:
                getattr(lib(), self._destroy)(self.h)
                self.h = None
        except Exception:
            pass


class Ciphertext(_DeviceObject):
    _destroy = "hec_ciphertext_destroy"

    def __init__(self, ctx: Context):
        self.ctx = ctx
        h = C.c_void_p()
        _check(lib().hec_ciphertext_create(ctx.h, C.byref(h)))
        self.h = h

    def upload(self, data: np.ndarray, scale: float):
        a = np.ascontiguousarray(data, dtype=np.uint64)
        _check(lib().hec_ciphertext_upload(self.h, _p(a), a.shape[0], a.shape[1], float(scale)))
        return self

    def fill_uniform(self, size, level, scale, seed):
        _check(lib().hec_ciphertext_fill_uniform(self.h, size, level, float(scale), seed))
        return self

    def info(self):
        s, l, sc = C.c_uint64(), C.c_uint64(), C.c_double()
        _check(lib().hec_ciphertext_info(self.h, C.byref(s), C.byref(l), C.byref(sc)))
        return s.value, l.value, sc.value

    @property
    def scale(self):
        return self.info()[2]

    def download(self):
        s, l, _ = self.info()
        out = np.empty((s, l, self.ctx.N), dtype=np.uint64)
        _check(lib().hec_ciphertext_download(self.h, _p(out)))
        return out

    def export_device(self, dev_ptr):
        """Copy the u64[size][level][N] words into device memory at dev_ptr (stream ordered)."""
        _check(lib().hec_ciphertext_export_device(self.h, C.c_void_p(dev_ptr)))

    def import_device(self, dev_ptr, size, level, scale):
        _check(lib().hec_ciphertext_import_device(self.h, C.c_void_p(dev_ptr), size, level, float(scale)))
        return self

    def copy(self):
        if not self.ctx.h:  # closed: hec_ciphertext_copy's answer, before a destination is asked of no context
            raise InvalidArgument(HEC_EINVAL, "encrypted is not valid for encryption parameters")
        c = Ciphertext(self.ctx)
        _check(lib().hec_ciphertext_copy(c.h, self.h))
        return c

    def load_seal(self, b: bytes):
        """Ciphertext::load(context, in, size) from SEAL's wire format; returns the bytes read."""
        used = C.c_uint64()
        _check(lib().hec_ciphertext_load_seal(self.h, C.c_char_p(b), len(b), C.byref(used)))
        return used.value

    def save_seal(self, compr=COMPR_ZSTD) -> bytes:
        """Ciphertext::save(stream, compr_mode) in SEAL's wire format."""
        n = C.c_uint64()
        _check(lib().hec_ciphertext_save_seal(self.h, compr, None, 0, C.byref(n)))
        buf = C.create_string_buffer(n.value)
        _check(lib().hec_ciphertext_save_seal(self.h, compr, buf, n.value, C.byref(n)))
        return buf.raw[: n.value]


class Plaintext(_DeviceObject):
    _destroy = "hec_plaintext_destroy"

    def __init__(self, ctx: Context, data, scale):
        self.ctx = ctx
        h = C.c_void_p()
        _check(lib().hec_plaintext_create(ctx.h, C.byref(h)))
        self.h = h
        if data is not None:
            a = np.ascontiguousarray(data, dtype=np.uint64)
            _check(lib().hec_plaintext_upload(self.h, _p(a), a.shape[0], float(scale)))

    def fill_uniform(self, level, scale, seed):
        _check(lib().hec_plaintext_fill_uniform(self.h, level, float(scale), seed))
        return self

    def info(self):
        lv, sc = C.c_uint64(), C.c_double()
        _check(lib().hec_plaintext_info(self.h, C.byref(lv), C.byref(sc)))
        return lv.value, sc.value

    def download(self):
        lv, _ = self.info()
        out = np.empty((lv, self.ctx.N), dtype=np.uint64)
        _check(lib().hec_plaintext_download(self.h, _p(out)))
        return out


class SecretKey(_DeviceObject):
    """seal::SecretKey on the device: u64[K][N], NTT form at the key level; wiped when destroyed."""
    _destroy = "hec_secret_key_destroy"

    def __init__(self, ctx: Context, data, handle=None):
        self.ctx = ctx
        if handle is not None:  # made on the device (Context.keygen_secret)
            self.h = handle
            return
        a = np.ascontiguousarray(data, dtype=np.uint64)
        if a.shape != (ctx.K, ctx.N):
            raise InvalidArgument(HEC_EINVAL, "secret key is not valid for encryption parameters")
        h = C.c_void_p()
        _check(lib().hec_secret_key_upload(ctx.h, _p(a), C.byref(h)))
        self.h = h

    def download(self):
        a = np.empty((self.ctx.K, self.ctx.N), dtype=np.uint64)
        _check(lib().hec_secret_key_download(self.h, _p(a)))
        return a


class PublicKey(_DeviceObject):
    """seal::PublicKey on the device: u64[2][K][N], NTT form at the key level."""
    _destroy = "hec_public_key_destroy"

    def __init__(self, ctx: Context, data, handle=None):
        self.ctx = ctx
        self.h = None
        if handle is not None:  # made on the device (Context.keygen_public)
            self.h = handle
            return
        a = np.ascontiguousarray(data, dtype=np.uint64)
        if a.shape != (2, ctx.K, ctx.N):
            raise InvalidArgument(HEC_EINVAL, "public key is not valid for encryption parameters")
        h = C.c_void_p()
        _check(lib().hec_public_key_upload(ctx.h, _p(a), C.byref(h)))
        self.h = h

    def download(self):
        a = np.empty((2, self.ctx.K, self.ctx.N), dtype=np.uint64)
        _check(lib().hec_public_key_download(self.h, _p(a)))
        return a


class KSwitchKey(_DeviceObject):
    _destroy = "hec_kswitch_key_destroy"

    def __init__(self, ctx: Context, data=None, seed=None, seal_bytes: bytes | None = None, handle=None):
        self.ctx = ctx
        h = C.c_void_p()
        if handle is not None:  # made on the device (Context.keygen_relin)
            h = handle
        elif seal_bytes is not None:  # RelinKeys::load(context, in, size)
            used = C.c_uint64()
            _check(lib().hec_kswitch_key_load_seal(ctx.h, C.c_char_p(seal_bytes), len(seal_bytes), C.byref(h),
                                                   C.byref(used)))
        elif data is not None:
            a = np.ascontiguousarray(data, dtype=np.uint64)
            _check(lib().hec_kswitch_key_upload(ctx.h, _p(a), C.byref(h)))
        else:
            _check(lib().hec_kswitch_key_fill_uniform(ctx.h, int(seed or 0), C.byref(h)))
        self.h = h

    def download(self):
        """u64[L][2][K][N] (hec_kswitch_key_download)"""
        c = self.ctx
        a = np.empty((c.L, 2, c.K, c.N), dtype=np.uint64)
        _check(lib().hec_kswitch_key_download(self.h, _p(a)))
        return a


class GaloisKeys(_DeviceObject):
    _destroy = "hec_galois_keys_destroy"

    def __init__(self, ctx: Context):
        self.ctx = ctx
        h = C.c_void_p()
        _check(lib().hec_galois_keys_create(ctx.h, C.byref(h)))
        self.h = h

    def add(self, elt, data):
        a = np.ascontiguousarray(data, dtype=np.uint64)
        _check(lib().hec_galois_keys_add(self.h, int(elt), _p(a)))

    def add_uniform(self, elt, seed):
        _check(lib().hec_galois_keys_add_uniform(self.h, int(elt), int(seed)))

    def has(self, elt):
        return bool(lib().hec_galois_keys_has(self.h, int(elt)))

    def download(self, elt):
        """the key of one Galois element, u64[L][2][K][N] (hec_galois_keys_download)"""
        c = self.ctx
        a = np.empty((c.L, 2, c.K, c.N), dtype=np.uint64)
        _check(lib().hec_galois_keys_download(self.h, int(elt), _p(a)))
        return a

    def load_seal(self, b: bytes, max_lists=None):
        """GaloisKeys::load(context, in, size): every key list of a SEAL-serialized GaloisKeys (at most max_lists
        non-empty lists; None: the library's fixed default, hec_galois_keys_load_seal_default_lists)."""
        used = C.c_uint64()
        if max_lists is None:
            _check(lib().hec_galois_keys_load_seal(self.h, C.c_char_p(b), len(b), C.byref(used)))
        else:
            _check(lib().hec_galois_keys_load_seal_ex(self.h, C.c_char_p(b), len(b), int(max_lists), C.byref(used)))
        return used.value
