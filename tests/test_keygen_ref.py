"""KeyGenerator / Encryptor, host side (no GPU): the seeded-ciphertext writer against the restated layout, byte for
byte in all three compression modes; its load expands c1 as Ciphertext::expand_seed; the Python restatement of the
key generation and encryption (tests/keygen_ref.py) makes keys and ciphertexts that the CPU oracle decrypts, rotates
and relinearizes; the new symbols are exported."""
import ctypes
import ctypes.util
import struct
import subprocess
import zlib

import numpy as np
import pytest

import keygen_ref as kr
import seal_format as sf

N = 1 << 10
BITS = [60, 40, 40, 60]
SEED = bytes(range(64))
SCALE = 2.0 ** 30


def zstd_decompress(body: bytes, cap: int) -> bytes:
    z = ctypes.CDLL(ctypes.util.find_library("zstd") or "libzstd.so.1")
    z.ZSTD_decompress.restype = ctypes.c_size_t
    z.ZSTD_decompress.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t]
    out = ctypes.create_string_buffer(cap)
    n = z.ZSTD_decompress(out, cap, body, len(body))
    assert n <= cap, "zstd error"
    return out.raw[:n]


NEW = ["hec_keygen_secret", "hec_keygen_public", "hec_public_key_upload", "hec_public_key_download",
       "hec_public_key_destroy", "hec_keygen_relin", "hec_keygen_galois", "hec_encrypt_symmetric", "hec_encrypt",
       "hec_seal_ciphertext_save_seeded"]


def test_new_symbols_declared_and_exported(hecdna):
    declared = hecdna.exported_symbols()
    out = subprocess.check_output(["nm", "-D", "--defined-only", hecdna.LIB_PATH]).decode()
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for s in NEW:
        assert s in declared and s in exported, s
    for name in ("keygen_secret", "keygen_public", "keygen_relin", "keygen_galois", "encrypt_symmetric", "encrypt"):
        assert callable(getattr(hecdna.Context, name))
    assert hecdna.PublicKey and callable(hecdna.seal_ciphertext_save_seeded)


def test_sub_seed_host_equals_python(hecdna):
    """the library's host BLAKE2Xb (LibStream, used for the larger cases) and the pure-Python one agree on a sub-seed
    and on a stream's first buffers"""
    a, b = kr.Streams(hecdna), kr.Streams(None)
    sub = a.sub(SEED, 4, 1, 2, 2047)
    assert sub == b.sub(SEED, 4, 1, 2, 2047) and len(sub) == 64
    assert a.open(sub).take(4096 + 100) == b.open(sub).take(4096 + 100)


@pytest.mark.parametrize("compr", [0, 1, 2])
@pytest.mark.parametrize("level", [1, 3])
def test_seeded_writer_matches_restated_layout(hecdna, orc, compr, level):
    m = orc.Oracle.create_coeff_modulus(N, BITS)
    rng = np.random.default_rng(level)
    c0 = np.stack([rng.integers(0, q, N, dtype=np.uint64) for q in m[:level]])
    data = np.stack([c0, np.zeros_like(c0)])
    plain = sf.ciphertext(data, SCALE, m, seeded_c0_only=True, seed=SEED)
    got = hecdna.seal_ciphertext_save_seeded(c0, SCALE, m, SEED, compr=compr)
    if compr == 0:
        assert got == plain
    else:
        magic, hs, vmaj, vmin, cm, res, total = struct.unpack("<HBBBBHQ", got[:16])
        assert (magic, hs, vmaj, vmin, cm, res, total) == (sf.MAGIC, 16, 4, 1, compr, 0, len(got))
        body = zlib.decompress(got[16:]) if compr == 1 else zstd_decompress(got[16:], len(plain))
        assert body == plain[16:]
    if compr == 1:
        assert got == sf.ciphertext(data, SCALE, m, seeded_c0_only=True, seed=SEED, compr=1)
    # and its load expands c1 from the seed
    d, scale, pid, used = hecdna.seal_ciphertext_load(got, m[:3])
    assert used == len(got) and scale == SCALE and d.shape == (2, level, N)
    assert np.array_equal(d[0], c0)
    assert np.array_equal(d[1], sf.expand_seed_c1(SEED, m[:level], N))
    with pytest.raises(hecdna.InvalidArgument):
        hecdna.seal_ciphertext_save_seeded(c0, SCALE, m, SEED[:32], compr=compr)


@pytest.fixture(scope="module")
def env(hecdna, orc):
    m = orc.Oracle.create_coeff_modulus(N, BITS)
    o = orc.Oracle(N, m)
    ref = kr.Ref(o, kr.Streams(hecdna))
    s = ref.secret(SEED)
    return o, ref, s


def sym_bound(scale):
    return (kr.CBD_MAX + 0.5) * N / scale


def asym_bound(scale, q_last):
    return sym_bound(scale) + N * ((N + 1) / 2 + 1 + kr.CBD_MAX * (2 * N + 1) / q_last) / scale


def test_secret_key_is_ternary(env):
    o, ref, s = env
    coeff = [o.ntt_inv(j, s[j]) for j in range(o.K)]
    q = ref.q
    c0 = [int(x) - q[0] if int(x) > 1 else int(x) for x in coeff[0]]
    assert set(c0) == {-1, 0, 1}
    for j in range(1, o.K):
        assert [int(x) - q[j] if int(x) > 1 else int(x) for x in coeff[j]] == c0


def test_restated_ciphertexts_decrypt_under_the_oracle(orc, env):
    o, ref, s = env
    rng = np.random.default_rng(5)
    pk = ref.public(s, bytes(64))
    for level in (o.L, 2):
        v = rng.uniform(-1, 1, N // 2) + 1j * rng.uniform(-1, 1, N // 2)
        pt = o.encode(v, SCALE, level)
        sym = ref.encrypt_symmetric(s, pt, SEED, 3)
        got = o.decode(o.decrypt(s, orc.Ct(sym, SCALE)), SCALE)
        err = np.max(np.abs(got - v))
        print(f"symmetric level {level}: error {err:.3e} bound {sym_bound(SCALE):.3e}")
        assert err <= sym_bound(SCALE)
        asym = ref.encrypt(orc, pk, pt, SCALE, SEED, 1)
        assert asym.shape == (2, level, N)
        got = o.decode(o.decrypt(s, orc.Ct(asym, SCALE)), SCALE)
        err = np.max(np.abs(got - v))
        bound = asym_bound(SCALE, ref.q[level])
        print(f"asymmetric level {level}: error {err:.3e} bound {bound:.3e}")
        assert err <= bound


def test_restated_keys_switch_under_the_oracle(orc, env):
    """a rotation through the restated Galois key and a relinearized square through the restated relin key decode to
    the rotated / squared vector (a wrong sign, digit or key term is off by many orders)"""
    o, ref, s = env
    rng = np.random.default_rng(6)
    v = rng.uniform(-1, 1, N // 2)
    ct = orc.Ct(ref.encrypt_symmetric(s, o.encode(v, SCALE, o.L), SEED, 0), SCALE)
    elt = o.elt_from_step(1)
    gk = {elt: ref.galois(s, elt, SEED)}
    rot = o.decode(o.decrypt(s, o.rotate(ct, 1, gk)), SCALE)
    assert np.max(np.abs(rot - np.roll(v, -1))) < 1e-3
    rk = ref.relin(s, SEED)
    sq = o.rescale(o.relinearize(o.square(ct), rk))
    got = o.decode(o.decrypt(s, sq), sq.scale)
    assert np.max(np.abs(got - v * v)) < 1e-3
