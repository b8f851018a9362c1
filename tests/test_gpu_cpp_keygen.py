"""he_demo selfcontained: the reference's batched_matmul_ckks flow (matrix_operations.cpp:1057-1156) through the C++
drop-in's KeyGenerator / Encryptor / Decryptor with no key or ciphertext from anywhere else.  With a fixed master seed
it reproduces the Python binding's doubles word for word (call k of the run uses the seed BLAKE2Xb(u64 k, key = master
seed): 0 the secret key, 1 the public key, 2 the relin key, 3 the Galois keys, 4 + i the encryption of column i), and
it matches the clear product.

Bounds.  eps_ref is measured: the same product on the oracle's own keys and (symmetric) ciphertexts.  The symmetric
run must stay within 8 eps_ref, as test_gpu_keygen.py's pipeline (noise of the same width from other streams).  The
demo's own form encrypts with the public key, whose fresh noise is wider; to first order the output error is
sum_j (d_i x_j + x_i d_j), so it is bounded by 2 dim max|x| asym + 8 eps_ref with asym the per-slot bound of a fresh
public-key encryption derived in test_gpu_keygen.py; a wrong key or sign is off by Q / scale, many orders more."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_cpp_facade import demo  # noqa: F401  (module fixture)

pytestmark = pytest.mark.gpu
N, BITS, SCALE, DIM = 1 << 13, [60, 40, 40, 60], 2.0 ** 40, 16
MASTER = bytes((7 * i + 1) & 0xFF for i in range(64))


def call_seed(hecdna, k):
    return hecdna.seal_blake2xb(struct.pack("<Q", k), MASTER, 64)


@pytest.fixture(scope="module")
def reference(orc):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    from make_golden import CFG1, cfg1_expected_plain, cfg1_inputs
    clear = cfg1_expected_plain(DIM, N // 2)
    o, m, sk, rk, gk, cts = cfg1_inputs(orc, dict(CFG1, n=DIM))
    outs = o.matmul_diag_col(cts, cts, rk, gk, nthreads=8)
    eps_ref = max(np.max(np.abs(o.decode(o.decrypt(sk, c), c.scale)[:DIM] - clear[i])) for i, c in enumerate(outs))
    return m, clear, eps_ref


@pytest.mark.parametrize("symmetric", [1, 0])
def test_selfcontained_matches_binding_and_clear_product(demo, hecdna, reference, tmp_path, symmetric):  # noqa: F811
    m, clear, eps_ref = reference
    data = np.array([[2 + DIM * c + r for r in range(DIM)] for c in range(DIM)], dtype=np.float64)
    inp, outp = str(tmp_path / "self.in"), str(tmp_path / "self.out")
    with open(inp, "wb") as f:
        f.write(b"HECSELF1" + struct.pack("<QQ", N, len(BITS)) + struct.pack("<%dQ" % len(BITS), *BITS))
        f.write(struct.pack("<dQ", SCALE, 1) + MASTER + struct.pack("<QQQ", symmetric, 1, DIM) + data.tobytes())
    subprocess.check_call([demo, "selfcontained", inp, outp])
    raw = open(outp, "rb").read()
    n, slots = struct.unpack("<QQ", raw[:16])
    assert (n, slots) == (DIM, N // 2)
    got = np.frombuffer(raw[16:], dtype=np.complex128).reshape(n, slots)

    ctx = hecdna.Context(N, m)
    sk = ctx.keygen_secret(call_seed(hecdna, 0))
    pk = ctx.keygen_public(sk, call_seed(hecdna, 1))
    rk = ctx.keygen_relin(sk, call_seed(hecdna, 2))
    gk = ctx.keygen_galois(sk, None, call_seed(hecdna, 3))
    vals = np.array([[data[c][r % DIM] for r in range(N // 2)] for c in range(DIM)], dtype=np.complex128)
    pts = ctx.encode(vals, SCALE)
    cts = [ctx.encrypt_symmetric(sk, p, call_seed(hecdna, 4 + i)) if symmetric
           else ctx.encrypt(pk, p, call_seed(hecdna, 4 + i)) for i, p in enumerate(pts)]
    exp = ctx.decrypt_decode(sk, ctx.matmul_diag_col(cts, cts, rk, gk))
    assert np.array_equal(got.view(np.float64), exp.view(np.float64))

    eps = max(np.max(np.abs(got[i][:DIM] - clear[i])) for i in range(DIM))
    bound = 8 * eps_ref
    if not symmetric:
        fresh = (21.5 * N + N * ((N + 1) / 2 + 1 + 21 * (2 * N + 1) / m[-1])) / SCALE
        bound += 2 * DIM * float(np.max(data)) * fresh
    print(f"selfcontained symmetric={symmetric}: eps_ref {eps_ref:.3e} demo {eps:.3e} bound {bound:.3e}")
    assert eps <= bound
