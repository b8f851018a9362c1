"""he_demo decrypt: the C++ drop-in's Decryptor::decrypt + CKKSEncoder::decode (cpp/include/hecdna/seal_compat.hpp)
on two ciphertexts gives the Python binding's doubles bit for bit (both go through hec_decrypt / hec_decode)."""
import struct
import subprocess

import numpy as np
import pytest

from test_gpu_cpp_facade import demo, write_input  # noqa: F401  (module fixture)

pytestmark = pytest.mark.gpu


def test_demo_decrypt_matches_binding(demo, orc, hecdna, tmp_path):  # noqa: F811
    N = 1 << 11
    m = orc.Oracle.create_coeff_modulus(N, [50, 36, 36, 50])
    o = orc.Oracle(N, m)
    sk = o.secret_key(17)
    rng = np.random.default_rng(17)
    vals = [rng.uniform(-1, 1, N // 2) + 1j * rng.uniform(-1, 1, N // 2) for _ in range(2)]
    cts = [o.encrypt(sk, o.encode(vals[0], 2.0 ** 40, 3), 2.0 ** 40, 1),
           o.multiply(o.encrypt(sk, o.encode(vals[1], 2.0 ** 30, 2), 2.0 ** 30, 2),
                      o.encrypt(sk, o.encode(vals[0], 2.0 ** 30, 2), 2.0 ** 30, 3))]   # size 3, another level
    inp, outp = str(tmp_path / "decrypt.in"), str(tmp_path / "decrypt.out")
    write_input(inp, N, m, cts, None, {})
    with open(inp, "ab") as f:
        f.write(struct.pack("<Q", 1))
        f.write(np.ascontiguousarray(sk, dtype=np.uint64).tobytes())
    subprocess.check_call([demo, "decrypt", inp, outp])
    raw = open(outp, "rb").read()
    n, slots = struct.unpack("<QQ", raw[:16])
    assert (n, slots) == (2, N // 2)
    got = np.frombuffer(raw[16:], dtype=np.complex128).reshape(n, slots)
    ctx = hecdna.Context(N, m)
    exp = ctx.decrypt_decode(ctx.secret_key(sk), [ctx.ciphertext(c.data, c.scale) for c in cts])
    assert np.array_equal(got.view(np.float64), exp.view(np.float64))
    # rounding + noise per fresh ciphertext (tests/test_gpu_decode.py): N (0.5 + 64 x 3.2) / scale; the product of
    # two such factors with |z| <= sqrt 2
    assert np.max(np.abs(got[0] - vals[0])) <= N * (0.5 + 64 * 3.2) / 2.0 ** 40
    eps = N * (0.5 + 64 * 3.2) / 2.0 ** 30
    assert np.max(np.abs(got[1] - vals[1] * vals[0])) <= 2 * np.sqrt(2) * eps + eps ** 2
