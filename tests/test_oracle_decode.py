"""CPU checks behind the GPU decoder's tests (tests/test_gpu_decode.py): the C ABI declares the client half, and the
tolerance those tests use is sound for the reference side alone: the oracle's decode stays within half of it of an
independent higher-precision evaluation of the same plaintext."""
import numpy as np
import pytest

U = 2.0 ** -53


def test_client_half_declared(hecdna):
    declared = hecdna.exported_symbols()
    for name in ("hec_secret_key_upload", "hec_secret_key_download", "hec_secret_key_destroy", "hec_decrypt",
                 "hec_decode", "hec_decrypt_decode"):
        assert name in declared, name
    for name in ("SecretKey",):
        assert hasattr(hecdna, name)
    for name in ("secret_key", "decrypt", "decode", "decrypt_decode"):
        assert hasattr(hecdna.Context, name)


@pytest.mark.parametrize("level", [1, 3])
def test_oracle_decode_within_half_the_gpu_tolerance(orc, level):
    """N = 2^10, scale 2^40, seeded complex v with |v_i| <= 1.  Independent evaluation: the coefficients composed
    exactly by CRT in Python integers (centred on Q), then slot i = sum_k c_k zeta^(3^i k) / scale, zeta = exp(i pi /
    N), as a direct O(N^2) sum in np.longdouble with the exponent reduced mod 2N as an integer."""
    N, scale = 1 << 10, 2.0 ** 40
    m = orc.Oracle.create_coeff_modulus(N, [50, 36, 36, 50])
    o = orc.Oracle(N, m)
    rng = np.random.default_rng(level)
    r, phi = np.sqrt(rng.uniform(0, 1, N // 2)), rng.uniform(0, 2 * np.pi, N // 2)
    v = r * np.exp(1j * phi)                                   # uniform in the unit disc
    pt = o.encode(v, scale, level)
    got = o.decode(pt, scale)
    co = [o.ntt_inv(i, pt[i]) for i in range(level)]
    Q = 1
    for q in m[:level]:
        Q *= q
    coeffs = []
    for k in range(N):
        acc = sum((int(co[i][k]) * pow(Q // m[i], -1, m[i]) % m[i]) * (Q // m[i]) for i in range(level)) % Q
        coeffs.append(acc - Q if acc > Q // 2 else acc)
    assert max(abs(c) for c in coeffs) < 2 ** 62                # exact as longdouble (64-bit mantissa)
    c = np.array(coeffs, dtype=np.longdouble) / np.longdouble(scale)
    k = np.arange(N, dtype=np.int64)
    pi = np.longdouble("3.14159265358979323846264338327950288")
    ref = np.empty(N // 2, dtype=np.clongdouble)
    pos = 1
    for i in range(N // 2):
        ang = ((pos * k) % (2 * N)).astype(np.longdouble) * (pi / np.longdouble(N))
        ref[i] = np.sum(c * np.cos(ang)) + 1j * np.sum(c * np.sin(ang))
        pos = pos * 3 % (2 * N)
    assert np.max(np.abs(ref - v)) < 1e-6                       # the independent sum does decode the plaintext
    err = float(np.linalg.norm((got.astype(np.clongdouble) - ref)))
    tol = (10 * np.log2(N) + 16) * U * np.sqrt(2 * np.sum(np.abs(got) ** 2))
    print(f"oracle decode level {level}: error {err:.3e} tol {tol:.3e} ratio {err / tol:.3f}")
    assert err <= tol / 2
