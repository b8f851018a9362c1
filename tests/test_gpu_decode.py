"""The client half on the GPU: hec_decrypt (bit-exact against the oracle's decrypt), hec_decode and hec_decrypt_decode
(against the oracle's decode within a derived floating-point tolerance: the decoder's order of operations is SEAL
4.1's as far as it can be restated without SEAL, so bit parity is not claimed).

Tolerance per output row, u = 2^-53, v the oracle's N/2 slots of that row:
    tol = (10 log2 N + 16) u sqrt(2 sum |v_i|^2)
Higham's FFT bound ||y^ - y||_2 <= eta log2 N ||y||_2 with eta ~ 5u per layer, counted twice because two
implementations are compared; + 16 covers the twist, the multiword-to-double sum and the division by scale;
||y||_2 over all N evaluation points is sqrt(2 sum |v_i|^2).  The 2-norm of the difference over the compared slots
must stay within tol (so must every single slot).  A wrong root, slot order or sign gives errors of order |v|.
The measured max(error / tol) per shape is recorded in DESIGN.md §4.9."""
import gc
from fractions import Fraction

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
BITS = {10: [50, 36, 36, 50], 11: [50, 36, 36, 50], 12: [50, 36, 36, 50], 13: [60, 40, 40, 60],
        16: [60] + [40] * 15 + [60]}


def tol_of(v, N):
    return (10 * np.log2(N) + 16) * U * np.sqrt(2 * np.sum(np.abs(v) ** 2))


class DEnv:
    """Oracle + GPU context + one secret key on both sides (no key-switching keys anywhere)."""

    def __init__(self, orc, hecdna, logN, bits=None):
        self.orc, self.hec = orc, hecdna
        self.N = 1 << logN
        self.m = orc.Oracle.create_coeff_modulus(self.N, bits or BITS[logN])
        self.L = len(self.m) - 1
        self.o = orc.Oracle(self.N, self.m)
        self.ctx = hecdna.Context(self.N, self.m)
        self.sk_h = self.o.secret_key(41 + logN)
        self.sk = self.ctx.secret_key(self.sk_h)
        self.rng = np.random.default_rng(logN)

    def vals(self, n=None):
        n = n or self.N // 2
        return self.rng.uniform(-1, 1, n) + 1j * self.rng.uniform(-1, 1, n)

    def enc(self, level, seed, scale=2.0 ** 40, vals=None):
        v = self.vals() if vals is None else vals
        return self.o.encrypt(self.sk_h, self.o.encode(v, scale, level), scale, seed)

    def up(self, ct):
        return self.ctx.ciphertext(ct.data, ct.scale)

    def close(self, got, ref_slots, what=""):
        """got: the first len(got) slots; ref_slots: the oracle's N/2 slots.  Returns error / tol."""
        err = np.linalg.norm(np.asarray(got) - ref_slots[: len(got)])
        tol = tol_of(ref_slots, self.N)
        print(f"decode N=2^{self.N.bit_length() - 1} {what}: error {err:.3e} tol {tol:.3e} ratio {err / tol:.3f}")
        assert err <= tol, (what, err, tol)
        return err / tol


_envs = {}


@pytest.fixture(scope="module")
def denv(orc, hecdna):
    def get(logN):
        if logN not in _envs:
            _envs[logN] = DEnv(orc, hecdna, logN)
        return _envs[logN]
    yield get
    _envs.clear()


# ------------------------------------------------------------------------------- decrypt ----
@pytest.mark.parametrize("poison", [0, 1])
def test_decrypt_bitexact(denv, poison):
    """Fresh size-2 ciphertexts at every level, a size-3 product, each alone and all in one mixed batch."""
    e = denv(11)
    e.ctx.set_option("poison", poison)
    try:
        cts = [e.enc(level, 10 + level) for level in (1, 2, 3)]
        cts.append(e.o.multiply(e.enc(3, 20), e.enc(3, 21)))
        cts.append(e.o.multiply(e.enc(2, 22), e.enc(2, 23)))
        assert [c.size for c in cts] == [2, 2, 2, 3, 3]
        exp = [e.o.decrypt(e.sk_h, c) for c in cts]
        for c, x in zip(cts, exp):
            pt = e.ctx.decrypt(e.sk, e.up(c))
            assert pt.info() == (c.level, c.scale)
            assert np.array_equal(pt.download(), x)
        order = [3, 0, 4, 2, 1]
        pts = e.ctx.decrypt(e.sk, [e.up(cts[i]) for i in order])
        for i, pt in zip(order, pts):
            assert pt.info() == (cts[i].level, cts[i].scale)
            assert np.array_equal(pt.download(), exp[i])
        assert np.array_equal(e.sk.download(), e.sk_h)
    finally:
        e.ctx.set_option("poison", 0)


# ------------------------------------------------------------------------------- decode -----
@pytest.mark.parametrize("logN", [10, 11, 12, 13, 16])
def test_decode_within_tolerance(denv, logN):
    """LDS chunk 2^9 / 2^10 / 2^11 with one register layer (N = 2^10 .. 2^12), two register layers (2^13), five
    register layers and the widest CRT (2^16 at level 16); a plaintext and a ciphertext each."""
    e = denv(logN)
    scale = 2.0 ** 40
    pt = e.o.encode(e.vals(), scale, e.L)
    ref = e.o.decode(pt, scale)
    got = e.ctx.decode(e.ctx.plaintext(pt, scale))
    assert got.shape == (e.N // 2,) and got.dtype == np.complex128
    e.close(got, ref, f"level {e.L} plaintext")
    ct = e.enc(e.L, 5)
    ref = e.o.decode(e.o.decrypt(e.sk_h, ct), scale)
    e.close(e.ctx.decrypt_decode(e.sk, e.up(ct)), ref, f"level {e.L} ciphertext")


def test_decode_batch_levels_nvalues_real(denv):
    """A batch of 3 at different levels (level 1: no composition) and scales; n_values 1, N/2 and a non-power of two;
    im = NULL."""
    e = denv(11)
    scales = [2.0 ** 30, 2.0 ** 40, 2.0 ** 25]
    pts = [e.o.encode(e.vals(), s, level) for s, level in zip(scales, (1, 3, 2))]
    refs = [e.o.decode(p, s) for p, s in zip(pts, scales)]
    gp = [e.ctx.plaintext(p, s) for p, s in zip(pts, scales)]
    full = e.ctx.decode(gp)
    assert full.shape == (3, e.N // 2)
    for i in range(3):
        e.close(full[i], refs[i], f"batch row {i}")
    for nv in (1, 37, e.N // 2):
        got = e.ctx.decode(gp, n_values=nv)
        assert got.shape == (3, nv)
        assert np.array_equal(got, full[:, :nv])      # the same slots, whatever the count
        real = e.ctx.decode(gp, n_values=nv, real=True)
        assert real.dtype == np.float64 and np.array_equal(real, full[:, :nv].real)
    one = e.ctx.decode(gp[0])                           # level 1 alone
    assert np.array_equal(one, full[0])


def test_crt_edge_cases_exact(denv):
    """Constant polynomials c (every word of limb i is c mod q_i) at level 3, scale 2^40: the transform of a constant
    adds exact zeros, so only the word sum and the scale multiply round: every slot is c / 2^40 within relative
    (level + 3) 2^-52."""
    e = denv(10)
    level, scale = 3, 2.0 ** 40
    Q = 1
    for q in e.m[:level]:
        Q *= q
    cs = [0, 1, -1, e.m[0], 2 ** 64, -2 ** 64, (Q - 1) // 2, -((Q - 1) // 2)]
    pts = [e.ctx.plaintext(np.stack([np.full(e.N, c % q, dtype=np.uint64) for q in e.m[:level]]), scale)
           for c in cs]
    got = e.ctx.decode(pts)
    for c, row in zip(cs, got):
        want = float(Fraction(c, 2 ** 40))
        assert np.all(row.imag == 0), c
        assert np.all(np.abs(row.real - want) <= (level + 3) * 2.0 ** -52 * abs(want)), (c, row[:2], want)


def test_round_trip_and_fused_path(denv):
    """decrypt_decode(encrypt(encode(v))) = v up to the encoder's rounding and the encryption noise, and the fused
    path gives decode(decrypt())'s doubles bit for bit.  Bound: the encoder rounds each of the N coefficients by at
    most 0.5, and a fresh symmetric encryption adds one noise coefficient each, a Gaussian of sigma 3.2 that SEAL
    clips at 6 sigma = 19.2 (64 x 3.2 is generous); a slot is a sum of the N coefficients times unit-modulus roots,
    over scale: |error| <= N 0.5 / scale + 64 x 3.2 N / scale."""
    e = denv(11)
    scale = 2.0 ** 40
    vs = [e.vals() for _ in range(3)]
    cts = [e.up(e.enc(level, 70 + level, scale, v)) for level, v in zip((3, 1, 2), vs)]
    cts.append(e.up(e.o.multiply(e.enc(3, 80, scale, vs[0]), e.enc(3, 81, scale, vs[1]))))
    fused = e.ctx.decrypt_decode(e.sk, cts)
    two = e.ctx.decode(e.ctx.decrypt(e.sk, cts))
    assert np.array_equal(fused, two)
    bound = e.N * 0.5 / scale + 64 * 3.2 * e.N / scale
    for v, row in zip(vs, fused):
        assert np.max(np.abs(row - v)) <= bound
    # the size-3 product at scale^2: (z0 + e0)(z1 + e1) with |z| <= sqrt 2 and |e| <= bound per factor
    assert np.max(np.abs(fused[3] - vs[0] * vs[1])) <= 2 * np.sqrt(2) * bound + bound ** 2
    nv = e.ctx.decrypt_decode(e.sk, cts, n_values=5, real=True)
    assert np.array_equal(nv, fused[:, :5].real)


# ------------------------------------------------------------------------------- errors -----
def test_errors_leave_outputs_unchanged(orc, hecdna, denv):
    import ctypes as C
    e = denv(11)
    L = hecdna.lib()
    other = hecdna.Context(e.N, e.m)
    good = e.up(e.enc(3, 90))
    gpt = e.ctx.decrypt(e.sk, good)
    sentinel = np.full((2, 8), 7.5)

    def decode_raw(ctx, pts, nv, re, im):
        dp = C.POINTER(C.c_double)
        arr = (C.c_void_p * len(pts))(*[p.h.value for p in pts])
        return L.hec_decode(ctx.h, arr, len(pts), nv, re.ctypes.data_as(dp), im.ctypes.data_as(dp))

    def dd_raw(sk, cts, nv, re, im):
        dp = C.POINTER(C.c_double)
        arr = (C.c_void_p * len(cts))(*[c.h.value for c in cts])
        return L.hec_decrypt_decode(e.ctx.h, sk.h, arr, len(cts), nv, re.ctypes.data_as(dp), im.ctypes.data_as(dp))

    def expect(rc, msg, re, im):
        assert rc == hecdna.HEC_EINVAL and msg in L.hec_last_error().decode(), (rc, L.hec_last_error())
        assert np.array_equal(re, sentinel) and np.array_equal(im, sentinel)

    size1 = e.ctx.ciphertext(e.enc(3, 91).data[:1], 2.0 ** 40)
    for bad in (e.ctx.ciphertext(), other.ciphertext(good.download(), 2.0 ** 40), size1):
        re, im = sentinel.copy(), sentinel.copy()
        expect(dd_raw(e.sk, [good, bad], 8, re, im), "encrypted is not valid for encryption parameters", re, im)
        out = e.ctx.plaintext(gpt.download(), 3.0)
        with pytest.raises(hecdna.InvalidArgument, match="encrypted is not valid for encryption parameters"):
            L_out = (C.c_void_p * 2)(out.h.value, out.h.value)
            hecdna._check(L.hec_decrypt(e.ctx.h, e.sk.h, (C.c_void_p * 2)(good.h.value, bad.h.value), 2, L_out))
        assert out.info() == (3, 3.0) and np.array_equal(out.download(), gpt.download())
    re, im = sentinel.copy(), sentinel.copy()
    expect(dd_raw(other.secret_key(e.sk_h), [good, good], 8, re, im),
           "secret key is not valid for encryption parameters", re, im)
    with pytest.raises(hecdna.InvalidArgument, match="secret key is not valid for encryption parameters"):
        e.ctx.decrypt(other.secret_key(e.sk_h), [good])
    with pytest.raises(hecdna.InvalidArgument, match="secret key is not valid for encryption parameters"):
        e.ctx.secret_key(e.sk_h[:2])
    # plain: an output handle of another context (decrypt), an empty or foreign input (decode)
    with pytest.raises(hecdna.InvalidArgument, match="plain is not valid for encryption parameters"):
        arr, foreign = (C.c_void_p * 1)(good.h.value), other.plaintext(None, 1.0)
        hecdna._check(L.hec_decrypt(e.ctx.h, e.sk.h, arr, 1, (C.c_void_p * 1)(foreign.h.value)))
    for bad in (e.ctx.plaintext(None, 1.0), other.plaintext(gpt.download(), 2.0 ** 40)):
        re, im = sentinel.copy(), sentinel.copy()
        expect(decode_raw(e.ctx, [gpt, bad], 8, re, im), "plain is not valid for encryption parameters", re, im)
    # scale out of bounds: the encoder's rule (level 3 has 50 + 36 + 36 = 122 bits)
    for s in (0.0, -1.0, 2.0 ** 122):
        re, im = sentinel.copy(), sentinel.copy()
        expect(decode_raw(e.ctx, [gpt, e.ctx.plaintext(gpt.download(), s)], 8, re, im), "scale out of bounds", re, im)
        re, im = sentinel.copy(), sentinel.copy()
        expect(dd_raw(e.sk, [good, e.ctx.ciphertext(good.download(), s)], 8, re, im), "scale out of bounds", re, im)
    assert decode_raw(e.ctx, [e.ctx.plaintext(gpt.download(), 2.0 ** 121)] * 2, 8, sentinel.copy(),
                      sentinel.copy()) == 0
    # n_values > N/2
    big = np.full((2, e.N // 2 + 1), 7.5)
    re, im = big.copy(), big.copy()
    rc = decode_raw(e.ctx, [gpt, gpt], e.N // 2 + 1, re, im)
    assert rc == hecdna.HEC_EINVAL and "values has invalid size" in L.hec_last_error().decode()
    assert np.array_equal(re, big) and np.array_equal(im, big)
    with pytest.raises(hecdna.InvalidArgument, match="values has invalid size"):
        e.ctx.decrypt_decode(e.sk, [good], n_values=e.N // 2 + 1)
    other.close()


# ------------------------------------------------------------------------------- lifetime ---
def test_secret_key_outlives_its_context(orc, hecdna):
    """A secret key destroyed after its context (as test_objects_outlive_their_context does for the other handles):
    its wipe and free touch the context only while it is alive; then a new context, possibly at the same address,
    works with a new key."""
    N = 1 << 10
    m = orc.Oracle.create_coeff_modulus(N, BITS[10])
    o = orc.Oracle(N, m)
    sk_h = o.secret_key(3)
    for _ in range(3):
        ctx = hecdna.Context(N, m)
        sk = ctx.secret_key(sk_h)
        before = ctx.secret_key(sk_h)
        del before                 # destroyed before its context
        gc.collect()
        ctx.close()
        del sk                     # ... and after it
        gc.collect()
    ctx = hecdna.Context(N, m)
    sk = ctx.secret_key(sk_h)
    ct = o.encrypt(sk_h, o.encode(np.arange(8.0), 2.0 ** 30, 2), 2.0 ** 30, 4)
    pt = ctx.decrypt(sk, ctx.ciphertext(ct.data, ct.scale))
    assert np.array_equal(pt.download(), o.decrypt(sk_h, ct))
