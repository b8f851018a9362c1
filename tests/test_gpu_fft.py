"""he::fft on the GPU (hec_fft / hec_bfft, reference src/core/he_fft.cpp:13-223), bit for bit against the
restatement of both schedules over the CPU oracle (tests/fft_ref.py), info() level and scale included: the FFT over
n ciphertexts and its inverse, the in-slot FFT on one and on several ciphertexts, the ends of the modulus chain, the
argument errors (with the outputs left untouched), the full-size kernels' paths at N = 2^15, and the C++ drop-in
(cpp/include/he_fft.h through bin/he_demo)."""
import numpy as np
import pytest

import fft_ref
from test_gpu_cpp_facade import demo, run, same  # noqa: F401  (module fixture)

pytestmark = pytest.mark.gpu


def up(ctx, c):
    return ctx.ciphertext(c.data, c.scale)


def check(g, e):
    assert g.info() == (2, e.level, e.scale)
    assert np.array_equal(g.download(), e.data)


def complex_cts(o, sk, count, level, scale, seed):
    rng = np.random.default_rng(seed)
    v = rng.uniform(-1, 1, (count, o.N // 2)) + 1j * rng.uniform(-1, 1, (count, o.N // 2))
    return [o.encrypt(sk, o.encode(v[i], scale, level), scale, seed + 1 + i) for i in range(count)]


def periodic_cts(o, sk, count, n, level, scale, seed):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        blk = rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)
        out.append(o.encrypt(sk, o.encode(np.tile(blk, o.N // 2 // n), scale, level), scale, seed + 1 + i))
    return out


@pytest.fixture(scope="module")
def e11(orc, hecdna):
    N = 1 << 11
    m = orc.Oracle.create_coeff_modulus(N, [60] + [40] * 5 + [60])
    o = orc.Oracle(N, m)
    sk = o.secret_key(101)
    gk = o.galois_keys(sk, [o.elt_from_step(s) for s in (1, 2, 4, 8, -1, -2, -4)], 102)
    cts = complex_cts(o, sk, 8, 6, 2.0**40, 103)
    ctx = hecdna.Context(N, m)
    return N, m, o, sk, gk, cts, ctx, ctx.galois_keys(gk)


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("n", [1, 2, 8])
def test_fft_bitexact(e11, hecdna, n, inverse):
    N, m, o, sk, gk, cts, ctx, ggk = e11
    exp = fft_ref.fft(o, hecdna, cts[:n], inverse)
    got = ctx.fft([up(ctx, c) for c in cts[:n]], inverse)
    assert len(got) == n
    for g, e in zip(got, exp):
        check(g, e)
    if n == 8:  # out[i] = in[i]
        io = [up(ctx, c) for c in cts[:n]]
        ctx.fft(io, inverse, out=io)
        for g, e in zip(io, exp):
            check(g, e)


def test_fft_chain_end(orc, hecdna):
    """N = 2^13, {60, 40, 40, 60}: n = 4 ends exactly at level 1; n = 8 and the inverse of n = 4 run off the chain"""
    N = 1 << 13
    m = orc.Oracle.create_coeff_modulus(N, [60, 40, 40, 60])
    o = orc.Oracle(N, m)
    sk = o.secret_key(111)
    cts = complex_cts(o, sk, 8, 3, 2.0**40, 112)
    ctx = hecdna.Context(N, m)
    exp = fft_ref.fft(o, hecdna, cts[:4])
    got = ctx.fft([up(ctx, c) for c in cts[:4]])
    for g, e in zip(got, exp):
        assert e.level == 1
        check(g, e)
    with pytest.raises(hecdna.InvalidArgument, match="end of modulus switching chain reached"):
        ctx.fft([up(ctx, c) for c in cts])
    outs = [up(ctx, c) for c in cts[4:]]
    with pytest.raises(hecdna.InvalidArgument, match="end of modulus switching chain reached"):
        ctx.fft([up(ctx, c) for c in cts[:4]], inverse=True, out=outs)
    for g, c in zip(outs, cts[4:]):  # untouched
        check(g, c)


@pytest.mark.parametrize("inverse", [False, True])
def test_bfft_bitexact(e11, hecdna, inverse):
    N, m, o, sk, gk, _, ctx, ggk = e11
    cts = periodic_cts(o, sk, 3, 8, 6, 2.0**40, 121)
    exp = [fft_ref.bfft(o, hecdna, c, 8, gk, inverse) for c in cts]
    one = ctx.bfft(up(ctx, cts[0]), 8, ggk, inverse)  # B = 1: the reference's call
    check(one, exp[0])
    many = ctx.bfft([up(ctx, c) for c in cts], 8, ggk, inverse)  # B = 3: every output its own B = 1 result
    for g, e, c in zip(many, exp, cts):
        check(g, e)
        assert np.array_equal(g.download(), ctx.bfft(up(ctx, c), 8, ggk, inverse).download())


def test_bfft_n16_and_missing_key(e11, hecdna, orc):
    """n = 16: rotations by 8, 4, 2, 1 and by -4, -2, -1.  Every rotation amount of the in-slot FFT is a power of two,
    whose NAF has one term, so SEAL's rotate_internal has no fallback for it: without the key for -2 the call is
    "Galois key not present", in the restatement and on the GPU alike, and nothing is written."""
    N, m, o, sk, gk, _, ctx, ggk = e11
    (ct,) = periodic_cts(o, sk, 1, 16, 6, 2.0**40, 131)
    check(ctx.bfft(up(ctx, ct), 16, ggk), fft_ref.bfft(o, hecdna, ct, 16, gk))
    part = {e: k for e, k in gk.items() if e != o.elt_from_step(-2)}
    with pytest.raises(orc.OracleError, match="Galois key not present"):
        fft_ref.bfft(o, hecdna, ct, 16, part)
    out = up(ctx, ct)
    with pytest.raises(hecdna.InvalidArgument, match="Galois key not present"):
        ctx.bfft([up(ctx, ct)], 16, ctx.galois_keys(part), out=[out])
    check(out, ct)


def test_bfft_all_slots(orc, hecdna):
    """n = slot_count = 512 at N = 2^10, {50, 36 x 10, 50}: steps = N / 4 (the largest default key) first; log2 512 =
    9 stages, from level 10 down to level 1, the end of the chain"""
    N = 1 << 10
    m = orc.Oracle.create_coeff_modulus(N, [50] + [36] * 10 + [50])
    o = orc.Oracle(N, m)
    sk = o.secret_key(141)
    gk = o.galois_keys(sk, o.default_galois_elts(), 142)
    (ct,) = periodic_cts(o, sk, 1, N // 2, 10, 2.0**36, 143)
    exp = fft_ref.bfft(o, hecdna, ct, N // 2, gk)
    assert exp.level == 1
    ctx = hecdna.Context(N, m)
    check(ctx.bfft(up(ctx, ct), N // 2, ctx.galois_keys(gk)), exp)


def test_fullsize(orc, hecdna):
    """N = 2^15, {60, 40 x 9, 60} (the kernels' paths depend on N): fft with n = 4, bfft with n = 4 and B = 2, keys
    for +-1 and +-2 only"""
    N = 1 << 15
    m = orc.Oracle.create_coeff_modulus(N, [60] + [40] * 9 + [60])
    o = orc.Oracle(N, m)
    sk = o.secret_key(151)
    gk = o.galois_keys(sk, [o.elt_from_step(s) for s in (1, 2, -1, -2)], 152)
    cts = periodic_cts(o, sk, 4, 4, 10, 2.0**40, 153)
    ctx = hecdna.Context(N, m)
    for g, e in zip(ctx.fft([up(ctx, c) for c in cts]), fft_ref.fft(o, hecdna, cts)):
        check(g, e)
    got = ctx.bfft([up(ctx, c) for c in cts[:2]], 4, ctx.galois_keys(gk))
    for g, c in zip(got, cts[:2]):
        check(g, fft_ref.bfft(o, hecdna, c, 4, gk))


def test_errors(e11, hecdna):
    N, m, o, sk, gk, cts, ctx, ggk = e11
    g = [up(ctx, c) for c in cts[:4]]
    outs = [up(ctx, c) for c in cts[4:8]]

    def untouched():
        for a, c in zip(outs, cts[4:8]):
            check(a, c)
    with pytest.raises(hecdna.InvalidArgument, match="power of two"):
        ctx.fft(g[:3], out=outs[:3])
    with pytest.raises(hecdna.InvalidArgument, match="power of two"):
        ctx.bfft(g[:1], 3, ggk, out=outs[:1])
    low = ctx.mod_switch_to_next(up(ctx, cts[1]))
    with pytest.raises(hecdna.InvalidArgument, match="parameter mismatch"):
        ctx.fft([g[0], low], out=outs[:2])
    with pytest.raises(hecdna.InvalidArgument, match="parameter mismatch"):
        ctx.bfft([g[0], low], 4, ggk, out=outs[:2])
    other = ctx.ciphertext(cts[1].data, cts[1].scale * (1 + 2.0**-52))  # SEAL-close, not bitwise equal
    with pytest.raises(hecdna.InvalidArgument, match="scale mismatch"):
        ctx.fft([g[0], other], out=outs[:2])
    with pytest.raises(hecdna.InvalidArgument, match="scale mismatch"):
        ctx.bfft([g[0], other], 4, ggk, out=outs[:2])
    big = ctx.multiply(up(ctx, cts[0]), g[1])  # size 3
    assert big.info()[0] == 3
    with pytest.raises(hecdna.InvalidArgument, match="encrypted size must be 2"):
        ctx.fft([g[0], big], out=outs[:2])
    with pytest.raises(hecdna.InvalidArgument, match="encrypted size must be 2"):
        ctx.bfft([big], 4, ggk, out=outs[:1])
    with pytest.raises(hecdna.InvalidArgument, match="at most slot_count"):
        ctx.bfft(g[:1], N, ggk, out=outs[:1])
    untouched()


@pytest.mark.parametrize("mode,n,inverse", [("fft:8", 8, False), ("fft:4:inv", 4, True), ("bfft:8", 8, False),
                                            ("bfft:8:inv", 8, True)])
def test_demo_he_fft(demo, e11, hecdna, tmp_path, mode, n, inverse):
    """cpp/include/he_fft.h through bin/he_demo: the drop-in's four functions equal the C-ABI results and the
    restatement"""
    N, m, o, sk, gk, cts, ctx, ggk = e11
    if mode.startswith("fft"):
        out = run(demo, mode, tmp_path, N, m, cts[:n], None, {})
        exp = fft_ref.fft(o, hecdna, cts[:n], inverse)
        cabi = ctx.fft([up(ctx, c) for c in cts[:n]], inverse)
    else:
        (ct,) = periodic_cts(o, sk, 1, n, 6, 2.0**40, 161)
        out = run(demo, mode, tmp_path, N, m, [ct], None, gk)
        exp = [fft_ref.bfft(o, hecdna, ct, n, gk, inverse)]
        cabi = [ctx.bfft(up(ctx, ct), n, ggk, inverse)]
    assert len(out) == len(exp)
    for g, e, c in zip(out, exp, cabi):
        same(g, e)
        assert np.array_equal(g[0], c.download()) and g[1] == c.info()[2]
