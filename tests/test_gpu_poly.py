"""he::math polynomial evaluation on the GPU (hec_math_poly, Context.poly): bit for bit, info() level and scale
included, against the Paterson-Stockmeyer schedule restated per operation over the CPU oracle (tests/poly_ref.py).
Both arithmetic classes of primes (FP64 below 2^42, integer above), every shape of the tree (leaves of 1 to 15 terms,
constant quotients, sparse polynomials, explicit block sizes), the end of the modulus chain, the FP64 sum of 15 terms on
boundary residues, in place, under poison, in chunks, the errors (with the outputs left untouched), the full-size
kernel instances at N = 2^15, and the C++ drop-in's overloads (cpp/include/he_math.h through bin/he_demo)."""
import numpy as np
import pytest

import poly_ref
import prime_classes as pc
from test_gpu_cpp_facade import demo, run, same  # noqa: F401  (module fixture)

pytestmark = pytest.mark.gpu


def up(ctx, c):
    return ctx.ciphertext(c.data, c.scale)


def check(g, e):
    assert g.info() == (2, e.level, e.scale)
    assert np.array_equal(g.download(), e.data)


def dense(d, seed=0):
    c = np.random.default_rng(500 + d + seed).uniform(-1, 1, d + 1)
    c[d] = 0.5 if abs(c[d]) < 0.1 else c[d]
    return [float(v) for v in c]


def monomial(d):
    return [0.0] * d + [1.0]


def odd_only(d):
    return [v if j % 2 else 0.0 for j, v in enumerate(dense(d))]


def demo_coeffs(d):
    """he_demo polyb:<d>'s polynomial"""
    c = [(((7 * j + 3) % 11) - 5) / 8.0 for j in range(d + 1)]
    if c[d] == 0.0:
        c[d] = 0.5
    return c


class Env:
    """One parameter set: five ciphertexts of values in [-1, 1], the restated schedule's results cached"""

    def __init__(self, orc, hecdna, N, bits, level, scale, seed, n=5):
        self.N, self.level, self.scale = N, level, scale
        self.m = orc.Oracle.create_coeff_modulus(N, bits)
        self.o = orc.Oracle(N, self.m)
        self.sk = self.o.secret_key(seed)
        self.rk = self.o.relin_key(self.sk, seed + 1)
        rng = np.random.default_rng(seed + 2)
        self.x = [rng.uniform(-1, 1, N // 2) for _ in range(n)]
        self.xs = [self.enc(v, level, scale, seed + 10 + i) for i, v in enumerate(self.x)]
        self.ctx = hecdna.Context(N, self.m)
        self.grk = self.ctx.relin_key(self.rk)
        self.cache = {}

    def enc(self, v, level, scale, seed):
        return self.o.encrypt(self.sk, self.o.encode(v, scale, level), scale, seed)

    def exp(self, i, coeffs, bs=None):
        key = (i, tuple(coeffs), bs)
        if key not in self.cache:
            self.cache[key] = poly_ref.poly(self.o, self.rk, self.xs[i], coeffs, bs)
        return self.cache[key]


@pytest.fixture(scope="module")
def e11(orc, hecdna):
    return Env(orc, hecdna, 1 << 11, [60] + [40] * 10 + [60], 10, 2.0**40, 601)


@pytest.mark.parametrize("d", [1, 2, 3, 7, 8, 15, 16, 31])
def test_bitexact_fp64_primes(e11, d):
    """40-bit data primes (the FP64 arithmetic), B = 1 and B = 3, every single equal to its batch entry"""
    e = e11
    c = dense(d)
    one = e.ctx.poly(up(e.ctx, e.xs[0]), c, e.grk)  # one ciphertext in, one out
    check(one, e.exp(0, c))
    many = e.ctx.poly([up(e.ctx, x) for x in e.xs[:3]], c, e.grk)
    assert len(many) == 3
    for i, g in enumerate(many):
        check(g, e.exp(i, c))
        single = e.ctx.poly([up(e.ctx, e.xs[i])], c, e.grk)[0]
        assert single.info() == g.info() and np.array_equal(single.download(), g.download())


SHAPES = {
    "x^8": (monomial(8), None),                  # constant-quotient nodes only: no leaf
    "x^16": (monomial(16), None),
    "odd15": (odd_only(15), None),
    "d9_c0_zero": ([0.0] + dense(9)[1:], None),
    "d9_c0": (dense(9), None),
    "x^8+c0": ([0.25] + monomial(8)[1:], None),  # the constant folded into the scalar stage
    "d15_bs2": (dense(15), 2),
    "d15_bs4": (dense(15), 4),
    "d15_bs8": (dense(15), 8),
    "d15_bs16": (dense(15), 16),                 # one 15-term leaf
    "d12_low_zero": ([0.0, 0.0, 0.0, 0.0] + dense(8), 4),          # an all-zero remainder leaf: no step for it
    "prod_node_const_rem": ([0.5, 0.0, 0.0, 0.0] + dense(3), 4),  # Eval(quo) x^4 + c0: add_plain after a product
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_tree_shapes(e11, name):
    e = e11
    c, bs = SHAPES[name]
    got = e.ctx.poly([up(e.ctx, x) for x in e.xs[:2]], c, e.grk, bs=bs)
    for i, g in enumerate(got):
        check(g, e.exp(i, c, bs))


def test_lower_input_level(e11):
    """an input at level 6 of the 10: every slot is read and written below the width it is carved at"""
    e = e11
    x6 = e.enc(e.x[0], 6, 2.0**40, 650)
    c = dense(15)
    exp = poly_ref.poly(e.o, e.rk, x6, c)
    assert exp.level == 1
    check(e.ctx.poly(up(e.ctx, x6), c, e.grk), exp)


def test_integer_primes_and_chain_end(orc, hecdna):
    """every data prime >= 2^42 (the integer arithmetic), N = 2^10, level 8, scale 2^50: dense d = 63 ends at level 1;
    d = 127 is the end of the chain, with the outputs untouched"""
    e = Env(orc, hecdna, 1 << 10, [60] + [50] * 7 + [60], 8, 2.0**50, 701, n=2)
    assert all(q >= 2**42 for q in e.m)
    c = dense(63)
    outs = e.ctx.poly([up(e.ctx, x) for x in e.xs], c, e.grk)
    for i, g in enumerate(outs):
        assert e.exp(i, c).level == 1
        check(g, e.exp(i, c))
    with pytest.raises(hecdna.InvalidArgument, match="end of modulus switching chain reached"):
        e.ctx.poly([up(e.ctx, x) for x in e.xs], dense(127), e.grk, out=outs)
    for i, g in enumerate(outs):
        check(g, e.exp(i, c))


@pytest.fixture(scope="module")
def edge(orc, hecdna):
    """41-, 42- and 43-bit data primes: the FP64 class at its widest beside the integer class"""
    N = 1 << 10
    m = orc.Oracle.create_coeff_modulus(N, [60, 41, 42, 43, 42, 41, 43, 42, 60])
    o = orc.Oracle(N, m)
    sk = o.secret_key(801)
    rk = o.relin_key(sk, 802)
    ctx = hecdna.Context(N, m)
    return N, m, o, rk, ctx, ctx.relin_key(rk)


@pytest.mark.parametrize("level", [7, 8])
@pytest.mark.parametrize("names", [("qm1", "qm1"), ("half_hi", "alt"), ("half_lo", "last")])
def test_fp64_sum_bound(orc, edge, level, names):
    """d = 15 at bs = 16, one leaf of 15 terms, on synthetic inputs of boundary residues (every word q_i - 1, the halves
    where rint ties, single extreme words).  From level 8 the leaf reads four limbs and rescales by the 43-bit prime
    (integer sums, FP64 sums in pass B at the 41- and 42-bit primes); from level 7 it rescales by the 42-bit prime (the
    FP64 last-limb sum).  The oracle evaluates any data, so the expectation is the restated schedule again"""
    N, m, o, rk, ctx, grk = edge
    assert [int(q).bit_length() for q in m[1:4]] == [41, 42, 43]
    x = pc.pattern_ct(orc, m, 2, level, N, list(names), 2.0**40)
    c = dense(15)
    exp = poly_ref.poly(o, rk, x, c, 16)
    assert exp.level == level - 5
    check(ctx.poly(up(ctx, x), c, grk, bs=16), exp)


def test_in_place(e11):
    e = e11
    c = dense(15)
    io = [up(e.ctx, x) for x in e.xs[:3]]
    got = e.ctx.poly(io, c, e.grk, out=io)
    assert got is io
    for i, g in enumerate(io):
        check(g, e.exp(i, c))


def test_poison(e11):
    """every workspace carve and fresh buffer filled with 0xFF first: a stage that read words no stage wrote would
    differ from the oracle"""
    e = e11
    e.ctx.set_option("poison", 1)
    try:
        for c, bs in ((dense(15), None), (dense(15), 16), (monomial(8), None)):
            got = e.ctx.poly([up(e.ctx, x) for x in e.xs[:2]], c, e.grk, bs=bs)
            for i, g in enumerate(got):
                check(g, e.exp(i, c, bs))
    finally:
        e.ctx.set_option("poison", 0)


def test_chunks(e11):
    """B = 5 in passes of 2, 2 and 1 equals one pass, word for word"""
    e = e11
    c = dense(15)
    res = {}
    for chunk in (2, 0):
        e.ctx.set_option("math_chunk", chunk)
        try:
            res[chunk] = [(g.info(), g.download()) for g in e.ctx.poly([up(e.ctx, x) for x in e.xs], c, e.grk)]
        finally:
            e.ctx.set_option("math_chunk", 0)
    assert len(res[2]) == 5
    for (i2, d2), (i0, d0) in zip(res[2], res[0]):
        assert i2 == i0 and np.array_equal(d2, d0)
    for i in range(3):
        assert np.array_equal(res[2][i][1], e.exp(i, c).data)


def test_fullsize(orc, hecdna):
    """N = 2^15 (the kernels' instances depend on N), {60, 40 x 4, 60}, level 5, d = 7, B = 2: ends at level 1"""
    e = Env(orc, hecdna, 1 << 15, [60, 40, 40, 40, 40, 60], 5, 2.0**40, 901, n=2)
    c = dense(7)
    got = e.ctx.poly([up(e.ctx, x) for x in e.xs], c, e.grk)
    for i, g in enumerate(got):
        assert e.exp(i, c).level == 1
        check(g, e.exp(i, c))


def test_errors_write_nothing(e11, hecdna):
    e = e11
    ctx = e.ctx
    olds = e.xs[:2]
    outs = [up(ctx, c) for c in olds]
    g = [up(ctx, c) for c in e.xs[:2]]

    def fails(msg, cts, coeffs, rk=None, bs=None):
        with pytest.raises(hecdna.InvalidArgument, match=msg):
            ctx.poly(cts, coeffs, rk or e.grk, bs=bs, out=outs[:len(cts)])
        for o, c in zip(outs, olds):
            check(o, c)
    big = ctx.multiply(up(ctx, e.xs[0]), g[1])
    assert big.info()[0] == 3
    fails("encrypted size must be 2", [g[0], big], dense(7))
    other = ctx.ciphertext(e.xs[1].data, e.xs[1].scale * (1 + 2.0**-52))  # SEAL-close, not bitwise equal
    fails("scale mismatch", [g[0], other], dense(7))
    ctx2 = hecdna.Context(e.N, e.m)
    fails("relin_keys is not valid for encryption parameters", [g[0]], dense(7), rk=ctx2.relin_key(e.rk))
    fails(r"bs must be a power of two in \[2, 16\]", [g[0]], dense(7), bs=3)
    fails(r"bs must be a power of two in \[2, 16\]", [g[0]], dense(7), bs=32)
    fails("polynomial must not be constant", [g[0]], [0.5])
    fails("polynomial must not be constant", [g[0]], [0.5, 0.0, 0.0])
    fails("coefficients must be finite", [g[0]], [0.5, float("inf")])


def test_demo_polyb(demo, e11, tmp_path):
    """the overloads of cpp/include/he_math.h through bin/he_demo: one ciphertext, then three as one batch"""
    e = e11
    c = demo_coeffs(15)
    out = run(demo, "polyb:15", tmp_path, e.N, e.m, e.xs[:3], e.rk, {})
    assert len(out) == 4
    same(out[0], e.exp(0, c))
    got = e.ctx.poly([up(e.ctx, x) for x in e.xs[:3]], c, e.grk)
    for i in range(3):
        same(out[1 + i], e.exp(i, c))
        assert np.array_equal(out[1 + i][0], got[i].download())
