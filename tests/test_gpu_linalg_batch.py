"""he::linalg's element-wise products and slot sums as batched engine calls (hec_multiply_relin_rescale_many,
hec_sum_elems_many; Matrix::operator*=, BatchedMatrix::operator*= / square_inplace / sum_bvec_elems_inplace), word for
word against the CPU oracle's per-operation sequences (multiply / square -> relinearize -> rescale, and
Oracle.sum_elems), info() level and scale included: both arithmetic classes of primes, every branch of the
rotate-and-add schedule, entries at mixed levels and scales in one call, in place, under poison, in chunks, the fused
rotate-accumulate epilogue against the separate add, the fallback key-switch paths, the full-size kernel instances at
N = 2^15, the errors (with the outputs left untouched) and the C++ drop-in (bin/he_demo linalgb)."""
import numpy as np
import pytest

from test_gpu_cpp_facade import demo, run, same  # noqa: F401  (module fixture)

pytestmark = pytest.mark.gpu
STEPS = (1, 2, 4, 8)


def up(ctx, c):
    return ctx.ciphertext(c.data, c.scale)


def check(g, e):
    assert g.info() == (2, e.level, e.scale)
    assert np.array_equal(g.download(), e.data)


class Env:
    """One parameter set: ciphertexts, the keys (Galois keys for the steps 1, 2, 4, 8 only), the oracle's results
    computed once each"""

    def __init__(self, orc, hecdna, N, bits, level, scale, seed, n=3):
        self.N, self.level, self.scale = N, level, scale
        self.m = orc.Oracle.create_coeff_modulus(N, bits)
        self.o = orc.Oracle(N, self.m)
        self.sk = self.o.secret_key(seed)
        self.rk = self.o.relin_key(self.sk, seed + 1)
        self.gk = self.o.galois_keys(self.sk, [self.o.elt_from_step(s) for s in STEPS], seed + 2)
        self.rng = np.random.default_rng(seed + 3)
        self.xs = [self.enc(level, scale, seed + 10 + i) for i in range(n)]
        self.ys = [self.enc(level, scale, seed + 20 + i) for i in range(n)]
        self.ctx = hecdna.Context(N, self.m)
        self.grk = self.ctx.relin_key(self.rk)
        self.ggk = self.ctx.galois_keys(self.gk)
        self.cache = {}

    def enc(self, level, scale, seed):
        v = self.rng.uniform(-1, 1, self.N // 2)
        return self.o.encrypt(self.sk, self.o.encode(v, scale, level), scale, seed)

    def prod(self, a, b):
        key = ("p", id(a), id(b))
        if key not in self.cache:
            t = self.o.square(a) if b is a else self.o.multiply(a, b)
            self.cache[key] = (a, b, self.o.rescale(self.o.relinearize(t, self.rk)))
        return self.cache[key][2]

    def sum(self, a, dim):
        key = ("s", id(a), dim)
        if key not in self.cache:
            self.cache[key] = (a, self.o.sum_elems(a, dim, self.gk))
        return self.cache[key][1]


@pytest.fixture(scope="module")
def e11(orc, hecdna):
    return Env(orc, hecdna, 1 << 11, [60] + [40] * 4 + [60], 4, 2.0**40, 501)


@pytest.mark.parametrize("dim", [1, 2, 5, 6, 7, 8, 12])
def test_sums_fp64_primes(e11, dim):
    """case 1: B = 3; the dims cover the odd first rotation, `partial`, the inner loop and the trailing window
    rotation of the schedule; each result also equals the B = 1 call on that entry"""
    e = e11
    got = e.ctx.sum_elems([up(e.ctx, c) for c in e.xs], dim, e.ggk)
    assert len(got) == 3
    for g, c in zip(got, e.xs):
        check(g, e.sum(c, dim))
        one = e.ctx.sum_elems(up(e.ctx, c), dim, e.ggk)  # one ciphertext in, one out
        assert one.info() == g.info() and np.array_equal(one.download(), g.download())


def test_products_and_squares_fp64_primes(e11):
    e = e11
    a, b = [up(e.ctx, c) for c in e.xs], [up(e.ctx, c) for c in e.ys]
    got = e.ctx.multiply_relin_rescale(a, b, e.grk)
    assert len(got) == 3
    for g, x, y in zip(got, e.xs, e.ys):
        check(g, e.prod(x, y))
    for g, x in zip(e.ctx.multiply_relin_rescale(a, a, e.grk), e.xs):  # b is a: the squares
        check(g, e.prod(x, x))
    for x, y in zip(a, e.xs):  # the inputs were not written
        check(x, y)
    one = e.ctx.multiply_relin_rescale(a[0], b[0], e.grk)
    check(one, e.prod(e.xs[0], e.ys[0]))
    mixed = e.ctx.multiply_relin_rescale([a[0], a[1]], [a[0], b[1]], e.grk)  # a square and a product in one pass
    check(mixed[0], e.prod(e.xs[0], e.xs[0]))
    check(mixed[1], e.prod(e.xs[1], e.ys[1]))


def test_integer_primes(orc, hecdna):
    """case 2: every data prime >= 2^42 (the integer arithmetic)"""
    e = Env(orc, hecdna, 1 << 10, [60] + [50] * 3 + [60], 3, 2.0**50, 601, n=2)
    assert all(q >= 2**42 for q in e.m)
    for dim in (5, 8):
        for g, c in zip(e.ctx.sum_elems([up(e.ctx, c) for c in e.xs], dim, e.ggk), e.xs):
            check(g, e.sum(c, dim))
    check(e.ctx.multiply_relin_rescale([up(e.ctx, e.xs[0])], [up(e.ctx, e.ys[0])], e.grk)[0], e.prod(e.xs[0], e.ys[0]))


def test_mixed_levels_and_scales(e11):
    """case 3: levels 4, 4, 3 with scales 2^40, 2^39, 2^40 in one call; the order is kept, the scales are per entry"""
    e = e11
    xs = [e.xs[0], e.enc(4, 2.0**39, 541), e.enc(3, 2.0**40, 542)]
    ys = [e.ys[0], e.enc(4, 2.0**39, 543), e.enc(3, 2.0**40, 544)]
    got = e.ctx.multiply_relin_rescale([up(e.ctx, c) for c in xs], [up(e.ctx, c) for c in ys], e.grk)
    exp = [e.prod(x, y) for x, y in zip(xs, ys)]
    assert [x.level for x in exp] == [3, 3, 2] and len({x.scale for x in exp}) == 3
    for g, x in zip(got, exp):
        check(g, x)
    for g, c in zip(e.ctx.sum_elems([up(e.ctx, c) for c in xs], 6, e.ggk), xs):
        check(g, e.sum(c, 6))


def test_in_place(e11):
    """case 4"""
    e = e11
    a = [up(e.ctx, c) for c in e.xs]
    assert e.ctx.multiply_relin_rescale(a, [up(e.ctx, c) for c in e.ys], e.grk, out=a) is a
    for g, x, y in zip(a, e.xs, e.ys):
        check(g, e.prod(x, y))
    x = [up(e.ctx, c) for c in e.xs]
    assert e.ctx.sum_elems(x, 7, e.ggk, out=x) is x
    for g, c in zip(x, e.xs):
        check(g, e.sum(c, 7))
    sq = [up(e.ctx, c) for c in e.xs]
    e.ctx.multiply_relin_rescale(sq, sq, e.grk, out=sq)
    for g, c in zip(sq, e.xs):
        check(g, e.prod(c, c))


def test_poison(e11):
    """case 5: every workspace carve and fresh buffer filled with 0xFF first"""
    e = e11
    e.ctx.set_option("poison", 1)
    try:
        for g, c in zip(e.ctx.sum_elems([up(e.ctx, c) for c in e.xs], 7, e.ggk), e.xs):
            check(g, e.sum(c, 7))
        got = e.ctx.multiply_relin_rescale([up(e.ctx, c) for c in e.xs], [up(e.ctx, c) for c in e.ys], e.grk)
        for g, x, y in zip(got, e.xs, e.ys):
            check(g, e.prod(x, y))
    finally:
        e.ctx.set_option("poison", 0)


def test_chunks(e11):
    """case 6: B = 5 in passes of 2, 2 and 1 equals one pass, word for word"""
    e = e11
    xs, ys = e.xs + e.ys[:2], e.ys + e.xs[:2]
    res = {}
    for chunk in (2, 0):
        e.ctx.set_option("math_chunk", chunk)
        try:
            s = e.ctx.sum_elems([up(e.ctx, c) for c in xs], 6, e.ggk)
            p = e.ctx.multiply_relin_rescale([up(e.ctx, c) for c in xs], [up(e.ctx, c) for c in ys], e.grk)
            res[chunk] = [(g.info(), g.download()) for g in s + p]
        finally:
            e.ctx.set_option("math_chunk", 0)
    assert len(res[2]) == 10
    for (i2, d2), (i0, d0) in zip(res[2], res[0]):
        assert i2 == i0 and np.array_equal(d2, d0)
    for i in range(3):
        assert np.array_equal(res[2][i][1], e.sum(e.xs[i], 6).data)
        assert np.array_equal(res[2][5 + i][1], e.prod(e.xs[i], e.ys[i]).data)


def launches(ctx, prefix):
    return sum(ctx.profile_read(c)[1] for c in ctx.profile_classes() if c.startswith(prefix))


def test_rot_add_fused_against_separate(e11):
    """case 7: the accumulate steps with the add in the key switch's last stage ("rot_add" 1) and as a k_ew_add launch
    after it (0): the same words, the fused class launched under 1 only, k_ew_add fewer times under 1"""
    e = e11
    for dim in (7, 8):
        res, adds, fused = {}, {}, {}
        for mode in (1, 0):
            e.ctx.set_option("rot_add", mode)
            e.ctx.profile(2)
            try:
                res[mode] = [(g.info(), g.download()) for g in
                             e.ctx.sum_elems([up(e.ctx, c) for c in e.xs], dim, e.ggk)]
                adds[mode] = launches(e.ctx, "k:k_ew_add")
                fused[mode] = launches(e.ctx, "k:k_bmac/divround_add")
            finally:
                e.ctx.profile(0)
                e.ctx.set_option("rot_add", 1)
        for (i1, d1), (i0, d0), c in zip(res[1], res[0], e.xs):
            assert i1 == i0 and np.array_equal(d1, d0)
            assert np.array_equal(d1, e.sum(c, dim).data)
        # dim 7: accumulate steps 1 | 2, 1 and two `bvec += partial`; dim 8: accumulate steps 4, 2, 1 and no partial
        steps, partials = (3, 2) if dim == 7 else (3, 0)
        assert fused == {1: steps, 0: 0}
        assert adds == {1: partials, 0: partials + steps}
    with pytest.raises(Exception):
        e.ctx.set_option("rot_add", 2)


@pytest.mark.parametrize("knob", ["mac_divround", "fan"])
def test_fallback_paths(e11, knob):
    """case 8: "mac_divround" = 0 (the separate divide-and-round pass B), then also "fan" = 0: the add follows the key
    switch as a k_ew_add launch"""
    e = e11
    knobs = ["mac_divround"] if knob == "mac_divround" else ["mac_divround", "fan"]
    for k in knobs:
        e.ctx.set_option(k, 0)
    try:
        for dim in (7, 8):
            for g, c in zip(e.ctx.sum_elems([up(e.ctx, c) for c in e.xs], dim, e.ggk), e.xs):
                check(g, e.sum(c, dim))
        check(e.ctx.multiply_relin_rescale(up(e.ctx, e.xs[0]), up(e.ctx, e.ys[0]), e.grk), e.prod(e.xs[0], e.ys[0]))
    finally:
        for k in knobs:
            e.ctx.set_option(k, 1)


def test_fullsize(orc, hecdna):
    """case 9: N = 2^15 (the kernels' instances depend on N), {60, 40, 40, 60}, level 3, B = 2: a sum and a product
    under the defaults (the single-pass mod-down is opt-in, so this is the fused epilogue of k_bmac/divround at
    P = 128), the sum again with "moddown1" = 0 set explicitly, and with "moddown1" = 1 (k_moddown1's instances with
    the addend)"""
    e = Env(orc, hecdna, 1 << 15, [60, 40, 40, 60], 3, 2.0**40, 701, n=2)
    cts = lambda: [up(e.ctx, c) for c in e.xs]  # noqa: E731
    for g, c in zip(e.ctx.sum_elems(cts(), 8, e.ggk), e.xs):
        check(g, e.sum(c, 8))
    check(e.ctx.multiply_relin_rescale(cts()[0], up(e.ctx, e.ys[0]), e.grk), e.prod(e.xs[0], e.ys[0]))
    for md1 in (0, 1):
        e.ctx.set_option("moddown1", md1)
        e.ctx.profile(2)
        try:
            for g, c in zip(e.ctx.sum_elems(cts(), 8, e.ggk), e.xs):
                check(g, e.sum(c, 8))
            assert launches(e.ctx, "k:k_moddown1/moddown_add") == (3 if md1 else 0)
            assert launches(e.ctx, "k:k_bmac/divround_add") == (0 if md1 else 3)
        finally:
            e.ctx.profile(0)
            e.ctx.set_option("moddown1", 0)


def test_errors_write_nothing(e11, orc, hecdna):
    """case 10: every check runs before anything is written"""
    e = e11
    ctx = e.ctx
    olds = e.xs[:2]
    outs = [up(ctx, c) for c in olds]

    def untouched():
        for g, c in zip(outs, olds):
            check(g, c)

    def psum(msg, cts, dim, gk=None):
        with pytest.raises(hecdna.InvalidArgument, match=msg):
            ctx.sum_elems(cts, dim, gk or e.ggk, out=outs[:len(cts)])
        untouched()

    def pprod(msg, a, b, rk=None):
        with pytest.raises(hecdna.InvalidArgument, match=msg):
            ctx.multiply_relin_rescale(a, b, rk or e.grk, out=outs[:len(a)])
        untouched()

    g = [up(ctx, c) for c in e.xs]
    few = ctx.galois_keys({k: v for k, v in e.gk.items() if k in [e.o.elt_from_step(1), e.o.elt_from_step(2)]})
    with pytest.raises(orc.OracleError, match="Galois key not present"):
        e.o.sum_elems(e.xs[0], 8, {k: e.gk[k] for k in [e.o.elt_from_step(1), e.o.elt_from_step(2)]})
    psum("Galois key not present", g[:2], 8, gk=few)
    psum("Galois key not present", g[:2], 1, gk=ctx.galois_keys({}))  # the discarded rotation needs its key too
    big = ctx.multiply(up(ctx, e.xs[0]), g[1])
    assert big.info()[0] == 3
    psum("encrypted size must be 2", [g[0], big], 5)
    pprod("encrypted size must be 2", [g[0], big], [g[1], g[1]])
    low = ctx.mod_switch_to_next(up(ctx, e.xs[1]))
    pprod("encrypted1 and encrypted2 parameter mismatch", [g[0], g[1]], [g[1], low])
    low1 = e.enc(1, 2.0**20, 551)
    with pytest.raises(orc.OracleError, match="end of modulus switching chain reached"):
        e.o.rescale(e.o.relinearize(e.o.square(low1), e.rk))
    pprod("end of modulus switching chain reached", [g[0], up(ctx, low1)], [g[1], up(ctx, low1)])
    huge = orc.Ct(e.xs[0].data, 2.0**100)
    with pytest.raises(orc.OracleError, match="scale out of bounds"):
        e.o.multiply(huge, huge)
    pprod("scale out of bounds", [g[0], up(ctx, huge)], [g[1], up(ctx, huge)])
    ctx2 = hecdna.Context(e.N, e.m)
    pprod("relin_keys is not valid for encryption parameters", [g[0]], [g[1]], rk=ctx2.relin_key(e.rk))
    psum("galois_keys is not valid for encryption parameters", [g[0]], 5, gk=ctx2.galois_keys(e.gk))
    psum("dim must be positive", [g[0]], 0)
    # an output that is another entry's input could be overwritten before a later pass reads it
    with pytest.raises(hecdna.InvalidArgument, match="an output may alias only its own entry's inputs"):
        ctx.sum_elems([g[0], g[1]], 5, e.ggk, out=[g[1], g[0]])
    check(g[0], e.xs[0])
    check(g[1], e.xs[1])
    assert ctx.sum_elems([], 5, e.ggk) == []
    assert ctx.multiply_relin_rescale([], [], e.grk) == []


def test_demo_linalgb(demo, e11, tmp_path):
    """case 11: BatchedMatrix::operator*=, square, sum_bvec_elems and the element-wise Matrix::operator*= of
    cpp/include/he_linalg.h through bin/he_demo, three ciphertexts"""
    e = e11
    out = run(demo, "linalgb:5", tmp_path, e.N, e.m, e.xs, e.rk, e.gk)
    assert len(out) == 12
    exp = [e.prod(c, c) for c in e.xs] * 2 + [e.sum(c, 5) for c in e.xs] + [e.prod(c, c) for c in e.xs]
    for g, x in zip(out, exp):
        same(g, x)
