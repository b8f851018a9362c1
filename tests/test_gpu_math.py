"""he::math on the GPU as batched engine calls (hec_math_signed_inv / inv_sqrt_twice / sqrt / abs and
hec_drop_chain_levels; reference src/core/he_math.cpp:22-269, include/he_util.h:27-48), bit for bit against the
restatement of the same schedules over the CPU oracle (oracle/he_math_ref.py), info() level and scale included: both
arithmetic classes of primes (FP64 below 2^42, integer above), the ends of the modulus chain, in place, under poison,
in chunks, the errors (with the outputs left untouched), the full-size kernel instances at N = 2^15, and the C++
drop-in's vector overloads (cpp/include/he_math.h through bin/he_demo)."""
import os
import sys

import numpy as np
import pytest

from test_gpu_cpp_facade import demo, run, same  # noqa: F401  (module fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import he_math_ref as hm  # noqa: E402

REF = {"signed_inv": hm.signed_inv, "inv_sqrt_twice": hm.inv_sqrt_twice, "sqrt": hm.sqrt, "abs": hm.abs_}
A = {"signed_inv": 1.0, "inv_sqrt_twice": 0.7, "sqrt": 1.0, "abs": 1.0}


def up(ctx, c):
    return ctx.ciphertext(c.data, c.scale)


def check(g, e):
    assert g.info() == (2, e.level, e.scale)
    assert np.array_equal(g.download(), e.data)


class Env:
    """One parameter set: three ciphertexts of positive values, three of signed values, the oracle's results cached"""

    def __init__(self, orc, hecdna, N, bits, level, scale, seed):
        self.N, self.level, self.scale = N, level, scale
        self.m = orc.Oracle.create_coeff_modulus(N, bits)
        self.o = orc.Oracle(N, self.m)
        self.sk = self.o.secret_key(seed)
        self.rk = self.o.relin_key(self.sk, seed + 1)
        rng = np.random.default_rng(seed + 2)
        self.x = [rng.uniform(0.5, 1.5, N // 2) for _ in range(3)]
        self.s = [rng.uniform(0.3, 1.0, N // 2) * rng.choice([-1.0, 1.0], N // 2) for _ in range(3)]
        self.xs = [self.enc(v, level, scale, seed + 10 + i) for i, v in enumerate(self.x)]
        self.ss = [self.enc(v, level, scale, seed + 20 + i) for i, v in enumerate(self.s)]
        self.ctx = hecdna.Context(N, self.m)
        self.grk = self.ctx.relin_key(self.rk)
        self.cache = {}

    def enc(self, v, level, scale, seed):
        return self.o.encrypt(self.sk, self.o.encode(v, scale, level), scale, seed)

    def inputs(self, name):
        return self.ss if name == "abs" else self.xs

    def exp(self, name, i, iters, cts=None):
        """the restated schedule on input i of the function's own inputs (or of cts), computed once"""
        src = cts if cts is not None else self.inputs(name)
        key = (name, i, iters, "s" if src is self.ss else "x")
        if key not in self.cache:
            self.cache[key] = REF[name](self.o, self.rk, src[i], A[name], iters)
        return self.cache[key]

    def dec(self, ct):
        return self.o.decode(self.o.decrypt(self.sk, ct), ct.scale).real


@pytest.fixture(scope="module")
def e11(orc, hecdna):
    return Env(orc, hecdna, 1 << 11, [60] + [40] * 10 + [60], 10, 2.0**40, 201)


CASES = [("signed_inv", 1), ("signed_inv", 2), ("signed_inv", 3), ("inv_sqrt_twice", 1), ("inv_sqrt_twice", 2),
         ("inv_sqrt_twice", 3), ("sqrt", 1), ("sqrt", 3), ("abs", 1), ("abs", 3)]


@pytest.mark.parametrize("name,iters", CASES)
def test_bitexact_fp64_primes(e11, name, iters):
    """case 1: 40-bit data primes (the FP64 arithmetic), B = 1 and B = 3; iters = 3 takes the i > 1 branch of
    inv_sqrt_twice, where x drops two levels"""
    e = e11
    fn = getattr(e.ctx, name)
    cts = e.inputs(name)
    one = fn(up(e.ctx, cts[0]), A[name], iters, e.grk)  # B = 1: one ciphertext in, one out
    check(one, e.exp(name, 0, iters))
    many = fn([up(e.ctx, c) for c in cts], A[name], iters, e.grk)
    assert len(many) == 3
    for i, (g, c) in enumerate(zip(many, cts)):
        check(g, e.exp(name, i, iters))
        single = fn([up(e.ctx, c)], A[name], iters, e.grk)[0]
        assert single.info() == g.info() and np.array_equal(single.download(), g.download())


@pytest.mark.parametrize("name", ["signed_inv", "abs"])
def test_in_place(e11, name):
    e = e11
    io = [up(e.ctx, c) for c in e.inputs(name)]
    got = getattr(e.ctx, name)(io, A[name], 3, e.grk, out=io)
    assert got is io
    for i, g in enumerate(io):
        check(g, e.exp(name, i, 3))


def test_poison(e11):
    """every workspace carve and fresh buffer filled with 0xFF first: a stage that read words no stage wrote would
    differ from the oracle"""
    e = e11
    e.ctx.set_option("poison", 1)
    try:
        for name in ("signed_inv", "inv_sqrt_twice", "sqrt", "abs"):
            got = getattr(e.ctx, name)([up(e.ctx, c) for c in e.inputs(name)], A[name], 3, e.grk)
            for i, g in enumerate(got):
                check(g, e.exp(name, i, 3))
    finally:
        e.ctx.set_option("poison", 0)


def test_integer_primes_and_chain_end(orc, hecdna):
    """case 2: every data prime >= 2^42 (the integer arithmetic), N = 2^10, level 8, scale 2^50, iters 3, B = 2; abs
    ends at level 1.  The expected ciphertexts decode to the functions' values"""
    e = Env(orc, hecdna, 1 << 10, [60] + [50] * 7 + [60], 8, 2.0**50, 301)
    assert all(q >= 2**42 for q in e.m)
    levels = {"signed_inv": 4, "inv_sqrt_twice": 3, "sqrt": 2, "abs": 1}
    truth = {"signed_inv": lambda v: 1 / v, "inv_sqrt_twice": lambda v: 1 / np.sqrt(2 * v), "sqrt": np.sqrt,
             "abs": np.abs}
    bound = {"signed_inv": 2e-2, "inv_sqrt_twice": 5e-3, "sqrt": 5e-3, "abs": 0.15}
    for name in levels:
        cts = e.inputs(name)[:2]
        vals = (e.s if name == "abs" else e.x)[:2]
        got = getattr(e.ctx, name)([up(e.ctx, c) for c in cts], A[name], 3, e.grk)
        for i, g in enumerate(got):
            exp = e.exp(name, i, 3)
            assert exp.level == levels[name]
            err = np.max(np.abs(e.dec(exp) - truth[name](vals[i])))
            print(name, i, "decoded error", err)
            assert err < bound[name]
            check(g, exp)


def test_chain_end_fp64(e11):
    """case 3: abs with 4 iterations from level 10 ends at level 1 exactly"""
    e = e11
    exp = e.exp("abs", 0, 4)
    assert exp.level == 1
    check(e.ctx.abs(up(e.ctx, e.ss[0]), 1.0, 4, e.grk), exp)


def test_errors_write_nothing(e11, orc, hecdna):
    """case 4"""
    e = e11
    ctx = e.ctx
    olds = e.xs[:2]
    outs = [up(ctx, c) for c in olds]

    def fails(msg, name, cts, a, iters, rk=None, n=1):
        with pytest.raises(hecdna.InvalidArgument, match=msg):
            getattr(ctx, name)(cts, a, iters, rk or e.grk, out=outs[:n])
        for g, c in zip(outs, olds):
            check(g, c)
    low5 = e.enc(e.s[0], 5, 2.0**40, 231)
    with pytest.raises(orc.OracleError, match="scale out of bounds"):
        hm.abs_(e.o, e.rk, low5, 1.0, 2)
    fails("scale out of bounds", "abs", [up(ctx, low5)], 1.0, 2)
    low1 = e.enc(e.x[0], 1, 2.0**20, 232)
    with pytest.raises(orc.OracleError, match="end of modulus switching chain reached"):
        hm.signed_inv(e.o, e.rk, low1, 1.0, 1)
    fails("end of modulus switching chain reached", "signed_inv", [up(ctx, low1)], 1.0, 1)
    g = [up(ctx, c) for c in e.xs]
    low = ctx.mod_switch_to_next(up(ctx, e.xs[1]))
    fails("encrypted1 and encrypted2 parameter mismatch", "signed_inv", [g[0], low], 1.0, 2, n=2)
    other = ctx.ciphertext(e.xs[1].data, e.xs[1].scale * (1 + 2.0**-52))  # SEAL-close, not bitwise equal
    fails("scale mismatch", "inv_sqrt_twice", [g[0], other], 0.7, 2, n=2)
    big = ctx.multiply(up(ctx, e.xs[0]), g[1])
    assert big.info()[0] == 3
    fails("encrypted size must be 2", "sqrt", [g[0], big], 1.0, 2, n=2)
    fails("iter_num must be positive", "abs", [g[0]], 1.0, 0)
    ctx2 = hecdna.Context(e.N, e.m)
    fails("relin_keys is not valid for encryption parameters", "signed_inv", [g[0]], 1.0, 2, rk=ctx2.relin_key(e.rk))
    fails("encoded value is too large", "signed_inv", [g[0]], float("nan"), 2)
    with pytest.raises(hecdna.InvalidArgument):
        ctx.set_option("math_chunk", -1)


def test_chunks(e11):
    """case 5: B = 5 in passes of 2, 2 and 1 equals one pass, word for word"""
    e = e11
    cts = e.xs + e.ss[:2]
    res = {}
    for chunk in (2, 0):
        e.ctx.set_option("math_chunk", chunk)
        try:
            res[chunk] = [(g.info(), g.download()) for g in
                          e.ctx.signed_inv([up(e.ctx, c) for c in cts], 1.0, 3, e.grk)]
        finally:
            e.ctx.set_option("math_chunk", 0)
    assert len(res[2]) == 5
    for (i2, d2), (i0, d0) in zip(res[2], res[0]):
        assert i2 == i0 and np.array_equal(d2, d0)
    for i in range(3):
        assert np.array_equal(res[2][i][1], e.exp("signed_inv", i, 3).data)


def test_drop_chain_levels(e11):
    """case 6: B = 3, two levels, in place"""
    e = e11
    g = [up(e.ctx, c) for c in e.xs]
    assert e.ctx.drop_chain_levels(g, 2) is g
    for a, b in zip(g, hm.drop_chain_levels(e.o, e.xs, 2)):
        assert b.level == 8
        check(a, b)
    e.ctx.drop_chain_levels(g, 0)  # nothing to drop
    for a, b in zip(g, hm.drop_chain_levels(e.o, e.xs, 2)):
        check(a, b)


def test_fullsize(orc, hecdna):
    """case 7: N = 2^15 (the kernels' instances depend on N), {60, 40, 40, 40, 60}, level 4, B = 2: both end at
    level 1"""
    e = Env(orc, hecdna, 1 << 15, [60, 40, 40, 40, 60], 4, 2.0**40, 401)
    for name in ("signed_inv", "inv_sqrt_twice"):
        got = getattr(e.ctx, name)([up(e.ctx, c) for c in e.xs[:2]], A[name], 2, e.grk)
        for i, g in enumerate(got):
            exp = e.exp(name, i, 2)
            assert exp.level == 1
            check(g, exp)


def test_demo_mathb(demo, e11, tmp_path):
    """case 8: the vector overloads of cpp/include/he_math.h through bin/he_demo, three ciphertexts as one batch"""
    e = e11
    out = run(demo, "mathb:3", tmp_path, e.N, e.m, e.xs, e.rk, {})
    assert len(out) == 12
    k = 0
    for name in ("signed_inv", "inv_sqrt_twice", "sqrt", "abs"):
        for i in range(3):
            same(out[k], e.exp(name, i, 3, cts=e.xs))
            k += 1
