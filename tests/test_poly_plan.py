"""CPU: hec_math_poly_plan, the host planner of hec_math_poly (hecdna.math_poly_plan), against the restatement of the
Paterson-Stockmeyer schedule over the CPU oracle (tests/poly_ref.py) at N = 2^10 on two chains: the level, the scale
double (compared with ==), the block size and the counts of products and leaves; the first error of a bad call; and
the accuracy of the restated schedule itself against numpy.polyval.  The planner is the walk the device call runs
before any device work, and the device call is bit-exact to the restatement (tests/test_gpu_poly.py), so this fixes its
levels, scales, errors and accuracy without a GPU."""
import numpy as np
import pytest

import poly_ref

N = 1 << 10
CHAINS = {"s40": ([60] + [40] * 10 + [60], 10, 2.0**40), "s50": ([60] + [50] * 7 + [60], 8, 2.0**50)}


class Env:
    def __init__(self, orc, name):
        bits, self.level, self.scale = CHAINS[name]
        self.m = orc.Oracle.create_coeff_modulus(N, bits)
        self.o = orc.Oracle(N, self.m)
        self.sk = self.o.secret_key(7)
        self.rk = self.o.relin_key(self.sk, 8)
        self.xv = np.random.default_rng(3).uniform(-1, 1, N // 2)
        self.x = self.o.encrypt(self.sk, self.o.encode(self.xv, self.scale, self.level), self.scale, 11)
        self.cache = {}

    def ref(self, coeffs, bs=None):
        """the restated schedule's (result, bs, products, leaves), computed once"""
        key = (tuple(coeffs), bs)
        if key not in self.cache:
            p = poly_ref.Poly(self.o, self.rk, self.x, coeffs, bs)
            r = p.run()
            self.cache[key] = (r, p.bs, p.nprod, p.nleaf)
        return self.cache[key]


@pytest.fixture(scope="module")
def envs(orc):
    return {k: Env(orc, k) for k in CHAINS}


def dense(d, seed=0):
    c = np.random.default_rng(100 + d + seed).uniform(-1, 1, d + 1)
    c[d] = 0.5 if abs(c[d]) < 0.1 else c[d]
    return [float(v) for v in c]


def monomial(d):
    return [0.0] * d + [1.0]


def odd_only(d):
    return [v if j % 2 else 0.0 for j, v in enumerate(dense(d))]


# the issue's table: d, coefficients, default bs, output level from 10, products, leaves
TABLE = [(7, dense(7), 4, 6, 4, 2), (8, dense(8), 4, 6, 5, 2), (15, dense(15), 4, 5, 7, 4), (16, dense(16), 8, 5, 9, 2),
         (31, dense(31), 8, 4, 11, 4), (63, dense(63), 8, 3, 16, 8), (8, monomial(8), 4, 6, 3, 0),
         (16, monomial(16), 8, 5, 4, 0)]


def compare(hecdna, e, coeffs, bs=None):
    r, rbs, nprod, nleaf = e.ref(coeffs, bs)
    got = hecdna.math_poly_plan(e.m, coeffs, e.level, e.scale, bs)
    assert got == (r.level, r.scale, rbs, nprod, nleaf)  # the scale double with ==
    assert r.scale == e.scale  # the output keeps the input's scale, bitwise
    return got


@pytest.mark.parametrize("row", range(len(TABLE)))
def test_table(envs, hecdna, row):
    d, coeffs, bs, level, nprod, nleaf = TABLE[row]
    got = compare(hecdna, envs["s40"], coeffs)
    assert got[0] == level and got[2:] == (bs, nprod, nleaf)
    got = compare(hecdna, envs["s50"], coeffs)  # the same counts two levels lower on the short chain
    assert got[0] == level - 2 and got[2:] == (bs, nprod, nleaf)


@pytest.mark.parametrize("chain", list(CHAINS))
def test_small_and_sparse(envs, hecdna, chain):
    e = envs[chain]
    # levels used, by the schedule's own rule (need): d = 3 at bs = 2 is (c2 + c3 x) x^2 + (c0 + c1 x), a leaf and a
    # product; d = 4 at bs = 4 is c4 x^4 + a cubic leaf; d = 9 is (c8 + c9 x) x^8 + the degree-7 tree
    used = {1: 1, 2: 2, 3: 2, 4: 3, 9: 4}
    for d, lv in used.items():
        assert compare(hecdna, e, dense(d))[0] == e.level - lv
    compare(hecdna, e, odd_only(15))
    c9 = dense(9)
    compare(hecdna, e, [0.0] + c9[1:])
    compare(hecdna, e, c9 + [0.0, 0.0])  # trailing zeros are trimmed
    for bs in (2, 4, 8, 16):
        got = compare(hecdna, e, dense(15), bs)
        assert got[2] == bs
    assert compare(hecdna, e, dense(15), 16)[3:] == (14, 1)  # one 15-term leaf over the powers x^2 .. x^15


def test_first_errors(envs, hecdna):
    e = envs["s50"]

    def fails(msg, coeffs, bs=None):
        with pytest.raises(ValueError, match=msg):
            poly_ref.Poly(e.o, e.rk, e.x, coeffs, bs).run()
        with pytest.raises(hecdna.InvalidArgument, match=msg):
            hecdna.math_poly_plan(e.m, coeffs, e.level, e.scale, bs)
    fails("polynomial must not be constant", [0.5])
    fails("polynomial must not be constant", [0.5, 0.0, 0.0, 0.0])
    fails("coefficients must be finite", [0.5, float("nan"), 1.0])
    fails(r"bs must be a power of two in \[2, 16\]", dense(15), 3)
    fails(r"bs must be a power of two in \[2, 16\]", dense(15), 32)
    fails("end of modulus switching chain reached", dense(127))  # 8 levels from level 8
    assert compare(hecdna, e, dense(63))[0] == 1                 # 7 levels: the end of the chain exactly
    with pytest.raises(hecdna.InvalidArgument, match="degree must be below 2\\^16"):
        hecdna.math_poly_plan(e.m, [1.0] * 65537, e.level, e.scale)
    with pytest.raises(hecdna.InvalidArgument, match="not valid for encryption parameters"):
        hecdna.math_poly_plan(e.m, dense(3), 9, e.scale)


# max |decode(decrypt(result)) - numpy.polyval| of the restated schedule, measured on the CPU at the fixed seeds above
MEASURED = {("s40", 31): 1.212e-08, ("s40", 63): 2.126e-08, ("s50", 31): 1.175e-11, ("s50", 63): 2.826e-11}


@pytest.mark.parametrize("chain,d", list(MEASURED))
def test_restatement_accuracy(envs, chain, d):
    """Dense d = 31 and d = 63, |c| <= 1, |x| <= 1: the restated schedule decrypts to numpy.polyval within 16 x the
    error it gave when this test was written (MEASURED; the margin covers other chains' noise of the same order).
    Measured: 1.212e-08 (d = 31) and 2.126e-08 (d = 63) at scale 2^40, 1.175e-11 and 2.826e-11 at scale 2^50.  The GPU
    call needs no accuracy test of its own: it is bit-exact to this schedule."""
    e = envs[chain]
    coeffs = dense(d)
    r = e.ref(coeffs)[0]
    got = e.o.decode(e.o.decrypt(e.sk, r), r.scale).real
    err = float(np.max(np.abs(got - np.polyval(coeffs[::-1], e.xv))))
    print(chain, d, "max error", err)
    assert err <= 16 * MEASURED[chain, d]
