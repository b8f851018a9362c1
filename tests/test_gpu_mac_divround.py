"""The key MAC's divide-and-round epilogue (option "mac_divround" / HEC_MAC_DIVROUND): the per-rotation key switch
accumulates the special-prime target first and the data targets' k_bmac launch divides-and-rounds its own accumulators,
so ACC's data limbs never reach memory.  Every case is compared word for word with the oracle, at one chunk size per
instantiation of the fused kernel (P = 32, 64, 128, 256), both arithmetic classes, every caller of keyswitch()
(aliased and non-aliased Galois key switches, relinearisation in place) and levels below the top."""
import os

import numpy as np
import pytest

from test_gpu_parity import Env, _env_with, _with_coeff_zeros

pytestmark = pytest.mark.gpu

# (log N, prime bits): P = 32 with a 50-bit integer q_0 and P and 36-bit FP64 targets; P = 64; P = 128; P = 256; and
# the bench's chain at N = 2^15 (P = 128, l = 10)
SHAPES = {
    "n11": (11, [50, 36, 36, 50]),
    "n12": (12, [60, 40, 40, 60]),
    "n14": (14, [60, 40, 40, 60]),
    "n16": (16, [60, 40, 60]),
    "n15": (15, [60] + [40] * 9 + [60]),
}
_envs = {}


def _env(orc, hecdna, name):
    """One context per shape for the module, keys for the steps -1 and 4 (3 = 4 - 1 takes two NAF terms) and the
    conjugation only."""
    if name not in _envs:
        logN, bits = SHAPES[name]
        N = 1 << logN
        o = orc.Oracle(N, orc.Oracle.create_coeff_modulus(N, bits))
        elts = [o.elt_from_step(-1), o.elt_from_step(4), 2 * N - 1]
        _envs[name] = Env(orc, hecdna, N, bits, seed=300 + logN, elts=elts)
    return _envs[name]


def _keyswitch_cases(e):
    L = len(e.m) - 1
    levels = sorted({L, max(L - 1, 1), 1}, reverse=True)
    for level in levels:
        a = e.rand_ct(2, level)
        # one key (aliased: the permutation goes through scratch, the key switch runs with elt = 1)
        e.same(e.ctx.rotate_vector(e.up(a), 4, e.gk), e.o.rotate(a, 4, e.gk_h))
        # two NAF terms: the second key switch reads the first one's output
        e.same(e.ctx.rotate_vector(e.up(a), 3, e.gk), e.o.rotate(a, 3, e.gk_h))
        elt = e.o.elt_from_step(-1)
        e.same(e.ctx.apply_galois(e.up(a), elt, e.gk), e.o.apply_galois(a, elt, e.gk_h))
        conj = 2 * e.N - 1
        e.same(e.ctx.apply_galois(e.up(a), conj, e.gk), e.o.apply_galois(a, conj, e.gk_h))
        # multiply + relinearise: in_nk = 2, IN and OUT the same buffer, the target its third poly
        x, y = e.rand_ct(2, level, 2.0**12), e.rand_ct(2, level, 2.0**12)  # the product's scale fits one prime
        g = e.ctx.relinearize(e.ctx.multiply(e.up(x), e.up(y)), e.rk)
        e.same(g, e.o.relinearize(e.o.multiply(x, y), e.rk_h))


def _matvec(e, n, ncol, seed, X=None):
    A = [e.enc(seed=seed + j) for j in range(n)]
    X = X or [e.enc(seed=seed + 500 + i) for i in range(ncol)]
    exp = e.o.matmul_diag_col(A, X, e.rk_h, e.gk_h, nthreads=8)
    got = e.ctx.matmul_diag_col([e.up(a) for a in A], [e.up(x) for x in X], e.rk, e.gk)
    for g, c in zip(got, exp):
        e.same(g, c)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_per_rotation_keyswitch_bitexact(orc, hecdna, shape):
    e = _env(orc, hecdna, shape)
    e.ctx.set_option("mac_divround", 1)
    _keyswitch_cases(e)


def test_switch_off_keeps_separate_pass_b(orc, hecdna):
    """mac_divround = 0 is the separate divide-and-round pass B: the same words."""
    e = _env(orc, hecdna, "n11")
    e.ctx.set_option("mac_divround", 0)
    try:
        _keyswitch_cases(e)
    finally:
        e.ctx.set_option("mac_divround", 1)


@pytest.mark.parametrize("shape", ["n11", "n14"])
def test_non_aliased_galois_keyswitch_bitexact(orc, hecdna, shape):
    """The trie walk without hoisting key-switches every rotation into a fresh buffer: the Galois permutation is
    applied in the loads of the target tile and of the IN term (elt != 1), for a batch of 3 columns; the lazy
    relinearisation at the end runs the in_nk = 2 form on the batch."""
    logN, bits = SHAPES[shape]
    o = orc.Oracle(1 << logN, orc.Oracle.create_coeff_modulus(1 << logN, bits))
    elts = [o.elt_from_step(s) for s in (1, -1, 2, 4)]  # 3 = 4 - 1 and 5 = 4 + 1 by NAF
    e = Env(orc, hecdna, 1 << logN, bits, seed=61, elts=elts)
    e.ctx.set_option("mac_divround", 1)
    e.ctx.set_option("hoist", 0)
    _matvec(e, 6, 3, 4000)


def test_hoisted_walk_with_per_rotation_nodes(orc, hecdna):
    """n = 40 diagonals, 5 columns at N = 2^11: a root with more than one sibling group, groups of 1, 2 and 3 below
    it and partial batch groups; nodes with a single child take the per-rotation key switch."""
    e = Env(orc, hecdna, 1 << 11, [50, 36, 36, 50], seed=41)
    e.ctx.set_option("mac_divround", 1)
    _matvec(e, 40, 5, 5000)


@pytest.mark.parametrize("nzeros", [3, 40])
def test_hoisted_walk_zero_coefficients(orc, hecdna, nzeros):
    e = Env(orc, hecdna, 1 << 11, [50, 36, 36, 50], seed=43)
    e.ctx.set_option("mac_divround", 1)
    rng = np.random.default_rng(nzeros)
    X = [_with_coeff_zeros(e, e.enc(seed=1100 + i), {0: rng.choice(e.N, nzeros, replace=False),
                                                     2: rng.choice(e.N, 2, replace=False)}) for i in range(2)]
    _matvec(e, 12, 2, 6000, X=X)


def test_hoisted_walk_short_of_rotation_buffers(orc, hecdna):
    e = _env_with(orc, hecdna, {"HEC_TENSOR_BUFS": "1", "HEC_MAC_DIVROUND": "1"}, 1 << 11, [50, 36, 36, 50], seed=45)
    _matvec(e, 12, 2, 7000)


def test_hoisted_walk_60bit_class(orc, hecdna):
    e = Env(orc, hecdna, 1 << 12, [60, 40, 40, 60], seed=47)
    e.ctx.set_option("mac_divround", 1)
    _matvec(e, 6, 2, 8000)


def test_switch_out_of_range_is_rejected(orc, hecdna):
    N = 1 << 11
    m = orc.Oracle.create_coeff_modulus(N, [50, 36, 36, 50])
    old = os.environ.get("HEC_MAC_DIVROUND")
    os.environ["HEC_MAC_DIVROUND"] = "7"
    try:
        with pytest.raises(hecdna.InvalidArgument, match="HEC_MAC_DIVROUND"):
            hecdna.Context(N, m)
    finally:
        if old is None:
            os.environ.pop("HEC_MAC_DIVROUND", None)
        else:
            os.environ["HEC_MAC_DIVROUND"] = old
    ctx = hecdna.Context(N, m)
    with pytest.raises(hecdna.InvalidArgument, match="mac_divround"):
        ctx.set_option("mac_divround", 7)
