"""The hoisted key MAC's divide-and-round epilogue (option "hmac_divround" / HEC_HMAC_DIVROUND): per sibling group of a
hoisted node k_hmacm accumulates the special-prime target first, the P-limb INTT and the fan-out give every child's
rounding limbs, and the data targets' k_hmacm launch divides-and-rounds its own accumulators straight into the
children's rotation buffers, so ACC's data limbs never reach memory.  Every case is compared word for word with the
oracle: one hoisted matvec per chunk size of the epilogue (P = 32, 64, 128, 256: 16, 8, 4 and 2 chunks per block) and
arithmetic class, sibling groups of every size, the zero corrections applied to the outputs, a level below the top, the
ct x pt walk, and the paths that keep the separate pass B."""
import os

import numpy as np
import pytest

from test_gpu_parity import Env, _ctpt_oracle, _env_with, _with_coeff_zeros

pytestmark = pytest.mark.gpu

# (log N, prime bits, diagonals, columns): P = 32 with a 50-bit integer q_0 and P and 36-bit FP64 targets; P = 64;
# P = 128; P = 256; and the bench's chain at N = 2^15 (P = 128, l = 10) with a partial FP64 batch group (3 columns)
SHAPES = {
    "n11": (11, [50, 36, 36, 50], 8, 2),
    "n12": (12, [60, 40, 40, 60], 8, 2),
    "n14": (14, [60, 40, 40, 60], 6, 2),
    "n16": (16, [60, 40, 60], 6, 2),
    "n15": (15, [60] + [40] * 9 + [60], 8, 3),
}
# steps 1 .. 7 by NAF: the root has the children 1, 2, -1, 4, -2 (a group of 5: slots of 2, 2 and 1), the node -1 the
# children 4 and 8, the nodes 1 and -2 a single child each (the per-rotation key switch)
STEPS = (1, -1, 2, -2, 4, -4, 8, -8)
_envs = {}
_refs = {}


def _env(orc, hecdna, name):
    """One context per shape for the module."""
    if name not in _envs:
        if name == "n11full":  # every default Galois key: the 40-diagonal walk and the ct x pt matvec
            _envs[name] = Env(orc, hecdna, 1 << 11, [50, 36, 36, 50], seed=41)
        else:
            logN, bits = SHAPES[name][:2]
            N = 1 << logN
            o = orc.Oracle(N, orc.Oracle.create_coeff_modulus(N, bits))
            _envs[name] = Env(orc, hecdna, N, bits, seed=500 + logN, elts=[o.elt_from_step(s) for s in STEPS])
    return _envs[name]


def _reference(e, key, n, ncol, seed, X=None, level=None):
    """Inputs and the oracle's outputs of one matvec, computed once per module and never modified."""
    if key not in _refs:
        A = [e.enc(seed=seed + j, level=level) for j in range(n)]
        X = X or [e.enc(seed=seed + 500 + i, level=level) for i in range(ncol)]
        _refs[key] = (A, X, e.o.matmul_diag_col(A, X, e.rk_h, e.gk_h, nthreads=8))
    return _refs[key]


def _check(e, ref):
    A, X, exp = ref
    got = e.ctx.matmul_diag_col([e.up(a) for a in A], [e.up(x) for x in X], e.rk, e.gk)
    assert len(got) == len(exp)
    for g, c in zip(got, exp):
        e.same(g, c)


def _with_options(e, opts, fn):
    """fn() under the given options, the engine's defaults restored afterwards."""
    defaults = {"hmac": 2, "hmac_divround": 1, "hmac_int": 1, "fan": 1}
    try:
        for k, v in opts.items():
            e.ctx.set_option(k, v)
        fn()
    finally:
        for k in opts:
            e.ctx.set_option(k, defaults[k])


@pytest.mark.parametrize("shape", list(SHAPES))
def test_hoisted_matvec_bitexact(orc, hecdna, shape):
    e = _env(orc, hecdna, shape)
    _, _, n, ncol = SHAPES[shape]
    _with_options(e, {"hmac_divround": 1}, lambda: _check(e, _reference(e, shape, n, ncol, 4000)))


def test_group_shapes(orc, hecdna):
    """n = 40 diagonals, 5 columns at N = 2^11: a root with more than one sibling group, groups of 1, 2 and 3 (the odd
    closer) below it, single-child nodes on the per-rotation path, and partial batch groups in both classes (5 is no
    multiple of 4 or 2)."""
    e = _env(orc, hecdna, "n11full")
    _with_options(e, {"hmac_divround": 1}, lambda: _check(e, _reference(e, "groups", 40, 5, 5000)))


@pytest.mark.parametrize("nzeros", [3, 40])
def test_zero_coefficients_correct_the_outputs(orc, hecdna, nzeros):
    """Zero digit coefficients that a child's automorphism negates: the correction is applied to the divided-and-rounded
    outputs (times P^-1); 40 zeros overflow the lists and the walk recomputes without hoisting."""
    e = _env(orc, hecdna, "n11full")
    rng = np.random.default_rng(nzeros)
    X = [_with_coeff_zeros(e, e.enc(seed=1100 + i), {0: rng.choice(e.N, nzeros, replace=False),
                                                     2: rng.choice(e.N, 2, replace=False)}) for i in range(2)]
    _with_options(e, {"hmac_divround": 1}, lambda: _check(e, _reference(e, ("zeros", nzeros), 12, 2, 6000, X=X)))


def test_level_below_the_top(orc, hecdna):
    """Inputs mod-switched down one level: l = 2 of L = 3, the 60-bit q_0 and one FP64 target."""
    e = _env(orc, hecdna, "n12")
    if "below" not in _refs:
        A = [e.o.mod_switch(e.enc(seed=7000 + j)) for j in range(8)]
        X = [e.o.mod_switch(e.enc(seed=7500 + i)) for i in range(2)]
        assert A[0].level == len(e.m) - 2
        _refs["below"] = (A, X, e.o.matmul_diag_col(A, X, e.rk_h, e.gk_h, nthreads=8))
    _with_options(e, {"hmac_divround": 1}, lambda: _check(e, _refs["below"]))


def test_ct_x_pt_walk(orc, hecdna):
    e = _env(orc, hecdna, "n11full")
    L = len(e.m) - 1
    pscale = 2.0**40
    P = [e.o.encode(e.rng.uniform(-1, 1, e.N // 2), pscale, L) for _ in range(12)]
    X = [e.enc(seed=700 + i) for i in range(2)]
    exp = _ctpt_oracle(e, P, pscale, X)

    def run():
        got = e.ctx.matmul_diagpt_col([e.ctx.plaintext(p, pscale) for p in P], [e.up(x) for x in X], e.gk)
        for g, c in zip(got, exp):
            e.same(g, c)
    _with_options(e, {"hmac_divround": 1}, run)


@pytest.mark.parametrize("opts", [{"hmac_divround": 0}, {"hmac_divround": 1, "hmac": 0}, {"hmac_divround": 1, "hmac": 1},
                                  {"hmac_divround": 1, "hmac_int": 0}, {"hmac_divround": 1, "fan": 0}],
                         ids=["off", "hmac0", "hmac1", "hmac_int0", "fan0"])
def test_fallbacks_stay_exact(orc, hecdna, opts):
    """The switch off, and the schedules the fold does not cover with the switch on (one hoisted MAC per child, one
    launch per sibling pair, the gathered-key 60-bit loop, no fan-out): the separate pass B, the same words."""
    e = _env(orc, hecdna, "n11")
    _, _, n, ncol = SHAPES["n11"]
    _with_options(e, opts, lambda: _check(e, _reference(e, "n11", n, ncol, 4000)))


def test_short_of_rotation_buffers(orc, hecdna):
    """One rotation buffer per depth cannot hold a sibling group: the unfolded path, child by child."""
    N = 1 << 11
    o = orc.Oracle(N, orc.Oracle.create_coeff_modulus(N, [50, 36, 36, 50]))
    e = _env_with(orc, hecdna, {"HEC_TENSOR_BUFS": "1", "HEC_HMAC_DIVROUND": "1"}, N, [50, 36, 36, 50], seed=45,
                  elts=[o.elt_from_step(s) for s in STEPS])
    _check(e, _reference(e, "bufs1", 8, 2, 7000))


@pytest.mark.parametrize("env", [{"HEC_HMAC_DIVROUND": "0"}, {"HEC_HMAC_DIVROUND": "1"},
                                 {"HEC_HMAC_DIVROUND": "1", "HEC_HOIST_MIN": "1"},
                                 {"HEC_HMAC_DIVROUND": "1", "HEC_HOIST_SCAN": "0"},
                                 {"HEC_HMAC_DIVROUND": "1", "HEC_TENSOR_DEFER": "1"}])
def test_keyswitch_variants_with_the_fold(orc, hecdna, env):
    """test_keyswitch_variants_bitexact's matvec (N = 2^12, every default key, 6 diagonals, 2 columns) under the new
    switch, alone and with the schedules around the hoisted MAC that it composes with."""
    e = _env_with(orc, hecdna, env, 1 << 12, [60, 40, 40, 60], seed=77)
    _check(e, _reference(e, "variants", 6, 2, 0))


def test_switch_out_of_range_is_rejected(orc, hecdna):
    N = 1 << 11
    m = orc.Oracle.create_coeff_modulus(N, [50, 36, 36, 50])
    old = os.environ.get("HEC_HMAC_DIVROUND")
    os.environ["HEC_HMAC_DIVROUND"] = "7"
    try:
        with pytest.raises(hecdna.InvalidArgument, match="HEC_HMAC_DIVROUND"):
            hecdna.Context(N, m)
    finally:
        if old is None:
            os.environ.pop("HEC_HMAC_DIVROUND", None)
        else:
            os.environ["HEC_HMAC_DIVROUND"] = old
    ctx = hecdna.Context(N, m)
    with pytest.raises(hecdna.InvalidArgument, match="hmac_divround"):
        ctx.set_option("hmac_divround", 7)
    with pytest.raises(hecdna.InvalidArgument, match="hmac_divround"):
        ctx.set_option("hmac_divround", -1)
