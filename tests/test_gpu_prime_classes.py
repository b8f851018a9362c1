"""The edges of the two arithmetic classes of primes (FP64 for q < 2^42, integer otherwise) and the exact-FP64 bounds at
their limits, bit for bit against the CPU oracle: chains with 41-, 42- and 43-bit primes, FP64-class digits far wider
than FP64-class targets, a special prime in the FP64 class, the residues 0, 1, q - 1, (q - 1) / 2 and (q + 1) / 2 as
inputs, and sums of half-residues that reach the bounds the kernels state (tests/prime_classes.py has the chains and
the inputs; tests/test_prime_classes.py checks on the CPU that they are what this module takes them for).  Every
assertion is equality with the oracle: there are no tolerances except the decoder's own (test_gpu_decode.py)."""
import contextlib

import numpy as np
import pytest

import fft_ref
import prime_classes as pc
import test_gpu_bsgs as tb
import test_gpu_decode as td
import test_gpu_fft as tf
import test_gpu_keygen as tk
import test_gpu_linalg_batch as tl
import test_gpu_math as tm
import test_gpu_parity as tp
from test_gpu_parity import Env

pytestmark = pytest.mark.gpu
N11 = pc.N11
OP_CHAINS = ("TOP", "EDGE", "INT", "ALLFP")
# the alternative key-switch schedules of test_keyswitch_variants_bitexact, then the ones it does not list
SWITCHES = next(mk.args[1] for mk in tp.test_keyswitch_variants_bitexact.pytestmark if mk.name == "parametrize")
MORE_SWITCHES = [{"HEC_MODDOWN1": "1"}, {"HEC_NTTB_SHFL": "2", "HEC_NTTB_SHFL_DR": "1"}, {"HEC_MAC_DIVROUND": "0"},
                 {"HEC_MAC_DIVROUND": "1"}, {"HEC_HMAC_DIVROUND": "0"}, {"HEC_HMAC_DIVROUND": "1"}]
# pairs of boundary patterns per poly: (q - 1)^2, (q - 1) x 1, the two halves against each other and themselves, ...
PAIRS = [(("qm1", "qm1"), ("qm1", "qm1")), (("qm1", "one"), ("one", "qm1")),
         (("half_lo", "half_hi"), ("half_hi", "half_lo")), (("half_hi", "half_hi"), ("half_hi", "qm1")),
         (("alt", "qm1"), ("qm1", "alt")), (("first", "last"), ("last", "qm1")),
         (("zero", "qm1"), ("one", "zero")), (("half_lo", "half_lo"), ("half_lo", "half_lo"))]

@pytest.fixture(scope="module")
def envs(orc, hecdna):
    """one Env per chain of the per-operation tests (default Galois keys, N = 2^11)"""
    made = {chain: Env(orc, hecdna, N11, pc.CHAINS[chain], seed=len(chain) + 40) for chain in OP_CHAINS}
    return made.__getitem__


def ct_pairs(e, chain, kind, level, size_a=2, size_b=2):
    """rand: one pair of uniform ciphertexts; boundary: one pair per entry of PAIRS (a third poly repeats the first)"""
    sc = pc.SCALE[chain]
    if kind == "rand":
        return [(e.rand_ct(size_a, level, sc), e.rand_ct(size_b, level, sc))]
    return [(pc.pattern_ct(e.orc, e.m, size_a, level, e.N, a, sc), pc.pattern_ct(e.orc, e.m, size_b, level, e.N, b, sc))
            for a, b in PAIRS]


# =============================================================================== 1. NTT ====
def _ntt_case(orc, hecdna, logN, mode=0):
    N = 1 << logN
    m = orc.Oracle.create_coeff_modulus(N, pc.NTT_BITS)
    o = orc.Oracle(N, m)
    ctx = hecdna.Context(N, m)
    if mode:
        ctx.set_option("nttb_shfl", mode)
    K = len(m)
    per_limb = [pc.transform_inputs(o, i, N) for i in range(K)]
    names = list(per_limb[0])
    if logN == 16:  # fewer patterns at the largest size, every width kept
        names = ["qm1", "half_hi", "alt", "last", "inv_of_qm1", "inv_of_alt", "fwd_of_one", "fwd_of_alt"]
    rng = np.random.default_rng(logN)
    polys = [np.stack([per_limb[i][n] for i in range(K)]) for n in names]
    polys.append(np.stack([rng.integers(0, q, N, dtype=np.uint64) for q in m]))
    a = np.stack(polys)
    exp_f = np.stack([np.stack([o.ntt_fwd(i, p[i]) for i in range(K)]) for p in a])
    exp_i = np.stack([np.stack([o.ntt_inv(i, p[i]) for i in range(K)]) for p in a])
    return m, o, ctx, names, a, exp_f, exp_i


def _ntt_check(ctx, a, exp_f, exp_i):
    assert np.array_equal(ctx.ntt(a), exp_f)
    assert np.array_equal(ctx.ntt(a, inverse=True), exp_i)
    assert np.array_equal(ctx.ntt(exp_f, inverse=True), a)
    sub = np.ascontiguousarray(a[:, 1:5])  # a limb offset: the 42-, 41-, 43- and 30-bit limbs alone
    assert np.array_equal(ctx.ntt(sub, limb0=1), exp_f[:, 1:5])
    assert np.array_equal(ctx.ntt(sub, limb0=1, inverse=True), exp_i[:, 1:5])


@pytest.mark.parametrize("logN", [10, 13, 16])
def test_ntt_boundary_patterns(orc, hecdna, logN):
    """ctx.ntt forward, inverse and at a limb offset over {60, 42, 41, 43, 30, 60} on the boundary words, on their
    preimages (the output is then exactly 0, 1, q - 1, the halves) and on a random polynomial; 16 stages at 2^16 only"""
    m, o, ctx, names, a, exp_f, exp_i = _ntt_case(orc, hecdna, logN)
    k = names.index("inv_of_qm1")
    assert np.all(exp_f[k] == np.array(m, dtype=np.uint64)[:, None] - 1)  # the preimages do land on q - 1
    _ntt_check(ctx, a, exp_f, exp_i)


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("logN", [13, 14, 15, 16])
def test_ntt_boundary_patterns_shuffle_pass_b(orc, hecdna, logN, mode):
    """The same under "nttb_shfl" 1 and 2.  k_nttb_shfl is the forward pass B of 128-point columns, which run_ntt2 has
    at logN = 14 and 15 only (every width of the chain, both store orders); at 13 and 16 the LDS pass runs and the
    option must change nothing"""
    m, o, ctx, names, a, exp_f, exp_i = _ntt_case(orc, hecdna, logN, mode)
    _ntt_check(ctx, a, exp_f, exp_i)


@pytest.mark.parametrize("logN", [10, 13])
def test_dyadic_and_device_pipeline_on_patterns(orc, hecdna, logN):
    """dyadic_multiply and the device pipeline (ntt_device, dyadic_device, inverse ntt_device) on pattern x pattern:
    (q - 1)^2, (q - 1) (q + 1) / 2, ((q + 1) / 2)^2, ... per limb"""
    N = 1 << logN
    m = orc.Oracle.create_coeff_modulus(N, pc.NTT_BITS)
    o = orc.Oracle(N, m)
    ctx = hecdna.Context(N, m)
    K = len(m)
    words = [pc.boundary_words(q, N) for q in m]
    left = ["qm1", "qm1", "half_hi", "half_hi", "half_lo", "alt", "first", "one"]
    right = ["qm1", "half_hi", "half_hi", "half_lo", "half_lo", "qm1", "last", "qm1"]
    a = np.stack([np.stack([words[i][n] for i in range(K)]) for n in left])
    b = np.stack([np.stack([words[i][n] for i in range(K)]) for n in right])
    q = np.array(m, dtype=object).reshape(1, K, 1)
    assert np.array_equal(ctx.dyadic_multiply(a, b), (a.astype(object) * b.astype(object) % q).astype(np.uint64))
    sa, sb = np.ascontiguousarray(a[:, 1:5]), np.ascontiguousarray(b[:, 1:5])
    assert np.array_equal(ctx.dyadic_multiply(sa, sb, limb0=1),
                          (sa.astype(object) * sb.astype(object) % q[:, 1:5]).astype(np.uint64))
    bufs = [hecdna.DeviceBuffer(ctx, a.nbytes) for _ in range(3)]
    bufs[0].upload(a)
    bufs[1].upload(b)
    ctx.ntt_device(bufs[0], K, len(a))
    ctx.dyadic_device(bufs[0], bufs[1], bufs[2], K, len(a))
    ctx.ntt_device(bufs[2], K, len(a), inverse=True)
    ctx.synchronize()
    exp_f = np.stack([np.stack([o.ntt_fwd(i, p[i]) for i in range(K)]) for p in a])
    assert np.array_equal(bufs[0].download(a.shape), exp_f)
    prod = (exp_f.astype(object) * b.astype(object) % q).astype(np.uint64)
    exp = np.stack([np.stack([o.ntt_inv(i, p[i]) for i in range(K)]) for p in prod])
    assert np.array_equal(bufs[2].download(a.shape), exp)


# =============================================================================== 2. per-operation parity ====
@pytest.mark.parametrize("kind", ["rand", "boundary"])
@pytest.mark.parametrize("chain", OP_CHAINS)
def test_add_sub_negate(envs, chain, kind):
    e = envs(chain)
    for a, b in ct_pairs(e, chain, kind, 3):
        e.same(e.ctx.add(e.up(a), e.up(b)), e.o.add(a, b))
        e.same(e.ctx.sub(e.up(a), e.up(b)), e.o.sub(a, b))
        e.same(e.ctx.negate(e.up(a)), e.o.negate(a))
    for a, c3 in ct_pairs(e, chain, kind, 3, 2, 3):  # size 2 + 3: the extra poly copied, negated
        e.same(e.ctx.add(e.up(a), e.up(c3)), e.o.add(a, c3))
        e.same(e.ctx.sub(e.up(a), e.up(c3)), e.o.sub(a, c3))
        e.same(e.ctx.add(e.up(c3), e.up(a)), e.o.add(c3, a))


@pytest.mark.parametrize("kind", ["rand", "boundary"])
@pytest.mark.parametrize("chain", OP_CHAINS)
def test_multiply_square(envs, chain, kind):
    e = envs(chain)
    for a, b in ct_pairs(e, chain, kind, 3):
        e.same(e.ctx.multiply(e.up(a), e.up(b)), e.o.multiply(a, b))
        e.same(e.ctx.square(e.up(a)), e.o.square(a))
        e.same(e.ctx.square(e.up(b)), e.o.square(b))
    for c3, a in ct_pairs(e, chain, kind, 3, 3, 2)[:3]:
        e.same(e.ctx.multiply(e.up(c3), e.up(a)), e.o.multiply(c3, a))


@pytest.mark.parametrize("kind", ["rand", "boundary"])
@pytest.mark.parametrize("chain", OP_CHAINS)
def test_plain_ops(envs, chain, kind):
    e = envs(chain)
    sc = pc.SCALE[chain]
    for a, b in ct_pairs(e, chain, kind, 3):
        pt = b.data[1]
        p = e.ctx.plaintext(pt, sc)
        e.same(e.ctx.multiply_plain(e.up(a), p), e.o.multiply_plain(a, pt, sc))
        e.same(e.ctx.add_plain(e.up(a), p), e.o.add_plain(a, pt, sc))
        e.same(e.ctx.sub_plain(e.up(a), p), e.o.sub_plain(a, pt, sc))


@pytest.mark.parametrize("kind", ["rand", "boundary"])
@pytest.mark.parametrize("chain", OP_CHAINS)
def test_relinearize_rescale_modswitch(envs, chain, kind):
    """levels 3 and 2: the special prime and q_2, then q_1, as the divisor of the divide-and-round tail"""
    e = envs(chain)
    for level in (3, 2):
        for c3, c2 in ct_pairs(e, chain, kind, level, 3, 2):
            e.same(e.ctx.relinearize(e.up(c3), e.rk), e.o.relinearize(c3, e.rk_h))
            e.same(e.ctx.rescale_to_next(e.up(c3)), e.o.rescale(c3))
            e.same(e.ctx.rescale_to_next(e.up(c2)), e.o.rescale(c2))
            e.same(e.ctx.mod_switch_to_next(e.up(c2)), e.o.mod_switch(c2))


@pytest.mark.parametrize("kind", ["rand", "boundary"])
@pytest.mark.parametrize("chain", OP_CHAINS)
def test_rotate_and_conjugate(envs, chain, kind):
    e = envs(chain)
    for a, b in ct_pairs(e, chain, kind, 3)[:5]:
        for steps in (1, 3, -1, 511):
            e.same(e.ctx.rotate_vector(e.up(a), steps, e.gk), e.o.rotate(a, steps, e.gk_h))
        elt = 2 * e.N - 1
        e.same(e.ctx.apply_galois(e.up(b), elt, e.gk), e.o.apply_galois(b, elt, e.gk_h))
    low = ct_pairs(e, chain, kind, 2)[0][0]  # a lower level: fewer digits, the same special prime
    e.same(e.ctx.rotate_vector(e.up(low), 3, e.gk), e.o.rotate(low, 3, e.gk_h))


# =============================================================================== 3. key-switch schedules ====
@pytest.fixture(scope="module")
def matvec_ref(orc, hecdna):
    """per chain: an Env (the host keys every switched context below uploads), A (6 diagonals), X (2 columns) and the
    oracle's product"""
    ref = {}
    for chain in ("EDGE", "ALLFP"):
        e = Env(orc, hecdna, N11, pc.CHAINS[chain], seed=77)
        sc = pc.SCALE[chain]
        A = [e.enc(scale=sc, seed=j) for j in range(6)]
        X = [e.enc(scale=sc, seed=40 + i) for i in range(2)]
        ref[chain] = (e, A, X, e.o.matmul_diag_col(A, X, e.rk_h, e.gk_h))
    return ref


@pytest.mark.parametrize("env", SWITCHES + MORE_SWITCHES, ids=lambda d: ",".join(f"{k[4:]}={v}" for k, v in d.items()))
@pytest.mark.parametrize("chain", ["EDGE", "ALLFP"])
def test_keyswitch_schedules(hecdna, matvec_ref, chain, env):
    """matmul_diag_col, n = 6, p = 2, under every alternative key-switch schedule: a context created under the
    switches (they are read at creation) with the reference Env's keys.  The single-pass mod-down has its instances at
    N = 2^15 only and the shuffle pass B at 2^14 and 2^15: they run again below"""
    e, A, X, exp = matvec_ref[chain]
    with pytest.MonkeyPatch.context() as mp:
        for k, v in env.items():
            mp.setenv(k, v)
        ctx = hecdna.Context(e.N, e.m)
    up = lambda c: ctx.ciphertext(c.data, c.scale)  # noqa: E731
    got = ctx.matmul_diag_col([up(a) for a in A], [up(x) for x in X], ctx.relin_key(e.rk_h), ctx.galois_keys(e.gk_h))
    for g, c in zip(got, exp):
        e.same(g, c)


@pytest.mark.parametrize("chain", ["EDGE", "ALLFP"])
def test_keyswitch_full_size_moddown1_and_shuffle(orc, hecdna, chain):
    """N = 2^15, where k_moddown1 and the wave-shuffle pass B (also for the divide-and-round) have their instances:
    rotations and the n = 6, p = 2 matvec under the defaults, under "moddown1" and under "nttb_shfl" 2 with
    "nttb_shfl_dr"; keys for the steps 1, 2, 4 and -1 only"""
    N = 1 << 15
    o = orc.Oracle(N, orc.Oracle.create_coeff_modulus(N, pc.CHAINS[chain]))
    e = Env(orc, hecdna, N, pc.CHAINS[chain], seed=15, elts=[o.elt_from_step(s) for s in (1, 2, 4, -1)])
    sc = pc.SCALE[chain]
    A = [e.enc(scale=sc, seed=j) for j in range(6)]
    X = [e.enc(scale=sc, seed=40 + i) for i in range(2)]
    exp = e.o.matmul_diag_col(A, X, e.rk_h, e.gk_h, nthreads=8)
    rot = [e.o.rotate(X[0], s, e.gk_h) for s in (1, 3)]
    for opts in ({}, {"moddown1": 1}, {"nttb_shfl": 2, "nttb_shfl_dr": 1}):
        for k, v in opts.items():
            e.ctx.set_option(k, v)
        try:
            for s, r in zip((1, 3), rot):
                e.same(e.ctx.rotate_vector(e.up(X[0]), s, e.gk), r)
            got = e.ctx.matmul_diag_col([e.up(a) for a in A], [e.up(x) for x in X], e.rk, e.gk)
            for g, c in zip(got, exp):
                e.same(g, c)
        finally:
            for k in opts:
                e.ctx.set_option(k, 0)


@pytest.mark.parametrize("nzeros", [3, 40])
def test_hoisted_zero_coefficients_top(orc, hecdna, nzeros):
    """the hoisted mod-up's correction for zero digit coefficients at 42-bit digits (limb 1) and at q_0"""
    e = Env(orc, hecdna, N11, pc.CHAINS["TOP"])
    rng = np.random.default_rng(nzeros)
    X = [tp._with_coeff_zeros(e, e.enc(seed=1100 + i), {0: rng.choice(e.N, 2, replace=False),
                                                        1: rng.choice(e.N, nzeros, replace=False),
                                                        2: rng.choice(e.N, 2, replace=False)}) for i in range(2)]
    A = [e.enc(seed=1200 + j) for j in range(12)]
    exp = e.o.matmul_diag_col(A, X, e.rk_h, e.gk_h)
    got = e.ctx.matmul_diag_col([e.up(a) for a in A], [e.up(x) for x in X], e.rk, e.gk)
    for g, c in zip(got, exp):
        e.same(g, c)


# =============================================================================== 4. sums at their bound ====
@pytest.fixture(scope="module")
def top(envs):
    return envs("TOP")


@contextlib.contextmanager
def _defer(e, mode):
    """tensor_defer 1 flushes every product on its own; the default defers up to TB_MAX = 12"""
    if mode:
        e.ctx.set_option("tensor_defer", 1)
    try:
        yield
    finally:
        e.ctx.set_option("tensor_defer", 12)


@pytest.fixture(scope="module", params=["half_lo", "half_hi"])
def bsgs_ref(request, top):
    """(plaintext words, columns, the oracle's composition): 1,023 rotations per column, once per plaintext word"""
    e, sc, n = top, pc.SCALE["TOP"], 1024
    pt = pc.pattern_poly(e.m, 3, e.N, request.param)
    X = [pc.invariant_ct(e.orc, e.m, 3, e.N, sc), e.rand_ct(2, 3, sc)]
    return pt, X, tb.bsgs_oracle(e, [pt] * n, X, n, e.gk_h, sc)


@pytest.mark.parametrize("defer1", [0, 1])
def test_bsgs_inner_sum_at_its_bound(top, bsgs_ref, defer1):
    """k_bsgs_inner's stated worst case through the public API: n = bs = 1024 plaintext diagonals whose every word is
    (q - 1) / 2 (or (q + 1) / 2) times the invariant ciphertext: 1024 products of +-(q - 1) / 2 in one sum, 2^51 at
    the 42-bit primes (test_prime_classes.py asserts that from the oracle's integers).  A second, random column shares
    the batch"""
    e = top
    sc, n = pc.SCALE["TOP"], 1024
    pt, X, exp = bsgs_ref
    assert np.all(exp[0].data[1] == 0) and len(set(exp[0].data[0, 1].tolist())) == 1  # one word everywhere, c1 = 0
    gp = e.ctx.plaintext(pt, sc)
    with _defer(e, defer1):
        got = e.ctx.matmul_diagpt_col_bsgs([gp] * n, [e.up(x) for x in X], e.gk, bs=n)
    for g, c in zip(got, exp):
        e.same(g, c)


@pytest.mark.parametrize("defer1", [0, 1])
@pytest.mark.parametrize("half", ["half_lo", "half_hi"])
def test_ctpt_sum_n13(top, half, defer1):
    """matmul_diagpt_col, n = 13: one past the deferred-product flush at TB_MAX = 12"""
    e = top
    sc = pc.SCALE["TOP"]
    pt = pc.pattern_poly(e.m, 3, e.N, half)
    X = [pc.invariant_ct(e.orc, e.m, 3, e.N, sc), e.rand_ct(2, 3, sc)]
    exp = tp._ctpt_oracle(e, [pt] * 13, sc, X)
    gp = e.ctx.plaintext(pt, sc)
    with _defer(e, defer1):
        got = e.ctx.matmul_diagpt_col([gp] * 13, [e.up(x) for x in X], e.gk)
    for g, c in zip(got, exp):
        e.same(g, c)


@pytest.mark.parametrize("defer1", [0, 1])
@pytest.mark.parametrize("n", [12, 13])
@pytest.mark.parametrize("half", ["half_lo", "half_hi", "qm1"])
def test_tensor_sum_at_tb_max(top, half, n, defer1):
    """matmul_diag_col with n = TB_MAX = 12 and one past the flush: constant-word diagonals in both polys, so the
    deferred tensor sums (k_tensor_multi2: |sum| <= 1.6 q T) add T terms of one sign against the invariant column"""
    e = top
    sc = pc.SCALE["TOP"]
    d = pc.pattern_ct(e.orc, e.m, 2, 3, e.N, [half, half], sc)
    X = [pc.invariant_ct(e.orc, e.m, 3, e.N, sc), e.rand_ct(2, 3, sc),
         pc.pattern_ct(e.orc, e.m, 2, 3, e.N, ["half_hi", "half_lo"], sc)]
    exp = e.o.matmul_diag_col([d] * n, X, e.rk_h, e.gk_h)
    gd = e.up(d)
    with _defer(e, defer1):
        got = e.ctx.matmul_diag_col([gd] * n, [e.up(x) for x in X], e.rk, e.gk)
    for g, c in zip(got, exp):
        e.same(g, c)


# =============================================================================== 5. layers with their own kernels ====
@pytest.fixture(scope="module")
def math_long(orc, hecdna):
    return tm.Env(orc, hecdna, N11, pc.CHAINS["LONG"], 11, pc.SCALE["LONG"], 801)


@pytest.mark.parametrize("name", ["sqrt", "abs"])
def test_he_math_long(math_long, name):
    """he::math at iters = 3, B = 2, on eleven digits of which ten are 42-bit, scale 2^42"""
    e = math_long
    cts = e.inputs(name)[:2]
    got = getattr(e.ctx, name)([tm.up(e.ctx, c) for c in cts], tm.A[name], 3, e.grk)
    for i, g in enumerate(got):
        tm.check(g, e.exp(name, i, 3))


@pytest.fixture(scope="module")
def linalg_long(orc, hecdna):
    return tl.Env(orc, hecdna, N11, pc.CHAINS["LONG"], 11, pc.SCALE["LONG"], 811, n=2)


def test_he_linalg_long(linalg_long):
    """multiply_relin_rescale and sum_elems (dim 5 and 8) with entries at levels 11 and 10 in one call"""
    e = linalg_long
    sc = pc.SCALE["LONG"]
    xs = [e.xs[0], e.enc(10, sc, 841), e.xs[1]]
    ys = [e.ys[0], e.enc(10, sc, 842), e.ys[1]]
    got = e.ctx.multiply_relin_rescale([tl.up(e.ctx, c) for c in xs], [tl.up(e.ctx, c) for c in ys], e.grk)
    for g, x, y in zip(got, xs, ys):
        tl.check(g, e.prod(x, y))
    for dim in (5, 8):
        for g, c in zip(e.ctx.sum_elems([tl.up(e.ctx, c) for c in xs], dim, e.ggk), xs):
            tl.check(g, e.sum(c, dim))


def test_he_fft_one_stage_long(orc, hecdna):
    """one stage of he::fft across two ciphertexts (forward and inverse) and the in-slot FFT with n = 4 (its first
    stage and the first three-term one)"""
    m = orc.Oracle.create_coeff_modulus(N11, pc.CHAINS["LONG"])
    o = orc.Oracle(N11, m)
    sk = o.secret_key(821)
    gk = o.galois_keys(sk, [o.elt_from_step(s) for s in (1, 2, -1)], 822)
    sc = pc.SCALE["LONG"]
    ctx = hecdna.Context(N11, m)
    cts = tf.complex_cts(o, sk, 2, 11, sc, 823)
    for inverse in (False, True):
        exp = fft_ref.fft(o, hecdna, cts, inverse)
        for g, x in zip(ctx.fft([tf.up(ctx, c) for c in cts], inverse), exp):
            tf.check(g, x)
    (ct,) = tf.periodic_cts(o, sk, 1, 4, 11, sc, 824)
    for inverse in (False, True):
        tf.check(ctx.bfft(tf.up(ctx, ct), 4, ctx.galois_keys(gk), inverse), fft_ref.bfft(o, hecdna, ct, 4, gk, inverse))


@pytest.mark.parametrize("chain", ["EDGE", "ALLFP"])
def test_encode_decrypt_decode(orc, hecdna, chain):
    """GPU encode (bit-exact, up to the encoder's largest accepted magnitude: ceil(log2 max) + 1 = total bits - 1),
    decrypt (bit-exact) and decrypt_decode (the decoder's own tolerance, test_gpu_decode.py)"""
    e = td.DEnv(orc, hecdna, 11, bits=pc.CHAINS[chain])
    sc = pc.SCALE[chain]
    rng = np.random.default_rng(5)
    for level in (3, 2, 1):
        z = rng.uniform(-1, 1, (2, e.N // 2)) + 1j * rng.uniform(-1, 1, (2, e.N // 2))
        for r, g in zip(z, e.ctx.encode(z, sc, level)):
            assert g.info() == (level, sc)
            assert np.array_equal(g.download(), e.o.encode(r, sc, level))
        total = sum(q.bit_length() for q in e.m[:level])
        top = 2.0 ** (total - 2) / sc  # the constant vector has one coefficient, top * scale: the largest accepted
        for v in (np.full(e.N // 2, top), np.full(e.N // 2, -top), rng.uniform(-top, top, e.N // 2) / e.N):
            assert np.array_equal(e.ctx.encode(v[None], sc, level)[0].download(), e.o.encode(v, sc, level))
        over = np.full(e.N // 2, 1.00001 * top)
        with pytest.raises(hecdna.HecError, match="encoded values are too large"):
            e.ctx.encode(over[None], sc, level)
        with pytest.raises(orc.OracleError, match="encoded values are too large"):
            e.o.encode(over, sc, level)
    cts = [e.enc(level, 10 + level, scale=sc) for level in (1, 2, 3)]
    cts.append(e.o.multiply(e.enc(3, 20, scale=sc), e.enc(3, 21, scale=sc)))
    for c in cts:
        pt = e.ctx.decrypt(e.sk, e.up(c))
        assert pt.info() == (c.level, c.scale)
        assert np.array_equal(pt.download(), e.o.decrypt(e.sk_h, c))
        ref = e.o.decode(e.o.decrypt(e.sk_h, c), c.scale)
        e.close(e.ctx.decrypt_decode(e.sk, e.up(c)), ref, f"{chain} level {c.level} size {c.size}")
    for name in ("qm1", "half_lo", "half_hi"):  # boundary words through the secret-key product
        c = pc.pattern_ct(orc, e.m, 2, 3, e.N, [name, "qm1"], sc)
        assert np.array_equal(e.ctx.decrypt(e.sk, e.up(c)).download(), e.o.decrypt(e.sk_h, c))


def test_keygen_edge(orc, hecdna):
    """secret, public, relin and Galois keys and both encrypt forms on EDGE against tests/keygen_ref.py"""
    e = tk.KEnv(orc, hecdna, 11, bits=pc.CHAINS["EDGE"])
    assert np.array_equal(e.sk.download(), e.s)
    sdk = tk.seed("edge public")
    pk = e.ctx.keygen_public(e.sk, sdk)
    pk_h = e.ref.public(e.s, sdk)
    assert np.array_equal(pk.download(), pk_h)
    sd = tk.seed("edge relin")
    assert np.array_equal(e.ctx.keygen_relin(e.sk, sd).download(), e.ref.relin(e.s, sd))
    sd = tk.seed("edge galois")
    elts = [3, 2 * e.N - 1]
    gk = e.ctx.keygen_galois(e.sk, elts, sd)
    for elt in elts:
        assert np.array_equal(gk.download(elt), e.ref.galois(e.s, elt, sd)), elt
    sd = tk.seed("edge encrypt")
    levels = [e.L, 2, 1]
    pts = [e.pt(l, 2.0 ** 30, k) for k, l in enumerate(levels)]
    cts = e.ctx.encrypt_symmetric(e.sk, [p[2] for p in pts], sd)
    for v, ct in enumerate(cts):
        assert ct.info() == (2, levels[v], 2.0 ** 30)
        assert np.array_equal(ct.download(), e.ref.encrypt_symmetric(e.s, pts[v][1], sd, v)), v
    cts = e.ctx.encrypt(pk, [p[2] for p in pts], sd)
    for v, ct in enumerate(cts):
        assert ct.info() == (2, levels[v], 2.0 ** 30)
        assert np.array_equal(ct.download(), e.ref.encrypt(e.orc, pk_h, pts[v][1], 2.0 ** 30, sd, v)), v
