"""The chain-length limits, bit for bit against the CPU oracle: modulus chains of HEC_MAXL + 1 = 33 primes at
N = 2^10 (tests/long_chain.py has the chains and the inputs; tests/test_long_chain.py checks on the CPU that they are
what this module takes them for).  Level 32 puts 32 summands into every 128-bit and FP64 key-switch sum, index 32 into
every per-limb table passed by value, 31 and 32 digits through the digit loops (both parities of their unrolled
tails), and levels 5 .. 18 of the all-60-bit chain through the 8-, 11- and 17-word CRT of the decoder, whose
accumulator words, carries and borrows the monomial plaintexts c X^k decide one at a time.  Every assertion is equality
with the oracle, except the decoder's own tolerance (test_gpu_decode.py: tol_of, unchanged)."""
import ctypes as C

import numpy as np
import pytest

import fft_ref
import long_chain as lc
import prime_classes as pc
import seal_format as sf
import test_gpu_bsgs as tb
import test_gpu_bsgs_ctct as tbc
import test_gpu_decode as td
import test_gpu_fft as tf
import test_gpu_keygen as tk
import test_gpu_linalg_batch as tl
import test_gpu_math as tm
import test_gpu_parity as tp
import test_gpu_prime_classes as tpc

pytestmark = pytest.mark.gpu
N, L = lc.N10, lc.MAXL
ALL = ("ALL60", "FP42", "ALLFP42")
MIXED = ("ALL60", "FP42")
PAIRS = tpc.PAIRS
SCHEDULES = tpc.SWITCHES + tpc.MORE_SWITCHES
HE_SCALE = {"ALL60": 2.0**60, "FP42": 2.0**42}   # he::math, he::linalg and he::fft rescale by a data prime each step
MATVEC_STEPS = (1, 2, 4, 8, -1, -2)              # the NAF terms of the rotations 1 .. 7: the root has five children


def env_id(d):
    return ",".join(f"{k[4:]}={v}" for k, v in d.items()) or "default"


def ctx_under(hecdna, e, env):
    """a context created under the switches (they are read at creation) over the Env's chain"""
    with pytest.MonkeyPatch.context() as mp:
        for k, v in env.items():
            mp.setenv(k, v)
        return hecdna.Context(e.N, e.m)


@pytest.fixture(scope="module")
def envs(orc, hecdna):
    """one Env per chain (default Galois keys), made on first use"""
    made = {}

    def get(chain):
        if chain not in made:
            made[chain] = tp.Env(orc, hecdna, N, lc.CHAINS[chain], seed=len(chain) + 60)
        return made[chain]
    return get


def ct_pairs(e, chain, kind, level, size_a=2, size_b=2):
    sc = lc.SCALE[chain]
    if kind == "rand":
        return [(e.rand_ct(size_a, level, sc), e.rand_ct(size_b, level, sc))]
    return [(pc.pattern_ct(e.orc, e.m, size_a, level, e.N, a, sc), pc.pattern_ct(e.orc, e.m, size_b, level, e.N, b, sc))
            for a, b in PAIRS]


# =============================================================================== 1. NTT over 33 limbs ====
@pytest.mark.parametrize("chain", ALL)
def test_ntt_33_limbs(envs, chain):
    """ctx.ntt forward and inverse over all 33 limbs (pmap[32] is an index) on the boundary words, their preimages and
    a random polynomial, and at limb offset 1 over 32 limbs"""
    e = envs(chain)
    K = len(e.m)
    assert K == 33
    per_limb = [pc.transform_inputs(e.o, i, N) for i in range(K)]
    names = list(per_limb[0])
    rng = np.random.default_rng(33)
    polys = [np.stack([per_limb[i][n] for i in range(K)]) for n in names]
    polys.append(np.stack([rng.integers(0, q, N, dtype=np.uint64) for q in e.m]))
    a = np.stack(polys)
    exp_f = np.stack([np.stack([e.o.ntt_fwd(i, p[i]) for i in range(K)]) for p in a])
    exp_i = np.stack([np.stack([e.o.ntt_inv(i, p[i]) for i in range(K)]) for p in a])
    k = names.index("inv_of_qm1")
    assert np.all(exp_f[k] == np.array(e.m, dtype=np.uint64)[:, None] - 1)  # the preimages do land on q - 1
    assert np.array_equal(e.ctx.ntt(a), exp_f)
    assert np.array_equal(e.ctx.ntt(a, inverse=True), exp_i)
    assert np.array_equal(e.ctx.ntt(exp_f, inverse=True), a)
    sub = np.ascontiguousarray(a[:, 1:])
    assert sub.shape[1] == 32
    assert np.array_equal(e.ctx.ntt(sub, limb0=1), exp_f[:, 1:])
    assert np.array_equal(e.ctx.ntt(sub, limb0=1, inverse=True), exp_i[:, 1:])


# =============================================================================== 2. every evaluator operation ====
@pytest.mark.parametrize("level", [L, 2])
@pytest.mark.parametrize("kind", ["rand", "boundary"])
@pytest.mark.parametrize("chain", ALL)
def test_add_sub_negate(envs, chain, kind, level):
    e = envs(chain)
    for a, b in ct_pairs(e, chain, kind, level):
        e.same(e.ctx.add(e.up(a), e.up(b)), e.o.add(a, b))
        e.same(e.ctx.sub(e.up(a), e.up(b)), e.o.sub(a, b))
        e.same(e.ctx.negate(e.up(a)), e.o.negate(a))
    for a, c3 in ct_pairs(e, chain, kind, level, 2, 3)[:3]:
        e.same(e.ctx.add(e.up(a), e.up(c3)), e.o.add(a, c3))
        e.same(e.ctx.sub(e.up(a), e.up(c3)), e.o.sub(a, c3))
        e.same(e.ctx.add(e.up(c3), e.up(a)), e.o.add(c3, a))


@pytest.mark.parametrize("level", [L, 2])
@pytest.mark.parametrize("kind", ["rand", "boundary"])
@pytest.mark.parametrize("chain", ALL)
def test_multiply_square(envs, chain, kind, level):
    e = envs(chain)
    for a, b in ct_pairs(e, chain, kind, level):
        e.same(e.ctx.multiply(e.up(a), e.up(b)), e.o.multiply(a, b))
        e.same(e.ctx.square(e.up(a)), e.o.square(a))
        e.same(e.ctx.square(e.up(b)), e.o.square(b))
    for c3, a in ct_pairs(e, chain, kind, level, 3, 2)[:3]:
        e.same(e.ctx.multiply(e.up(c3), e.up(a)), e.o.multiply(c3, a))


@pytest.mark.parametrize("level", [L, 2])
@pytest.mark.parametrize("kind", ["rand", "boundary"])
@pytest.mark.parametrize("chain", ALL)
def test_plain_ops(envs, chain, kind, level):
    e = envs(chain)
    sc = lc.SCALE[chain]
    for a, b in ct_pairs(e, chain, kind, level):
        pt = b.data[1]
        p = e.ctx.plaintext(pt, sc)
        e.same(e.ctx.multiply_plain(e.up(a), p), e.o.multiply_plain(a, pt, sc))
        e.same(e.ctx.add_plain(e.up(a), p), e.o.add_plain(a, pt, sc))
        e.same(e.ctx.sub_plain(e.up(a), p), e.o.sub_plain(a, pt, sc))


@pytest.mark.parametrize("level", [L, 2])
@pytest.mark.parametrize("kind", ["rand", "boundary"])
@pytest.mark.parametrize("chain", ALL)
def test_relinearize_rescale_modswitch(envs, chain, kind, level):
    """level 32: the special prime, then q_31, divides; 32 digits in the relinearisation's sums"""
    e = envs(chain)
    for c3, c2 in ct_pairs(e, chain, kind, level, 3, 2):
        e.same(e.ctx.relinearize(e.up(c3), e.rk), e.o.relinearize(c3, e.rk_h))
        e.same(e.ctx.rescale_to_next(e.up(c3)), e.o.rescale(c3))
        e.same(e.ctx.rescale_to_next(e.up(c2)), e.o.rescale(c2))
        e.same(e.ctx.mod_switch_to_next(e.up(c2)), e.o.mod_switch(c2))


@pytest.mark.parametrize("level", [L, 2])
@pytest.mark.parametrize("kind", ["rand", "boundary"])
@pytest.mark.parametrize("chain", ALL)
def test_rotate_and_conjugate(envs, chain, kind, level):
    e = envs(chain)
    for a, b in ct_pairs(e, chain, kind, level)[:3]:
        for steps in (1, 3, -1, 511):
            e.same(e.ctx.rotate_vector(e.up(a), steps, e.gk), e.o.rotate(a, steps, e.gk_h))
        elt = 2 * e.N - 1
        e.same(e.ctx.apply_galois(e.up(b), elt, e.gk), e.o.apply_galois(b, elt, e.gk_h))


# =============================================================================== 3. key switch at l = 32 ====
class SwitchCase:
    """Per chain: the keys (plain u64[L][2][K][N] arrays on both sides) and, per named input, a size-3 ciphertext
    whose c2 is the target (relinearize) and a size-2 one whose c1 is (rotation by one step), with the oracle's results.
      worst:  every target word q_J - 1, every key word q_I - 1: the largest 128-bit sums (2^125 of 2^128)
      halves: every target word 1, every key word (q_I - 1) / 2: 32 FP64 products of +(q - 1) / 2 each, 16 q of the
              18.02 q the FP64 sums are bounded by
      rand:   uniform target, a generated key
      qm1, half_hi: those words in the target, a generated key
    Constant words are their own Galois permutation, so the rotation's target is the same polynomial."""

    def __init__(self, e, chain):
        self.e = e
        o, m, sc = e.o, e.m, lc.SCALE[chain]
        self.elt = o.elt_from_step(1)
        wt, wk = lc.worst_switch(m, L, N)
        hk = np.empty_like(wk)
        for i in range(len(m)):
            hk[:, :, i, :] = (int(m[i]) - 1) // 2
        self.keys = {"worst": (wk, wk), "halves": (hk, hk), "rand": (e.rk_h, e.gk_h[self.elt])}
        targets = {"worst": ("worst", wt), "halves": ("halves", pc.pattern_poly(m, L, N, "one")),
                   "rand": ("rand", e.rand_ct(1, L, sc).data[0]),
                   "qm1": ("rand", pc.pattern_poly(m, L, N, "qm1")),
                   "half_hi": ("rand", pc.pattern_poly(m, L, N, "half_hi"))}
        self.cases = {}
        for name, (key, t) in targets.items():
            base = e.rand_ct(2, L, sc).data
            c3 = e.orc.Ct(np.concatenate([base, t[None]]), sc)
            c2 = e.orc.Ct(np.stack([base[0], t]), sc)
            rk_h, gk_h = self.keys[key]
            self.cases[name] = (key, c3, o.relinearize(c3, rk_h), c2, o.rotate(c2, 1, {self.elt: gk_h}))


@pytest.fixture(scope="module")
def switch_cases(envs):
    made = {}

    def get(chain):
        if chain not in made:
            made[chain] = SwitchCase(envs(chain), chain)
        return made[chain]
    return get


@pytest.mark.parametrize("env", [{}] + SCHEDULES, ids=env_id)
@pytest.mark.parametrize("chain", MIXED)
def test_keyswitch_l32_schedules(hecdna, switch_cases, chain, env):
    """relinearize and one rotation at l = 32 under the default and under every alternative key-switch schedule; the
    schedules that have no instance at N = 2^10 must change nothing"""
    sc = switch_cases(chain)
    e = sc.e
    ctx = ctx_under(hecdna, e, env)
    keys = {k: (ctx.relin_key(r), ctx.galois_keys({sc.elt: g})) for k, (r, g) in sc.keys.items()}
    for name, (key, c3, exp3, c2, exp2) in sc.cases.items():
        rk, gk = keys[key]
        e.same(ctx.relinearize(ctx.ciphertext(c3.data, c3.scale), rk), exp3)
        e.same(ctx.rotate_vector(ctx.ciphertext(c2.data, c2.scale), 1, gk), exp2)
    ctx.close()


# =============================================================================== 4. hoisted matvec ====
class MatvecCase:
    """n = 8 diagonals, p = 3 vectors at one level, keys for the NAF terms of the rotations only; the oracle's ct x ct
    and ct x pt products"""

    def __init__(self, orc, hecdna, chain, level):
        bits, sc = lc.CHAINS[chain], lc.SCALE[chain]
        o = orc.Oracle(N, orc.Oracle.create_coeff_modulus(N, bits))
        self.e = e = tp.Env(orc, hecdna, N, bits, seed=70 + level, elts=[o.elt_from_step(s) for s in MATVEC_STEPS])
        self.sc = sc
        self.A = [e.enc(level=level, scale=sc, seed=j) for j in range(8)]
        self.X = [e.enc(level=level, scale=sc, seed=40 + i) for i in range(3)]
        self.P = [e.o.encode(e.rng.uniform(-1, 1, N // 2), sc, level) for _ in range(8)]
        self.exp = e.o.matmul_diag_col(self.A, self.X, e.rk_h, e.gk_h)
        self.exp_pt = e.o.matmul_diagpt_col_set(self.P, sc, list(range(8)), self.X, e.gk_h)

    def check(self, ctx):
        e = self.e
        up = lambda c: ctx.ciphertext(c.data, c.scale)  # noqa: E731
        rk, gk = (e.rk, e.gk) if ctx is e.ctx else (ctx.relin_key(e.rk_h), ctx.galois_keys(e.gk_h))
        got = ctx.matmul_diag_col([up(a) for a in self.A], [up(x) for x in self.X], rk, gk)
        for g, c in zip(got, self.exp):
            e.same(g, c)
        got = ctx.matmul_diagpt_col([ctx.plaintext(p, self.sc) for p in self.P], [up(x) for x in self.X], gk)
        for g, c in zip(got, self.exp_pt):
            e.same(g, c)


@pytest.fixture(scope="module")
def matvec_cases(orc, hecdna):
    made = {}

    def get(chain, level):
        if (chain, level) not in made:
            made[chain, level] = MatvecCase(orc, hecdna, chain, level)
        return made[chain, level]
    return get


HOISTED = [{}, {"HEC_HMAC": "0"}, {"HEC_HMAC": "1"}, {"HEC_HMAC_INT": "0"}, {"HEC_HMAC_DIVROUND": "0"},
           {"HEC_HOIST": "0"}]


@pytest.mark.parametrize("env", HOISTED, ids=env_id)
@pytest.mark.parametrize("level", [L, L - 1])
@pytest.mark.parametrize("chain", MIXED)
def test_hoisted_matvec(hecdna, matvec_cases, chain, level, env):
    """ct x ct and ct x pt, n = 8, p = 3: the root's five children form sibling groups of the hoisted MAC.  Levels 32
    and 31: l - 1 and l digits at the data targets and at the special prime are 31 / 32 and 30 / 31, both parities of
    k_hmacm's loop unrolled by two"""
    mc = matvec_cases(chain, level)
    if not env:
        mc.check(mc.e.ctx)
        return
    ctx = ctx_under(hecdna, mc.e, env)
    mc.check(ctx)
    ctx.close()


@pytest.mark.parametrize("env", [{}, {"HEC_HMAC": "1"}, {"HEC_HMAC_DIVROUND": "0"}], ids=env_id)
@pytest.mark.parametrize("level", [L, L - 1])
def test_hoisted_matvec_all_fp(hecdna, matvec_cases, level, env):
    """q_0 and the special prime in the FP64 class: every hoisted sum is an FP64 one, and the special prime's 32 digits
    at level 32 (31 at level 31) are the only run of the FP64 loop's two-digit (one-digit) tail at that count"""
    mc = matvec_cases("ALLFP42", level)
    if not env:
        mc.check(mc.e.ctx)
        return
    ctx = ctx_under(hecdna, mc.e, env)
    mc.check(ctx)
    ctx.close()


@pytest.mark.parametrize("chain", MIXED)
def test_hoisted_walk_zero_list_overflow_l32(matvec_cases, chain):
    """a column whose c1 has q_J - 1 in every NTT word: N - 1 zero coefficients in each of the 32 digits, far more than
    the hoisted mod-up lists, so the walk falls back; a second, ordinary column shares the batch"""
    mc = matvec_cases(chain, L)
    e = mc.e
    worst = e.orc.Ct(np.stack([e.rand_ct(1, L, mc.sc).data[0], lc.worst_switch(e.m, L, N)[0]]), mc.sc)
    X = [worst, mc.X[0]]
    exp = e.o.matmul_diag_col(mc.A, X, e.rk_h, e.gk_h)
    got = e.ctx.matmul_diag_col([e.up(a) for a in mc.A], [e.up(x) for x in X], e.rk, e.gk)
    for g, c in zip(got, exp):
        e.same(g, c)
    e.same(got[1], mc.exp[0])


# =============================================================================== 5. BSGS, both forms ====
@pytest.mark.parametrize("chain", MIXED)
def test_bsgs_l32(envs, chain):
    """n = 8, bs = 3 (two full giant groups and a partial one), p = 3, level 32, against the per-operation composition"""
    e = envs(chain)
    sc = lc.SCALE[chain]
    X = [e.enc(level=L, scale=sc, seed=500 + i) for i in range(3)]
    P = [e.o.encode(e.rng.uniform(-1, 1, N // 2), sc, L) for _ in range(8)]
    exp = tb.bsgs_oracle(e, P, X, 3, e.gk_h, sc)
    got = e.ctx.matmul_diagpt_col_bsgs([e.ctx.plaintext(q, sc) for q in P], [e.up(x) for x in X], e.gk, bs=3)
    for g, c in zip(got, exp):
        e.same(g, c)
    A = [e.enc(level=L, scale=sc, seed=520 + j) for j in range(8)]
    exp = tbc.bsgs_oracle(e, A, X, 3, e.rk_h, e.gk_h)
    got = e.ctx.matmul_diag_col_bsgs([e.up(a) for a in A], [e.up(x) for x in X], e.rk, e.gk, bs=3)
    for g, c in zip(got, exp):
        e.same(g, c)


# =============================================================================== 6. the batched layers ====
@pytest.fixture(scope="module")
def math_envs(orc, hecdna):
    made = {}

    def get(chain):
        if chain not in made:
            made[chain] = tm.Env(orc, hecdna, N, lc.CHAINS[chain], L, HE_SCALE[chain], 901)
        return made[chain]
    return get


@pytest.mark.parametrize("name,iters", [("signed_inv", 29), ("sqrt", 15)])
@pytest.mark.parametrize("chain", MIXED)
def test_he_math_down_the_chain(math_envs, chain, name, iters):
    """one call from level 32 to level 2 (signed_inv: one level per iteration; sqrt: two), B = 2: every level of the
    chain is the top of a product, a relinearisation and a rescale once"""
    e = math_envs(chain)
    cts = e.inputs(name)[:2]
    got = getattr(e.ctx, name)([tm.up(e.ctx, c) for c in cts], tm.A[name], iters, e.grk)
    for i, g in enumerate(got):
        exp = e.exp(name, i, iters)
        assert exp.level == 2
        tm.check(g, exp)


@pytest.mark.parametrize("chain", MIXED)
def test_he_linalg_mixed_levels(orc, hecdna, chain):
    """multiply_relin_rescale and sum_elems (dim 5 and 8) with entries at levels 32 and 3 in one call"""
    sc = HE_SCALE[chain]
    e = tl.Env(orc, hecdna, N, lc.CHAINS[chain], L, sc, 911, n=2)
    xs = [e.xs[0], e.enc(3, sc, 941), e.xs[1]]
    ys = [e.ys[0], e.enc(3, sc, 942), e.ys[1]]
    got = e.ctx.multiply_relin_rescale([tl.up(e.ctx, c) for c in xs], [tl.up(e.ctx, c) for c in ys], e.grk)
    for g, x, y in zip(got, xs, ys):
        tl.check(g, e.prod(x, y))
    for dim in (5, 8):
        for g, c in zip(e.ctx.sum_elems([tl.up(e.ctx, c) for c in xs], dim, e.ggk), xs):
            tl.check(g, e.sum(c, dim))


@pytest.mark.parametrize("chain", MIXED)
def test_he_fft_l32(orc, hecdna, chain):
    """one stage of he::fft across two ciphertexts (forward and inverse) and the in-slot FFT with n = 4, from level 32"""
    m = orc.Oracle.create_coeff_modulus(N, lc.CHAINS[chain])
    o = orc.Oracle(N, m)
    sk = o.secret_key(921)
    gk = o.galois_keys(sk, [o.elt_from_step(s) for s in (1, 2, -1)], 922)
    sc = HE_SCALE[chain]
    ctx = hecdna.Context(N, m)
    cts = tf.complex_cts(o, sk, 2, L, sc, 923)
    for inverse in (False, True):
        exp = fft_ref.fft(o, hecdna, cts, inverse)
        for g, x in zip(ctx.fft([tf.up(ctx, c) for c in cts], inverse), exp):
            tf.check(g, x)
    (ct,) = tf.periodic_cts(o, sk, 1, 4, L, sc, 924)
    for inverse in (False, True):
        tf.check(ctx.bfft(tf.up(ctx, ct), 4, ctx.galois_keys(gk), inverse), fft_ref.bfft(o, hecdna, ct, 4, gk, inverse))


# =============================================================================== 7. encode and decrypt ====
@pytest.fixture(scope="module")
def denvs(orc, hecdna):
    made = {}

    def get(chain):
        if chain not in made:
            made[chain] = td.DEnv(orc, hecdna, 10, bits=lc.CHAINS[chain])
        return made[chain]
    return get


@pytest.mark.parametrize("chain", ALL)
def test_encode_decrypt_l32(denvs, chain):
    """encode at level 32, bit-exact, up to a constant vector whose single coefficient value x scale is +-2^1022 (the
    largest finite path of the residue computation); decrypt of size 2 and size 3 at level 32, bit-exact"""
    e = denvs(chain)
    sc = lc.SCALE[chain]
    rng = np.random.default_rng(7)
    z = rng.uniform(-1, 1, (2, N // 2)) + 1j * rng.uniform(-1, 1, (2, N // 2))
    for r, g in zip(z, e.ctx.encode(z, sc, L)):
        assert g.info() == (L, sc)
        assert np.array_equal(g.download(), e.o.encode(r, sc, L))
    top = 2.0**1022 / sc
    for v in (np.full(N // 2, top), np.full(N // 2, -top), rng.uniform(-top, top, N // 2) / N):
        want = e.o.encode(v, sc, L)
        assert np.array_equal(e.ctx.encode(v[None], sc, L)[0].download(), want)
    for i in (0, L - 1):  # the constant's one coefficient is 2^1022 exactly
        co = e.o.ntt_inv(i, e.o.encode(np.full(N // 2, top), sc, L)[i])
        assert int(co[0]) == pow(2, 1022, e.m[i]) and not co[1:].any()
    cts = [e.enc(L, 11, scale=sc), e.o.multiply(e.enc(L, 20, scale=sc), e.enc(L, 21, scale=sc))]
    assert [c.size for c in cts] == [2, 3]
    for c in cts:
        pt = e.ctx.decrypt(e.sk, e.up(c))
        assert pt.info() == (c.level, c.scale)
        assert np.array_equal(pt.download(), e.o.decrypt(e.sk_h, c))
    for name in ("qm1", "half_hi"):  # boundary words through the secret-key product at every one of the 32 limbs
        c = pc.pattern_ct(e.orc, e.m, 3, L, N, [name, "qm1", "half_lo"], sc)
        assert np.array_equal(e.ctx.decrypt(e.sk, e.up(c)).download(), e.o.decrypt(e.sk_h, c))


# =============================================================================== 8. decode through every CRT class ====
def ratio(got, ref, what):
    """DEnv.close's assertion without its line of output per row: the 2-norm of the difference within tol_of(ref)"""
    err = float(np.linalg.norm(np.asarray(got) - ref[: len(got)]))
    tol = float(td.tol_of(ref, N))
    assert np.isfinite(tol) and err <= tol, (what, err, tol)
    return err / tol


@pytest.mark.parametrize("level", lc.DECODE_LEVELS)
def test_decode_random_every_class(denvs, level):
    """a random encoding as a plaintext and as a ciphertext through decrypt_decode, within tol_of of the oracle"""
    e = denvs("ALL60")
    scale = 2.0**40
    pt = e.o.encode(e.vals(), scale, level)
    got = e.ctx.decode(e.ctx.plaintext(pt, scale))
    e.close(got, e.o.decode(pt, scale), f"ALL60 level {level} WM {lc.wm_class(lc.crt_words(e.m, level))} plaintext")
    ct = e.enc(level, 5 + level)
    ref = e.o.decode(e.o.decrypt(e.sk_h, ct), scale)
    e.close(e.ctx.decrypt_decode(e.sk, e.up(ct)), ref, f"ALL60 level {level} ciphertext")


@pytest.mark.parametrize("level", lc.DECODE_LEVELS)
def test_decode_monomial_grid(denvs, level):
    """c X^k for every c of the grid in one decode call: within tol_of of the closed form and of the oracle"""
    e = denvs("ALL60")
    cs = lc.grid(e.m, level)
    ks = [lc.grid_k(idx, N) for idx in range(len(cs))]
    scales = [lc.grid_scale(c) for c in cs]
    pts = [lc.monomial_plain(e.o, e.m, level, c, k, N) for c, k in zip(cs, ks)]
    got = e.ctx.decode([e.ctx.plaintext(p, s) for p, s in zip(pts, scales)])
    assert got.shape == (len(cs), N // 2)
    r_exact = r_oracle = 0.0
    for c, k, s, p, row in zip(cs, ks, scales, pts, got):
        what = f"level {level} c = {'-' if c < 0 else ''}2^{np.log2(float(abs(c))):.3f} k = {k}"
        r_exact = max(r_exact, ratio(row, lc.monomial_slots(c, s, k, N), what + " exact"))
        r_oracle = max(r_oracle, ratio(row, e.o.decode(p, s), what + " oracle"))
    print(f"decode monomial grid ALL60 level {level} WM {lc.wm_class(lc.crt_words(e.m, level))} ({len(cs)} monomials): "
          f"max error / tol {r_exact:.3f} against the closed form, {r_oracle:.3f} against the oracle")


def test_decode_too_wide_writes_nothing(hecdna, denvs):
    """levels 19 and 32 of ALL60 need 18 and 31 words: InvalidArgument, alone and behind a good entry, outputs untouched"""
    e = denvs("ALL60")
    lib = hecdna.lib()
    scale = 2.0**40
    good = e.ctx.plaintext(e.o.encode(e.vals(), scale, 4), scale)
    sentinel = np.full((2, 8), 7.5)
    dp = C.POINTER(C.c_double)
    for level in lc.REJECT_LEVELS:
        bad = e.ctx.plaintext(e.o.encode(e.vals(), scale, level), scale)
        with pytest.raises(hecdna.InvalidArgument, match="too wide"):
            e.ctx.decode(bad)
        re, im = sentinel.copy(), sentinel.copy()
        arr = (C.c_void_p * 2)(good.h.value, bad.h.value)
        rc = lib.hec_decode(e.ctx.h, arr, 2, 8, re.ctypes.data_as(dp), im.ctypes.data_as(dp))
        assert rc == hecdna.HEC_EINVAL and "too wide" in lib.hec_last_error().decode()
        assert np.array_equal(re, sentinel) and np.array_equal(im, sentinel)
        ct = e.enc(level, 50 + level)
        with pytest.raises(hecdna.InvalidArgument, match="too wide"):
            e.ctx.decrypt_decode(e.sk, e.up(ct))
    e.close(e.ctx.decode(good), e.o.decode(good.download(), scale), "level 4 after the rejections")


def test_decode_mixed_classes_in_one_call(denvs):
    """one entry per word-count class, and level 1, in one decode call, at different scales"""
    e = denvs("ALL60")
    levels = [8, 17, 1, 4, 18, 11]
    assert {lc.wm_class(lc.crt_words(e.m, lv)) for lv in levels} == set(lc.WM_CLASSES)
    scales = [2.0**(30 + 3 * i) for i in range(len(levels))]
    pts = [e.o.encode(e.vals(), s, lv) for s, lv in zip(scales, levels)]
    got = e.ctx.decode([e.ctx.plaintext(p, s) for p, s in zip(pts, scales)])
    for lv, p, s, row in zip(levels, pts, scales, got):
        e.close(row, e.o.decode(p, s), f"mixed batch level {lv}")
        assert np.array_equal(row, e.ctx.decode(e.ctx.plaintext(p, s)))  # the same doubles alone


# =============================================================================== 9. keygen and encryption ====
@pytest.fixture(scope="module")
def kenv(orc, hecdna):
    return tk.KEnv(orc, hecdna, 10, bits=lc.CHAINS["FP42"])


def test_keygen_secret_public_relin_k33(kenv):
    e = kenv
    assert e.K == 33
    assert np.array_equal(e.sk.download(), e.s)
    sdk = tk.seed("long public")
    assert np.array_equal(e.ctx.keygen_public(e.sk, sdk).download(), e.ref.public(e.s, sdk))
    sd = tk.seed("long relin")
    assert np.array_equal(e.ctx.keygen_relin(e.sk, sd).download(), e.ref.relin(e.s, sd))


def test_keygen_galois_k33(kenv):
    e = kenv
    sd = tk.seed("long galois")
    elts = [3, 2 * e.N - 1]
    gk = e.ctx.keygen_galois(e.sk, elts, sd)
    for elt in elts:
        assert np.array_equal(gk.download(elt), e.ref.galois(e.s, elt, sd)), elt


def test_encrypt_k33(kenv):
    e = kenv
    sdk = tk.seed("long public")
    pk = e.ctx.keygen_public(e.sk, sdk)
    pk_h = e.ref.public(e.s, sdk)
    sd = tk.seed("long encrypt")
    levels = [e.L, 2, 1]
    assert e.L == 32
    pts = [e.pt(lv, 2.0**30, k) for k, lv in enumerate(levels)]
    cts = e.ctx.encrypt_symmetric(e.sk, [p[2] for p in pts], sd)
    for v, ct in enumerate(cts):
        assert ct.info() == (2, levels[v], 2.0**30)
        assert np.array_equal(ct.download(), e.ref.encrypt_symmetric(e.s, pts[v][1], sd, v)), v
    cts = e.ctx.encrypt(pk, [p[2] for p in pts], sd)
    for v, ct in enumerate(cts):
        assert ct.info() == (2, levels[v], 2.0**30)
        assert np.array_equal(ct.download(), e.ref.encrypt(e.orc, pk_h, pts[v][1], 2.0**30, sd, v)), v


# =============================================================================== 10. SEAL wire format ====
def test_seal_round_trip_k33(envs, hecdna):
    """one ciphertext at level 32 saved and loaded (plain and zstd), and the relinearisation key of 32 x 2 x 33 limbs
    loaded from its SEAL bytes"""
    e = envs("FP42")
    sc = lc.SCALE["FP42"]
    ct = e.enc(level=L, scale=sc, seed=1)
    blob = sf.ciphertext(ct.data, ct.scale, e.m)
    g = hecdna.Ciphertext(e.ctx)
    assert g.load_seal(blob + b"tail") == len(blob)
    e.same(g, ct)
    assert e.up(ct).save_seal(hecdna.COMPR_NONE) == blob
    h = hecdna.Ciphertext(e.ctx)
    h.load_seal(e.up(ct).save_seal())
    e.same(h, ct)
    rk = hecdna.KSwitchKey(e.ctx, seal_bytes=sf.kswitch_keys(e.N, e.m, [e.rk_h]))
    assert np.array_equal(rk.download(), e.rk_h)
    a = e.rand_ct(3, L, sc)
    e.same(e.ctx.relinearize(e.up(a), rk), e.o.relinearize(a, e.rk_h))


# =============================================================================== the mod-up passes' job count ====
@pytest.fixture(scope="module")
def wide_batch(orc, hecdna):
    """p = 64 vectors and n = 2 diagonals at level 32 on FP42, the key for the one rotation, and the oracle's product
    for three of the vectors"""
    bits, sc = lc.CHAINS["FP42"], lc.SCALE["FP42"]
    o = orc.Oracle(N, orc.Oracle.create_coeff_modulus(N, bits))
    e = tp.Env(orc, hecdna, N, bits, seed=64, elts=[o.elt_from_step(1)])
    A = [e.enc(level=L, scale=sc, seed=j) for j in range(2)]
    X = [e.enc(level=L, scale=sc, seed=100 + i) for i in range(64)]
    picks = (0, 31, 63)
    return e, A, X, picks, e.o.matmul_diag_col(A, [X[i] for i in picks], e.rk_h, e.gk_h)


def test_wide_batch_default_schedule(wide_batch):
    """the default schedule's launches have B l jobs along y: 64 vectors in one call equal two calls of 32"""
    e, A, X, picks, exp = wide_batch
    gA = [e.up(a) for a in A]
    one = e.ctx.matmul_diag_col(gA, [e.up(x) for x in X], e.rk, e.gk)
    two = (e.ctx.matmul_diag_col(gA, [e.up(x) for x in X[:32]], e.rk, e.gk)
           + e.ctx.matmul_diag_col(gA, [e.up(x) for x in X[32:]], e.rk, e.gk))
    assert len(one) == len(two) == 64
    for g, h in zip(one, two):
        assert g.info() == h.info() and np.array_equal(g.download(), h.download())
    for i, c in zip(picks, exp):
        e.same(one[i], c)


@pytest.mark.parametrize("env", [{"HEC_FAN": "0"}, {"HEC_FUSED_MODUP_MAC": "0"}], ids=env_id)
def test_wide_batch_modup_jobs_rejected(hecdna, wide_batch, env):
    """the A/B-only mod-up passes have B l l jobs along y: 64 x 32 x 32 = 65,536 is one past the launch limit and is
    refused by name before the launch; 63 vectors fit and give the oracle's words"""
    e, A, X, picks, exp = wide_batch
    ctx = ctx_under(hecdna, e, env)
    up = lambda c: ctx.ciphertext(c.data, c.scale)  # noqa: E731
    rk, gk = ctx.relin_key(e.rk_h), ctx.galois_keys(e.gk_h)
    gA = [up(a) for a in A]
    with pytest.raises(hecdna.InvalidArgument, match="too many ciphertexts for one mod-up pass.*65535"):
        ctx.matmul_diag_col(gA, [up(x) for x in X], rk, gk)
    got = ctx.matmul_diag_col(gA, [up(x) for x in X[1:]], rk, gk)
    assert len(got) == 63
    e.same(got[30], exp[1])
    e.same(got[62], exp[2])
    ctx.close()
