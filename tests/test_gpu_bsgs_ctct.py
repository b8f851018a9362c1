"""hec_matmul_diag_col_bsgs: the ct x ct matvec on the baby-step giant-step schedule, bit-exact against the oracle's
per-operation composition in the schedule's order (rotate, multiply, add, relinearize, rotate, add, rescale), over
both key shapes (a key per planned step; the default power-of-two set, whose rotations are NAF chains), and its
errors.  N = 2^11, [50, 36, 36, 50]: both prime classes at level 3.  n = 24, p = 3: the batch does not divide the
kernel's BG = 2.  The diagonals are encryptions of bsgs_diagonals(D, bs)'s rows."""
import numpy as np
import pytest

from _helpers import col_vector, diag_vectors
from test_gpu_parity import Env

pytestmark = pytest.mark.gpu

N11, BITS11 = 1 << 11, [50, 36, 36, 50]
n, p = 24, 3
# test_functional_against_plain_product: twice the worst ratio (BSGS error / reference schedule's error) that
# tools/bsgs_ctct_error.py measured on the CPU over five seeds with the oracle alone: 0.467, 0.297, 0.188, 0.551, 0.811
# 
ERR_RATIO_M = 2 * 0.8108
TILES = [(bg, gg, order) for bg in (1, 2) for gg in (2, 4, 8) for order in (0, 1)]
DEFAULT_TILE = {"bsgs_ct_bg": 2, "bsgs_ct_gg": 8, "bsgs_order": 1}


def bsgs_oracle(e, A, X, bs, rk_h, gk_h):
    """The definition, from pinned oracle operations: inner_g = sum_i multiply(rotate(x, i), A'[g bs + i]),
    r_g = relinearize(inner_g), out = rescale(r_0 + sum_{g >= 1} rotate(r_g, g bs))."""
    eff = min(bs, len(A))
    G = -(-len(A) // eff)
    outs = []
    for x in X:
        rots = [x] + [e.o.rotate(x, i, gk_h) for i in range(1, eff)]
        acc = None
        for g in range(G):
            inner = None
            for i in range(eff):
                if g * eff + i >= len(A):
                    break
                t = e.o.multiply(rots[i], A[g * eff + i])
                inner = t if inner is None else e.o.add(inner, t)
            r = e.o.relinearize(inner, rk_h)
            r = r if g == 0 else e.o.rotate(r, g * eff, gk_h)
            acc = r if acc is None else e.o.add(acc, r)
        outs.append(e.o.rescale(acc))
    return outs


class Case:
    """One matrix, p input vectors and their encryptions under one secret key (Env's seed fixes it, so every key
    set below belongs to the same key); the BSGS-form diagonals per block size, encrypted once (diagonal j with seed
    7000 + j whatever the block size) and left unchanged."""

    def __init__(self, orc, hecdna):
        self.orc, self.hec = orc, hecdna
        self.e = Env(orc, hecdna, N11, BITS11)  # default Galois keys
        e = self.e
        self.L = len(e.m) - 1
        rng = np.random.default_rng(2025)
        self.M = rng.uniform(-1, 1, (n, n))
        self.x = rng.uniform(-1, 1, (p, n))
        self.D = np.stack(diag_vectors(self.M, e.N // 2))
        self.X = [e.enc(col_vector(self.x[i], e.N // 2), seed=4000 + i) for i in range(p)]
        self._A, self._env = {}, {}

    def A(self, bs):
        if bs not in self._A:
            rows = self.D if bs is None else self.hec.bsgs_diagonals(self.D, bs)
            self._A[bs] = [self.e.enc(r, seed=7000 + j) for j, r in enumerate(rows)]
        return self._A[bs]

    def env_with_step_keys(self, bs):
        """The same secret key (and relinearisation key) with a Galois key for exactly the planned steps of (n, bs)."""
        if bs not in self._env:
            _, steps = self.hec.bsgs_plan(n, bs)
            self._env[bs] = Env(self.orc, self.hec, N11, BITS11, elts=[self.e.o.elt_from_step(s) for s in steps])
        return self._env[bs]


@pytest.fixture(scope="module")
def case(orc, hecdna):
    return Case(orc, hecdna)


def run(e, A, X, bs, out=None):
    return e.ctx.matmul_diag_col_bsgs([e.up(a) for a in A], [e.up(x) for x in X], e.rk, e.gk, bs=bs, out=out)


def words(cts):
    return [(g.info(), g.download()) for g in cts]


def same_words(got, want):
    for g, w in zip(got, want):
        assert g.info() == w[0] and np.array_equal(g.download(), w[1])


# ------------------------------------------------------------------ 1. bit-exact against the composition
@pytest.mark.parametrize("bs", [5, 8])
@pytest.mark.parametrize("keys", ["per_step", "default"])
def test_bitexact_against_oracle_composition(case, bs, keys):
    """per_step: every rotation is one key switch.  default: NAF tries deeper than 1 and multi-element giant
    rotations.  bs = 5 leaves a partial last giant group (24 = 4 x 5 + 4) and G = 5: the default tile of 8 giants is
    partial, and it relinearises giant 0 (into the accumulator) apart from its other four (bs = 8: G = 3)."""
    e = case.env_with_step_keys(bs) if keys == "per_step" else case.e
    exp = bsgs_oracle(e, case.A(bs), case.X, bs, e.rk_h, e.gk_h)
    got = run(e, case.A(bs), case.X, bs)
    for g, c in zip(got, exp):
        e.same(g, c)


# ------------------------------------------------------------------ 2. degenerate and coinciding block sizes
@pytest.mark.parametrize("bs", [24, 32])
def test_whole_matrix_block_equals_reference_schedule(case, bs):
    """bs_eff = n: one giant group, no giant rotation, A' = A, and the two definitions coincide word for word."""
    e = case.e
    diags = [e.up(a) for a in case.A(bs)]
    cols = [e.up(x) for x in case.X]
    ref = e.ctx.matmul_diag_col(diags, cols, e.rk, e.gk)
    got = e.ctx.matmul_diag_col_bsgs(diags, cols, e.rk, e.gk, bs=bs)
    same_words(got, words(ref))


def test_block_size_one_is_all_giants(case):
    e = case.e
    exp = bsgs_oracle(e, case.A(1), case.X, 1, e.rk_h, e.gk_h)
    for g, c in zip(run(e, case.A(1), case.X, 1), exp):
        e.same(g, c)


def test_default_block_size(case, hecdna):
    """bs=None is the smallest power of two >= sqrt(24) = 8."""
    e = case.e
    assert hecdna.bsgs_plan(n)[0] == 8
    same_words(run(e, case.A(8), case.X, None), words(run(e, case.A(8), case.X, 8)))


# ------------------------------------------------------------------ 3. batch, chunk and tile independence
def test_batch_and_chunk_independence(case):
    e = case.e
    whole = words(run(e, case.A(8), case.X, 8))
    for i in range(p):
        same_words(run(e, case.A(8), [case.X[i]], 8), whole[i:i + 1])
    e.ctx.set_option("bsgs_chunk", 2)  # passes of 2 and 1 vectors
    try:
        chunked = run(e, case.A(8), case.X, 8)
    finally:
        e.ctx.set_option("bsgs_chunk", 0)
    same_words(chunked, whole)


@pytest.fixture(scope="module")
def default_tile_words(case):
    return words(run(case.e, case.A(5), case.X, 5))


@pytest.mark.parametrize("bg,gg,order", TILES)
def test_kernel_tiles_compute_the_same_words(case, default_tile_words, bg, gg, order):
    """Every tile of k_bsgs_inner_ct and both grid orders give the default's bits (G = 5 at bs = 5: partial tiles for
    every gg; p = 3: a partial batch group for bg = 2)."""
    e = case.e
    try:
        for k, v in {"bsgs_ct_bg": bg, "bsgs_ct_gg": gg, "bsgs_order": order}.items():
            e.ctx.set_option(k, v)
        got = run(e, case.A(5), case.X, 5)
    finally:
        for k, v in DEFAULT_TILE.items():
            e.ctx.set_option(k, v)
    same_words(got, default_tile_words)


@pytest.mark.parametrize("name,value", [("bsgs_ct_bg", 0), ("bsgs_ct_bg", 4), ("bsgs_ct_gg", 1), ("bsgs_ct_gg", 3),
                                        ("bsgs_ct_gg", 16)])
def test_tile_outside_the_instantiated_set_is_refused(case, name, value):
    with pytest.raises(case.hec.InvalidArgument):
        case.e.ctx.set_option(name, value)


def test_output_may_be_its_own_input(case):
    e = case.e
    exp = words(run(e, case.A(8), case.X, 8))
    cols = [e.up(x) for x in case.X]
    got = e.ctx.matmul_diag_col_bsgs([e.up(a) for a in case.A(8)], cols, e.rk, e.gk, bs=8, out=cols)
    assert all(g is c for g, c in zip(got, cols))
    same_words(got, exp)


def test_rotate_diagonals_from_natural_form(case):
    """bsgs_rotate_diagonals: diagonal j rotated right by (j // 8) * 8 slots with the per-ciphertext rotate call (the
    default keys' NAF chains of the negative steps), the inputs left as they are; the matvec on the result decrypts to
    M @ x.  The words are checked against the oracle's rotate; the decrypted product only has to tell the right
    convention from a wrong one (a wrong step or direction errs by the size of M @ x, about 1, where the schedules'
    own error at these parameters is 1e-7), hence 1e-5."""
    e = case.e
    nat = [e.up(a) for a in case.A(None)]
    rot = e.ctx.bsgs_rotate_diagonals(nat, 8, e.gk)
    for j, (r, a) in enumerate(zip(rot, case.A(None))):
        e.same(nat[j], a)
        e.same(r, e.o.rotate(a, -(j // 8) * 8, e.gk_h) if j // 8 else a)
    got = e.ctx.matmul_diag_col_bsgs(rot, [e.up(x) for x in case.X], e.rk, e.gk, bs=8)
    dec = e.ctx.decrypt_decode(e.ctx.secret_key(e.sk), got, n_values=n, real=True)
    for i in range(p):
        assert np.max(np.abs(dec[i] - case.M @ case.x[i])) < 1e-5


# ------------------------------------------------------------------ 4. lower level
def test_lower_level(case):
    e = case.e
    X2 = [e.o.mod_switch(x) for x in case.X]
    A2 = [e.o.mod_switch(a) for a in case.A(8)]
    exp = bsgs_oracle(e, A2, X2, 8, e.rk_h, e.gk_h)
    got = run(e, A2, X2, 8)
    for g, c in zip(got, exp):
        assert g.info()[1] == 1
        e.same(g, c)


# ------------------------------------------------------------------ 5. full-size ring
def test_full_size_ring(orc, hecdna):
    """N = 2^15, {60, 40 x 9, 60}, default keys: n = 16, bs = 4, p = 2 (level 10: the 60-bit first prime's 128-bit
    middle product and the FP64-class 40-bit primes)."""
    e = Env(orc, hecdna, 1 << 15, [60] + [40] * 9 + [60], seed=99)
    rng = np.random.default_rng(5)
    D = rng.uniform(-1, 1, (16, 64))
    rows = hecdna.bsgs_diagonals(np.tile(D, (1, e.N // 2 // 64)), 4)
    A = [e.enc(r, seed=6500 + j) for j, r in enumerate(rows)]
    X = [e.enc(seed=6000 + i) for i in range(2)]
    exp = bsgs_oracle(e, A, X, 4, e.rk_h, e.gk_h)
    got = run(e, A, X, 4)
    for g, c in zip(got, exp):
        e.same(g, c)


# ------------------------------------------------------------------ 6. errors
def test_errors_leave_outputs_untouched(case, hecdna):
    e = case.e
    L = case.L
    diags = [e.up(a) for a in case.A(8)]
    cols = [e.up(x) for x in case.X]
    marks = [e.rand_ct(2, L, scale=3.0) for _ in range(p)]
    out = [e.up(m) for m in marks]

    def untouched():
        for g, m in zip(out, marks):
            e.same(g, m)

    def fails(match, ds=diags, cs=cols, gk=e.gk, o=out, bs=8):
        with pytest.raises(hecdna.InvalidArgument, match=match):
            e.ctx.matmul_diag_col_bsgs(ds, cs, e.rk, gk, bs=bs, out=o)
        untouched()

    only_step1 = e.ctx.galois_keys({k: v for k, v in e.gk_h.items() if k == e.o.elt_from_step(1)})
    fails("Galois key not present", gk=only_step1)  # baby step 2 has no key and no NAF chain
    no_giant = e.ctx.galois_keys({k: v for k, v in e.gk_h.items() if k != e.o.elt_from_step(16)})
    fails("Galois key not present", gk=no_giant)  # the giant step 16, after every baby step passed
    fails("encrypted size must be 2", cs=cols[:2] + [e.up(e.rand_ct(3, L))])
    fails("parameter mismatch", ds=diags[:5] + [e.up(e.o.mod_switch(case.A(8)[5]))] + diags[6:])
    fails("scale mismatch", ds=diags[:7] + [e.ctx.ciphertext(case.A(8)[7].data, 2.0**39)] + diags[8:])
    low_a = [e.up(e.enc(case.D[j], seed=6200 + j, level=1, scale=2.0**20)) for j in range(n)]
    low_x = [e.up(e.enc(seed=6100 + i, level=1, scale=2.0**20)) for i in range(p)]
    fails("end of modulus switching chain reached", ds=low_a, cs=low_x)
    fails("bs must be at most 512", ds=[diags[0]] * 513, bs=513)  # bs_eff = 513
    with pytest.raises(hecdna.InvalidArgument):
        e.ctx.matmul_diag_col_bsgs(diags, cols, e.rk, e.gk, bs=0, out=out)
    untouched()
    # an output that is another entry's input; one listed twice
    before = [c.download() for c in cols]
    for bad in ([cols[1], out[1], out[2]], [out[0], out[0], out[2]]):
        with pytest.raises(hecdna.InvalidArgument, match="alias"):
            e.ctx.matmul_diag_col_bsgs(diags, cols, e.rk, e.gk, bs=8, out=bad)
        untouched()
        for c, b in zip(cols, before):
            assert np.array_equal(c.download(), b)


# ------------------------------------------------------------------ 7. the cap
def test_cap_is_accepted(hecdna):
    """bs_eff = 512, the largest the entry takes, at the widest FP64-class primes (42 bits): n = bs = 512, p = 1 on
    uniform synthetic ciphertexts and keys equals matmul_diag_col on the same handles (G = 1: the definitions
    coincide).  This checks the plumbing at the cap; uniform residues do not reach the worst case of the exact FP64
    sums, which rests on the derivation at k_bsgs_inner_ct."""
    from prime_classes import FP_LIMIT
    m = hecdna.create_coeff_modulus(N11, [50, 42, 42, 50])
    assert m[1] < FP_LIMIT and m[2] < FP_LIMIT and m[1] > FP_LIMIT // 2
    ctx = hecdna.Context(N11, m)
    L, scale, cap = 3, 2.0**40, 512
    diags = [hecdna.Ciphertext(ctx).fill_uniform(2, L, scale, 30000 + j) for j in range(cap)]
    cols = [hecdna.Ciphertext(ctx).fill_uniform(2, L, scale, 900)]
    rk = ctx.relin_key(seed=5)
    gk = ctx.galois_keys(uniform_elts=ctx.default_galois_elts(), seed=6)
    ref = ctx.matmul_diag_col(diags, cols, rk, gk)
    got = ctx.matmul_diag_col_bsgs(diags, cols, rk, gk, bs=cap)
    same_words(got, words(ref))


# ------------------------------------------------------------------ 8. functional check
def plain_error(e, ct, want):
    """max |decode(decrypt(ct)) - want| over the first len(want) slots, by the oracle."""
    got = e.o.decode(e.o.decrypt(e.sk, ct), ct.scale)[: len(want)]
    return float(np.max(np.abs(got - want)))


def test_functional_against_plain_product(case):
    """The bs = 8 result decrypts to M @ x: its max-abs error over the n slots is at most ERR_RATIO_M times the
    error of the reference schedule (the oracle's matmul_diag_col on the natural diagonals, encrypted with the seeds
    of the BSGS ones) on the same matrix, vectors and keys."""
    e = case.e
    sk = e.ctx.secret_key(e.sk)
    got = run(e, case.A(8), case.X, 8)
    dec = e.ctx.decrypt_decode(sk, got, n_values=n, real=True)
    ref = e.o.matmul_diag_col(case.A(None), case.X, e.rk_h, e.gk_h)
    for i in range(p):
        want = case.M @ case.x[i]
        err = float(np.max(np.abs(dec[i] - want)))
        ref_err = plain_error(e, ref[i], want)
        print(f"vector {i}: bsgs error {err:.3e}, reference schedule's {ref_err:.3e}, ratio {err / ref_err:.3f}")
        assert err <= ERR_RATIO_M * ref_err
