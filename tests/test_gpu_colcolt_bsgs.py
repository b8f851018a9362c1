"""hec_matmul_col_colT_bsgs: the col x col^T product on the baby-step giant-step schedule, bit-exact against the
oracle's per-operation composition in the schedule's order (rotate by the baby and the negative giant steps, multiply,
add, relinearize, rescale, and for the natural form rotate by the positive giant steps), over both key shapes (a key
per planned step; the default power-of-two set, whose rotations are NAF chains) and both output forms, and its errors.
N = 2^11, [50, 36, 36, 50]: both prime classes at level 3.  n = 6 columns, p = 11 outputs: bs = 4 gives G = 3 with a
last group of 3, bs = 3 gives G = 4 with a last group of 2, and neither divides a 4-wide tile."""
import numpy as np
import pytest

import prime_classes as pc
from _helpers import col_vector
from test_gpu_bsgs_ctct import bsgs_oracle
from test_gpu_parity import Env

pytestmark = pytest.mark.gpu

N11, BITS11 = 1 << 11, [50, 36, 36, 50]
n, p = 6, 11
# test_functional_*: twice the worst ratio that tools/bsgs_error.py --form colcolT measured on the CPU over five seeds
# with the oracle alone.
# (a) composition error / matmul_col_colT error, max over the p outputs and all slots, bs = 4; per seed, form 0 then 1:
#     0.9520, 1.1745, 1.0000, 1.8790, 1.5588 and 0.9521, 1.1749, 1.0000, 1.8789, 1.5588
# (b) "form-1 output -> BSGS ct x ct matvec" error / "matmul_col_colT -> matmul_diag_col" error (d = 8, bs = 4, scale
#     2^36, two vectors): 1.8548, 0.5752, 0.5708, 0.8907, 1.0320
M_A = 2 * 1.8791
M_B = 2 * 1.8548
TILES = [(tb, tg) for tb in (1, 2, 4) for tg in (1, 2, 4)]
DEFAULTS = {"cct_jchunk": 0, "cct_tb": 4, "cct_tg": 2, "bsgs_order": 1, "poison": 0, "hoist": 1}


def cct_oracle(e, A, B, p_, bs, form, rk_h, gk_h):
    """The definition, from pinned oracle operations: acc_i = sum_j multiply(rotate(B[j], b), rotate(A[j], -g bs)),
    r_i = rescale(relinearize(acc_i)), out[i] = r_i (form 1) or rotate(r_i, g bs) (form 0), i = g bs + b."""
    eff = min(bs, p_)
    G = -(-p_ // eff)
    Bb = [[b] + [e.o.rotate(b, k, gk_h) for k in range(1, eff)] for b in B]
    Ag = [[a] + [e.o.rotate(a, -g * eff, gk_h) for g in range(1, G)] for a in A]
    outs = []
    for i in range(p_):
        g, b = divmod(i, eff)
        acc = None
        for j in range(len(A)):
            t = e.o.multiply(Bb[j][b], Ag[j][g])
            acc = t if acc is None else e.o.add(acc, t)
        r = e.o.rescale(e.o.relinearize(acc, rk_h))
        outs.append(e.o.rotate(r, g * eff, gk_h) if form == 0 and g else r)
    return outs


class Case:
    """The columns' slot vectors and their encryptions under one secret key (Env's seed fixes it, so every key set
    below belongs to the same key), left unchanged."""

    def __init__(self, orc, hecdna):
        self.orc, self.hec = orc, hecdna
        self.e = Env(orc, hecdna, N11, BITS11)  # default Galois keys
        e = self.e
        self.L = len(e.m) - 1
        rng = np.random.default_rng(2026)
        self.a = rng.uniform(-1, 1, (n, e.N // 2))
        self.b = rng.uniform(-1, 1, (n, e.N // 2))
        self.A = [e.enc(self.a[j], seed=3000 + j) for j in range(n)]
        self.B = [e.enc(self.b[j], seed=3100 + j) for j in range(n)]
        self._env, self._ref, self._words = {}, None, {}

    def env_with_step_keys(self, bs, form):
        """The same secret key (and relinearisation key) with a Galois key for exactly the planned steps."""
        if (bs, form) not in self._env:
            _, steps = self.hec.colcolT_bsgs_plan(p, bs, form)
            self._env[bs, form] = Env(self.orc, self.hec, N11, BITS11,
                                      elts=[self.e.o.elt_from_step(s) for s in steps])
        return self._env[bs, form]

    def reference(self):
        """Context.matmul_col_colT on the default keys: (info, words) per output, computed once"""
        if self._ref is None:
            self._ref = words(up_run_ref(self.e, self.A, self.B, p))
        return self._ref

    def default_words(self, bs, form):
        """the call at the default options on the default keys, computed once per (bs, form)"""
        if (bs, form) not in self._words:
            self._words[bs, form] = words(run(self.e, self.A, self.B, p, bs, form))
        return self._words[bs, form]


@pytest.fixture(scope="module")
def case(orc, hecdna):
    return Case(orc, hecdna)


def run(e, A, B, p_, bs, form, out=None, gk=None, rk=None):
    return e.ctx.matmul_col_colT_bsgs([e.up(a) for a in A], [e.up(b) for b in B], p_, rk or e.rk, gk or e.gk, bs=bs,
                                      bsgs_form=form, out=out)


def up_run_ref(e, A, B, p_):
    return e.ctx.matmul_col_colT([e.up(a) for a in A], [e.up(b) for b in B], p_, e.rk, e.gk)


def words(cts):
    return [(g.info(), g.download()) for g in cts]


def same_words(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.info() == w[0] and np.array_equal(g.download(), w[1])


# ------------------------------------------------------------------ 1. bit-exact against the composition
@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("keys", ["per_step", "default"])
@pytest.mark.parametrize("bs", [4, 3])
def test_bitexact_against_oracle_composition(case, bs, keys, form):
    """per_step: every rotation is one key switch and each trie is one hoisted node.  default: NAF chains, negative
    steps included, so both tries are deeper than 1 and form 0's output rotations are chains."""
    e = case.env_with_step_keys(bs, form) if keys == "per_step" else case.e
    exp = cct_oracle(e, case.A, case.B, p, bs, form, e.rk_h, e.gk_h)
    got = run(e, case.A, case.B, p, bs, form)
    assert len(got) == p
    for g, c in zip(got, exp):
        assert g.info()[1] == case.L - 1
        e.same(g, c)


# ------------------------------------------------------------------ 2. the coinciding block
@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("bs", [11, 16])
def test_whole_block_equals_col_colT(case, bs, form):
    """bs_eff = p: one giant group, no giant rotation, and the two definitions coincide word for word in both forms."""
    same_words(run(case.e, case.A, case.B, p, bs, form), case.reference())


# ------------------------------------------------------------------ 3. degenerate and default block sizes
@pytest.mark.parametrize("form", [0, 1])
def test_block_size_one_is_all_giants(case, form):
    e = case.e
    exp = cct_oracle(e, case.A, case.B, p, 1, form, e.rk_h, e.gk_h)
    for g, c in zip(run(e, case.A, case.B, p, 1, form), exp):
        e.same(g, c)


def test_default_block_size(case, hecdna):
    """bs=None is the smallest power of two >= sqrt(11) = 4."""
    assert hecdna.colcolT_bsgs_plan(p)[0] == 4
    for form in (0, 1):
        same_words(run(case.e, case.A, case.B, p, None, form), case.default_words(4, form))


# ------------------------------------------------------------------ 4. pass, tile and poison independence
def with_options(case, opts, bs, form):
    e = case.e
    try:
        for k, v in opts.items():
            e.ctx.set_option(k, v)
        return run(e, case.A, case.B, p, bs, form)
    finally:
        for k, v in DEFAULTS.items():
            e.ctx.set_option(k, v)


@pytest.mark.parametrize("jchunk", [1, 4, 5])
def test_pass_size_independence(case, jchunk):
    """passes of 1, of 4 + 2 and of 5 + 1 columns: every pass after the first reads the stored sums and adds"""
    same_words(with_options(case, {"cct_jchunk": jchunk}, 4, 0), case.default_words(4, 0))


@pytest.mark.parametrize("bs", [4, 3])
@pytest.mark.parametrize("tb,tg", TILES)
def test_kernel_tiles_compute_the_same_words(case, tb, tg, bs):
    """Every tile of k_colcolt_inner gives the default's bits (bs = 4: G = 3 and a last group of 3; bs = 3: G = 4 and a
    last group of 2: partial edge tiles for every width above 1)."""
    same_words(with_options(case, {"cct_tb": tb, "cct_tg": tg}, bs, 1), case.default_words(bs, 1))


@pytest.mark.parametrize("order", [0, 1])
def test_grid_order_and_chunked_tiles(case, order):
    same_words(with_options(case, {"bsgs_order": order, "cct_tb": 2, "cct_tg": 2, "cct_jchunk": 4}, 3, 0),
               case.default_words(3, 0))


@pytest.mark.parametrize("name,value", [("poison", 1), ("hoist", 0)])
def test_poison_and_hoist_independence(case, name, value):
    for form in (0, 1):
        same_words(with_options(case, {name: value}, 4, form), case.default_words(4, form))


@pytest.mark.parametrize("name,value", [("cct_tb", 0), ("cct_tb", 3), ("cct_tg", 8), ("cct_jchunk", 513),
                                        ("cct_jchunk", -1)])
def test_option_outside_its_set_is_refused(case, name, value):
    with pytest.raises(case.hec.InvalidArgument):
        case.e.ctx.set_option(name, value)


# ------------------------------------------------------------------ 5. the FP64 bound at its limit
@pytest.fixture(scope="module")
def top(orc, hecdna):
    return Env(orc, hecdna, N11, pc.CHAINS["TOP"])


BOUND_PAIRS = {
    # every product's centred residue is -(q - 1) / 2: all three sums run one-signed to (q - 1) J / 2, the middle to
    # (q - 1) J, which is 2^51 at J = 512 and the 42-bit primes
    "lo": [(("half_lo", "half_lo"), ("qm1", "qm1"))],
    "hi": [(("half_hi", "half_hi"), ("qm1", "qm1"))],  # +(q - 1) / 2 likewise
    "mixed": [(("half_hi", "half_lo"), ("qm1", "alt")), (("alt", "qm1"), ("half_lo", "half_hi")),
              (("qm1", "half_hi"), ("half_hi", "alt"))],
}


@pytest.mark.parametrize("cols", [512, 515])
@pytest.mark.parametrize("pair", sorted(BOUND_PAIRS))
def test_inner_sum_at_its_bound(top, pair, cols):
    """k_colcolt_inner's stated worst case through the public API at the widest FP64-class primes: p = 1 (G = 1: no
    rotation touches the crafted words, and the definitions coincide), 512 columns in one launch at the cap, and 515:
    a second pass of 3 added to the stored sums.  Word for word Context.matmul_col_colT, whose kernel is integer
    only."""
    e, sc = top, pc.SCALE["TOP"]
    def ct(names):
        return e.up(pc.pattern_ct(e.orc, e.m, 2, 3, e.N, list(names), sc))

    hs = [(ct(bn), ct(an)) for bn, an in BOUND_PAIRS[pair]]
    B = [hs[j % len(hs)][0] for j in range(cols)]
    A = [hs[j % len(hs)][1] for j in range(cols)]
    ref = e.ctx.matmul_col_colT(A, B, 1, e.rk, e.gk)
    got = e.ctx.matmul_col_colT_bsgs(A, B, 1, e.rk, e.gk)
    same_words(got, words(ref))


# ------------------------------------------------------------------ 6. errors
@pytest.fixture(scope="module")
def err_env(case):
    """keys for exactly the planned steps of (p, bs = 4, form 0): 1, 2, 3, -4, -8, 4, 8"""
    return case.env_with_step_keys(4, 0)


class Errs:
    def __init__(self, case, e):
        self.case, self.e, self.hec = case, e, case.hec
        self.A = [e.up(a) for a in case.A]
        self.B = [e.up(b) for b in case.B]
        self.marks = [e.rand_ct(2, case.L, scale=3.0) for _ in range(p)]
        self.out = [e.up(m) for m in self.marks]

    def untouched(self):
        for g, m in zip(self.out, self.marks):
            self.e.same(g, m)

    def fails(self, match, A=None, B=None, gk=None, rk=None, out=None, form=0, bs=4, exc=None):
        e = self.e
        with pytest.raises(exc or self.hec.InvalidArgument, match=match):
            e.ctx.matmul_col_colT_bsgs(A or self.A, B or self.B, p, rk or e.rk, gk or e.gk, bs=bs, bsgs_form=form,
                                       out=out or self.out)
        self.untouched()

    def keys_without(self, step):
        e = self.e
        return e.ctx.galois_keys({k: v for k, v in e.gk_h.items() if k != e.o.elt_from_step(step)})


@pytest.fixture(scope="module")
def errs(case, err_env):
    return Errs(case, err_env)


def test_missing_negative_giant_key(errs):
    """-8 has no key and its NAF chain is the step itself; every baby and -4 passed before it"""
    for form in (0, 1):
        errs.fails("Galois key not present", gk=errs.keys_without(-8), form=form)


def test_missing_positive_giant_key_only_matters_in_natural_form(errs):
    e = errs.e
    gk = errs.keys_without(8)
    errs.fails("Galois key not present", gk=gk, form=0)
    got = e.ctx.matmul_col_colT_bsgs(errs.A, errs.B, p, e.rk, gk, bs=4, bsgs_form=1)
    same_words(got, words(e.ctx.matmul_col_colT_bsgs(errs.A, errs.B, p, e.rk, e.gk, bs=4, bsgs_form=1)))
    errs.untouched()


def test_input_errors(errs, case):
    e, L = errs.e, case.L
    errs.fails("encrypted size must be 2", B=errs.B[:2] + [e.up(e.rand_ct(3, L))] + errs.B[3:])
    errs.fails("encrypted size must be 2", A=errs.A[:5] + [e.up(e.rand_ct(3, L))])
    errs.fails("parameter mismatch", A=errs.A[:2] + [e.up(e.o.mod_switch(case.A[2]))] + errs.A[3:])
    errs.fails("scale mismatch", A=errs.A[:3] + [e.ctx.ciphertext(case.A[3].data, 2.0**39)] + errs.A[4:])
    low_a = [e.up(e.enc(seed=6200 + j, level=1, scale=2.0**20)) for j in range(n)]
    low_b = [e.up(e.enc(seed=6300 + j, level=1, scale=2.0**20)) for j in range(n)]
    errs.fails("end of modulus switching chain reached", A=low_a, B=low_b)
    errs.fails("relin_keys is not valid", rk=case.e.rk)  # another context's
    errs.fails("galois_keys is not valid", gk=case.e.gk)
    errs.fails("form", form=2)
    with pytest.raises(errs.hec.InvalidArgument):
        e.ctx.matmul_col_colT_bsgs(errs.A, errs.B, p, e.rk, e.gk, bs=0, out=errs.out)
    errs.untouched()


def test_aliased_outputs(errs):
    e = errs.e
    before = [c.download() for c in errs.A + errs.B]
    for bad in ([errs.A[1]] + errs.out[1:], errs.out[:4] + [errs.B[0]] + errs.out[5:],
                [errs.out[0], errs.out[0]] + errs.out[2:]):
        for form in (0, 1):
            errs.fails("alias", out=bad, form=form)
    for c, w in zip(errs.A + errs.B, before):
        assert np.array_equal(c.download(), w)


def test_check_order(errs, case):
    """the order the header fixes: the scales before the Galois keys, the keys before the aliasing rule"""
    e = errs.e
    no_key = errs.keys_without(-8)
    bad_scale = errs.A[:3] + [e.ctx.ciphertext(case.A[3].data, 2.0**39)] + errs.A[4:]
    errs.fails("scale mismatch", A=bad_scale, gk=no_key)
    errs.fails("Galois key not present", gk=no_key, out=[errs.A[1]] + errs.out[1:])
    errs.fails("form", form=2, gk=case.e.gk)  # the form before the key set's context


# ------------------------------------------------------------------ 7. functional check
def max_error(e, cts, want):
    dec = e.ctx.decrypt_decode(e.ctx.secret_key(e.sk), cts, n_values=e.N // 2, real=True)
    return max(float(np.max(np.abs(dec[i] - want[i]))) for i in range(len(want)))


def test_functional_against_plain_product(case):
    """Form 0 decrypts to slot vectors sum_j roll(b[j], -i) a[j]; form 1's out[i] to the same vector rolled right by
    (i // bs_eff) bs_eff slots.  The max-abs error over the p outputs and all slots is at most M_A times that of
    Context.matmul_col_colT on the same inputs and keys."""
    e = case.e
    want = [sum(np.roll(case.b[j], -i) * case.a[j] for j in range(n)) for i in range(p)]
    ref_err = max_error(e, up_run_ref(e, case.A, case.B, p), want)
    for form in (0, 1):
        got = run(e, case.A, case.B, p, 4, form)
        w = want if form == 0 else [np.roll(want[i], (i // 4) * 4) for i in range(p)]
        err = max_error(e, got, w)
        print(f"form {form}: bsgs error {err:.3e}, matmul_col_colT's {ref_err:.3e}, ratio {err / ref_err:.3f}")
        assert err <= M_A * ref_err


# ------------------------------------------------------------------ 8. the chain the form exists for
def test_bsgs_form_feeds_the_bsgs_matvec(case):
    """M M^T x with no rotation between the two products: the columns of a d = 8 matrix as A = B give the d diagonals of
    M M^T, in BSGS form for bs = 4, and matmul_diag_col_bsgs takes them as they are.  Bit-exact against the two
    definitions chained; the decrypted product errs by at most M_B times matmul_col_colT -> matmul_diag_col."""
    e = case.e
    d, bs, sc = 8, 4, 2.0**36
    rng = np.random.default_rng(88)
    M = rng.uniform(-1, 1, (d, d))
    xs = rng.uniform(-1, 1, (2, d))
    cols = [e.enc(col_vector(M[:, j], e.N // 2), scale=sc, seed=8000 + j) for j in range(d)]
    X = [e.enc(col_vector(x, e.N // 2), level=case.L - 1, scale=sc, seed=8100 + i) for i, x in enumerate(xs)]
    gcols = [e.up(c) for c in cols]
    gX = [e.up(x) for x in X]
    D = e.ctx.matmul_col_colT_bsgs(gcols, gcols, d, e.rk, e.gk, bs=bs, bsgs_form=True)
    got = e.ctx.matmul_diag_col_bsgs(D, gX, e.rk, e.gk, bs=bs)
    exp = bsgs_oracle(e, cct_oracle(e, cols, cols, d, bs, 1, e.rk_h, e.gk_h), X, bs, e.rk_h, e.gk_h)
    for g, c in zip(got, exp):
        e.same(g, c)
    ref = e.ctx.matmul_diag_col(e.ctx.matmul_col_colT(gcols, gcols, d, e.rk, e.gk), gX, e.rk, e.gk)
    sk = e.ctx.secret_key(e.sk)
    dec = e.ctx.decrypt_decode(sk, got, n_values=d, real=True)
    dec_ref = e.ctx.decrypt_decode(sk, ref, n_values=d, real=True)
    want = [M @ M.T @ x for x in xs]
    err = max(float(np.max(np.abs(dec[i] - want[i]))) for i in range(2))
    ref_err = max(float(np.max(np.abs(dec_ref[i] - want[i]))) for i in range(2))
    print(f"chain: bsgs error {err:.3e}, reference chain's {ref_err:.3e}, ratio {err / ref_err:.3f}")
    assert err <= M_B * ref_err
