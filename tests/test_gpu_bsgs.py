"""hec_matmul_diagpt_col_bsgs: the ct x pt matvec on the baby-step giant-step schedule, bit-exact against the
oracle's per-operation composition in the schedule's order (rotate, multiply_plain, add, rescale), over both key
shapes (a key per planned step; the default power-of-two set, whose rotations are NAF chains), and its errors.
N = 2^11, [50, 36, 36, 50]: both prime classes at level 3.  n = 24, p = 3: the batch does not divide the kernel's BG."""
import numpy as np
import pytest

from _helpers import col_vector, diag_vectors
from test_gpu_parity import Env

pytestmark = pytest.mark.gpu

N11, BITS11 = 1 << 11, [50, 36, 36, 50]
n, p = 24, 3
PSCALE = 2.0**40
# test_functional_against_plain_product: twice the worst ratio (BSGS error / reference schedule's error) that
# tools/bsgs_error.py measured on the CPU over five seeds with the oracle alone: 0.468, 0.291, 0.188, 0.551, 0.811
# 
ERR_RATIO_M = 2 * 0.8111


def bsgs_oracle(e, P, X, bs, gk_h, pscale=PSCALE):
    """The definition, from pinned oracle operations: inner_g = sum_i multiply_plain(rotate(x, i), P'[g bs + i]),
    out = rescale(inner_0 + sum_{g >= 1} rotate(inner_g, g bs))."""
    eff = min(bs, len(P))
    G = -(-len(P) // eff)
    outs = []
    for x in X:
        rots = [x] + [e.o.rotate(x, i, gk_h) for i in range(1, eff)]
        acc = None
        for g in range(G):
            inner = None
            for i in range(eff):
                if g * eff + i >= len(P):
                    break
                t = e.o.multiply_plain(rots[i], P[g * eff + i], pscale)
                inner = t if inner is None else e.o.add(inner, t)
            r = inner if g == 0 else e.o.rotate(inner, g * eff, gk_h)
            acc = r if acc is None else e.o.add(acc, r)
        outs.append(e.o.rescale(acc))
    return outs


class Case:
    """One matrix, p input vectors and their encryptions under one secret key (Env's seed fixes it, so every key
    set below belongs to the same key); the BSGS-form plaintexts per block size, encoded once and left unchanged."""

    def __init__(self, orc, hecdna):
        self.orc, self.hec = orc, hecdna
        self.e = Env(orc, hecdna, N11, BITS11)  # default Galois keys
        e = self.e
        self.L = len(e.m) - 1
        rng = np.random.default_rng(2024)
        self.M = rng.uniform(-1, 1, (n, n))
        self.x = rng.uniform(-1, 1, (p, n))
        self.D = np.stack(diag_vectors(self.M, e.N // 2))
        self.X = [e.enc(col_vector(self.x[i], e.N // 2), seed=4000 + i) for i in range(p)]
        self._P, self._env = {}, {}

    def P(self, bs, level=None):
        key = (bs, level or self.L)
        if key not in self._P:
            rows = self.hec.bsgs_diagonals(self.D, bs)
            self._P[key] = [self.e.o.encode(r, PSCALE, key[1]) for r in rows]
        return self._P[key]

    def env_with_step_keys(self, bs):
        """The same secret key with a Galois key for exactly the planned steps of (n, bs)."""
        if bs not in self._env:
            _, steps = self.hec.bsgs_plan(n, bs)
            self._env[bs] = Env(self.orc, self.hec, N11, BITS11, elts=[self.e.o.elt_from_step(s) for s in steps])
        return self._env[bs]


@pytest.fixture(scope="module")
def case(orc, hecdna):
    return Case(orc, hecdna)


def run(e, P, X, bs, out=None):
    return e.ctx.matmul_diagpt_col_bsgs([e.ctx.plaintext(q, PSCALE) for q in P], [e.up(x) for x in X], e.gk, bs=bs,
                                        out=out)


# ------------------------------------------------------------------ 1. bit-exact against the composition
@pytest.mark.parametrize("bs", [5, 8])
@pytest.mark.parametrize("keys", ["per_step", "default"])
def test_bitexact_against_oracle_composition(case, bs, keys):
    """per_step: the root of the baby trie has bs - 1 children (4 and 7: more than one sibling group of the hoisted
    MAC) and every giant is one key switch.  default: NAF tries deeper than 1 and multi-element giant rotations.
    bs = 5 leaves a partial last giant group (24 = 4 x 5 + 4) and G = 5 a partial tile of giants; bs = 8 has G = 3."""
    e = case.env_with_step_keys(bs) if keys == "per_step" else case.e
    exp = bsgs_oracle(e, case.P(bs), case.X, bs, e.gk_h)
    got = run(e, case.P(bs), case.X, bs)
    for g, c in zip(got, exp):
        e.same(g, c)


# ------------------------------------------------------------------ 2. degenerate and coinciding block sizes
@pytest.mark.parametrize("bs", [24, 32])
def test_whole_matrix_block_equals_reference_schedule(case, bs):
    """bs_eff = n: no giant step, P' = P, and the two definitions coincide word for word."""
    e = case.e
    pts = [e.ctx.plaintext(q, PSCALE) for q in case.P(bs)]
    cols = [e.up(x) for x in case.X]
    ref = e.ctx.matmul_diagpt_col(pts, cols, e.gk)
    got = e.ctx.matmul_diagpt_col_bsgs(pts, cols, e.gk, bs=bs)
    for g, r in zip(got, ref):
        assert g.info() == r.info()
        assert np.array_equal(g.download(), r.download())


def test_block_size_one_is_all_giants(case):
    e = case.e
    exp = bsgs_oracle(e, case.P(1), case.X, 1, e.gk_h)
    for g, c in zip(run(e, case.P(1), case.X, 1), exp):
        e.same(g, c)


def test_default_block_size(case, hecdna):
    """bs=None is the smallest power of two >= sqrt(24) = 8."""
    e = case.e
    assert hecdna.bsgs_plan(n)[0] == 8
    a = run(e, case.P(8), case.X, None)
    b = run(e, case.P(8), case.X, 8)
    for g, r in zip(a, b):
        assert g.info() == r.info() and np.array_equal(g.download(), r.download())


# ------------------------------------------------------------------ 3. batch independence
def test_batch_and_chunk_independence(case):
    e = case.e
    whole = [(g.info(), g.download()) for g in run(e, case.P(8), case.X, 8)]
    for i in range(p):
        g = run(e, case.P(8), [case.X[i]], 8)[0]
        assert g.info() == whole[i][0] and np.array_equal(g.download(), whole[i][1])
    e.ctx.set_option("bsgs_chunk", 2)  # passes of 2 and 1 vectors
    try:
        chunked = run(e, case.P(8), case.X, 8)
    finally:
        e.ctx.set_option("bsgs_chunk", 0)
    for g, w in zip(chunked, whole):
        assert g.info() == w[0] and np.array_equal(g.download(), w[1])
    with pytest.raises(case.hec.InvalidArgument):
        e.ctx.set_option("bsgs_chunk", -1)


@pytest.mark.parametrize("bg,gg,order", [(1, 2, 0), (4, 4, 1), (2, 4, 0), (4, 8, 1), (1, 16, 1), (2, 16, 0)])
def test_kernel_tiles_compute_the_same_words(case, bg, gg, order):
    """Every tile of k_bsgs_inner and both grid orders give the default's bits (G = 5 at bs = 5: partial tiles for
    every gg; p = 3: a partial batch group for bg = 2 and 4)."""
    e = case.e
    whole = [(g.info(), g.download()) for g in run(e, case.P(5), case.X, 5)]
    opts = {"bsgs_bg": bg, "bsgs_gg": gg, "bsgs_order": order}
    try:
        for k, v in opts.items():
            e.ctx.set_option(k, v)
        got = run(e, case.P(5), case.X, 5)
    finally:
        for k, v in {"bsgs_bg": 2, "bsgs_gg": 8, "bsgs_order": 1}.items():
            e.ctx.set_option(k, v)
    for g, w in zip(got, whole):
        assert g.info() == w[0] and np.array_equal(g.download(), w[1])
    with pytest.raises(case.hec.InvalidArgument):
        e.ctx.set_option("bsgs_gg", 3)


def test_output_may_be_its_own_input(case):
    e = case.e
    exp = run(e, case.P(8), case.X, 8)
    cols = [e.up(x) for x in case.X]
    got = e.ctx.matmul_diagpt_col_bsgs([e.ctx.plaintext(q, PSCALE) for q in case.P(8)], cols, e.gk, bs=8, out=cols)
    for g, r in zip(got, exp):
        assert g.info() == r.info() and np.array_equal(g.download(), r.download())


# ------------------------------------------------------------------ 4. lower level
def test_lower_level(case):
    e = case.e
    X2 = [e.o.mod_switch(x) for x in case.X]
    P2 = case.P(8, level=2)
    exp = bsgs_oracle(e, P2, X2, 8, e.gk_h)
    got = run(e, P2, X2, 8)
    for g, c in zip(got, exp):
        assert g.info()[1] == 1
        e.same(g, c)


# ------------------------------------------------------------------ 5. full-size ring
def test_full_size_ring(orc, hecdna):
    """N = 2^15, {60, 40 x 9, 60}, default keys: n = 16, bs = 4, p = 2 (level 10, the 60-bit first prime and the
    FP64-class 40-bit primes)."""
    e = Env(orc, hecdna, 1 << 15, [60] + [40] * 9 + [60], seed=99)
    L = len(e.m) - 1
    rng = np.random.default_rng(5)
    D = rng.uniform(-1, 1, (16, 64))
    rows = hecdna.bsgs_diagonals(np.tile(D, (1, e.N // 2 // 64)), 4)
    P = [e.o.encode(r, PSCALE, L) for r in rows]
    X = [e.enc(seed=6000 + i) for i in range(2)]
    exp = bsgs_oracle(e, P, X, 4, e.gk_h)
    got = run(e, P, X, 4)
    for g, c in zip(got, exp):
        e.same(g, c)


# ------------------------------------------------------------------ 6. errors
def test_errors_leave_outputs_untouched(case, hecdna):
    e = case.e
    L = case.L
    pts = [e.ctx.plaintext(q, PSCALE) for q in case.P(8)]
    cols = [e.up(x) for x in case.X]
    marks = [e.rand_ct(2, L, scale=3.0) for _ in range(p)]
    out = [e.up(m) for m in marks]

    def untouched():
        for g, m in zip(out, marks):
            e.same(g, m)

    def fails(match, pdiags=pts, cs=cols, gk=e.gk, o=out):
        with pytest.raises(hecdna.InvalidArgument, match=match):
            e.ctx.matmul_diagpt_col_bsgs(pdiags, cs, gk, bs=8, out=o)
        untouched()

    only_step1 = e.ctx.galois_keys({k: v for k, v in e.gk_h.items() if k == e.o.elt_from_step(1)})
    fails("Galois key not present", gk=only_step1)  # baby step 2 has no key and no NAF chain
    no_giant = e.ctx.galois_keys({k: v for k, v in e.gk_h.items() if k != e.o.elt_from_step(16)})
    fails("Galois key not present", gk=no_giant)  # the giant step 16, after every baby step passed
    fails("encrypted size must be 2", cs=cols[:2] + [e.up(e.rand_ct(3, L))])
    other_level = e.ctx.plaintext(e.o.encode(case.D[0], PSCALE, L - 1), PSCALE)
    fails("parameter mismatch", pdiags=pts[:5] + [other_level] + pts[6:])
    other_scale = e.ctx.plaintext(case.P(8)[7], 2.0**39)
    fails("scale mismatch", pdiags=pts[:7] + [other_scale] + pts[8:])
    low_p = [e.ctx.plaintext(e.o.encode(case.D[j], 2.0**20, 1), 2.0**20) for j in range(n)]
    low_x = [e.up(e.enc(seed=6100 + i, level=1, scale=2.0**20)) for i in range(p)]
    fails("end of modulus switching chain reached", pdiags=low_p, cs=low_x)
    with pytest.raises(hecdna.InvalidArgument):
        e.ctx.matmul_diagpt_col_bsgs(pts, cols, e.gk, bs=0, out=out)
    untouched()
    # an output that is another entry's input; one listed twice
    before = [c.download() for c in cols]
    for bad in ([cols[1], out[1], out[2]], [out[0], out[0], out[2]]):
        with pytest.raises(hecdna.InvalidArgument, match="alias"):
            e.ctx.matmul_diagpt_col_bsgs(pts, cols, e.gk, bs=8, out=bad)
        untouched()
        for c, b in zip(cols, before):
            assert np.array_equal(c.download(), b)


# ------------------------------------------------------------------ 7. functional check
def plain_error(e, ct, want):
    """max |decode(decrypt(ct)) - want| over the first len(want) slots, by the oracle."""
    got = e.o.decode(e.o.decrypt(e.sk, ct), ct.scale)[: len(want)]
    return float(np.max(np.abs(got - want)))


def test_functional_against_plain_product(case):
    """The bs = 8 result decrypts to M @ x: its max-abs error over the n slots is at most ERR_RATIO_M times the
    error of the reference schedule (the oracle's matmul_diagpt_col_set) on the same inputs."""
    e = case.e
    sk = e.ctx.secret_key(e.sk)
    got = run(e, case.P(8), case.X, 8)
    dec = e.ctx.decrypt_decode(sk, got, n_values=n, real=True)
    Pref = [e.o.encode(d, PSCALE, case.L) for d in case.D]
    ref = e.o.matmul_diagpt_col_set(Pref, PSCALE, list(range(n)), case.X, e.gk_h)
    for i in range(p):
        want = case.M @ case.x[i]
        err = float(np.max(np.abs(dec[i] - want)))
        ref_err = plain_error(e, ref[i], want)
        print(f"vector {i}: bsgs error {err:.3e}, reference schedule's {ref_err:.3e}, ratio {err / ref_err:.3f}")
        assert err <= ERR_RATIO_M * ref_err
