"""The inputs of test_gpu_prime_classes.py checked on the CPU with the oracle alone: each chain's primes fall in the
arithmetic classes the GPU tests are written for, the invariant ciphertext and the half-residue plaintexts give the
sums the FP64 kernels bound, and an exact-integer model of the FP64 forward transform stays inside the bound the
kernels state for it (hec_device.h: |X| < 10 q < 2^45.4)."""
import numpy as np
import pytest

import prime_classes as pc


@pytest.fixture(scope="module")
def chains(orc):
    return {k: orc.Oracle.create_coeff_modulus(pc.N11, bits) for k, bits in pc.CHAINS.items()}


def fp(q):
    return q < pc.FP_LIMIT


# ------------------------------------------------------------------ the classes each chain is named for
def test_widths_are_just_under_the_power_of_two(orc):
    """The prime search returns primes just under 2^bits: a 42-bit prime is at the top of the FP64 class and a 43-bit
    one at the bottom of the integer class.  The values SEAL's search gives at these sizes."""
    m = orc.Oracle.create_coeff_modulus
    assert m(pc.N11, [42, 42]) == [0x3ffffff9001, 0x3ffffffa001]
    assert m(pc.N11, [43]) == [0x7fffffdd001]
    assert m(pc.N11, [30]) == [0x3fff4001]
    for logN in (10, 13, 16):
        q = m(1 << logN, pc.NTT_BITS)
        assert [x.bit_length() for x in q] == pc.NTT_BITS
        assert [fp(x) for x in q] == [False, True, True, False, True, False]
        assert q[1] > 0.999 * 2**42  # the slack of every FP64 bound is smallest here


def test_top(chains):
    q = chains["TOP"]
    assert [fp(x) for x in q] == [False, True, True, False]
    assert all(x > pc.FP_LIMIT - (1 << 20) for x in q[1:3])  # within 2^-22 of the class limit
    assert q[1] != q[2]


def test_edge(chains):
    q = chains["EDGE"]
    assert [fp(x) for x in q] == [False, True, False, False]
    assert q[2].bit_length() == 43 and q[1].bit_length() == 42
    assert q[1] < q[2] <= 2 * q[1]        # digit 2 at target 1: one conditional subtraction; digit 1 at target 2: none
    assert q[0] > 2 * q[1] and q[0] > 2 * q[2]  # the 60-bit digit: the split reduction (FP64) and Barrett (integer)
    assert q[1] > pc.C30_LIMIT


def test_int(chains):
    q = chains["INT"]
    assert not any(fp(x) for x in q)
    assert q[1].bit_length() == 43
    assert q[2] > 2 * q[1] and q[0] > 2 * q[1]  # red == 2 at the 43-bit target from digit 2 as well as from q_0
    assert q[1] <= q[0] and q[1] <= q[2] and q[0] <= 2 * q[2] and q[2] <= 2 * q[0]  # red 0 and 1 elsewhere


def test_allfp(chains):
    q = chains["ALLFP"]
    assert all(fp(x) for x in q)           # q_0 and the special prime included
    assert q[1] <= pc.C30_LIMIT < q[2]     # c30 == 0 for q_1 only
    assert q[0] > 2**11 * q[1]             # an FP64-class digit 2^12 wider than an FP64-class target
    assert q[0] > 2 * q[2] and q[2] > 2 * q[1] and q[3] > 2 * q[1] and q[3] > 2 * q[2]
    assert q[0] != q[3] and q[0] <= 2 * q[3] and q[3] <= 2 * q[0]


def test_long(chains):
    q = chains["LONG"]
    assert len(q) == 12 and len(set(q)) == 12
    assert [fp(x) for x in q] == [False] + [True] * 10 + [False]
    assert all(x.bit_length() == 42 for x in q[1:11])


# ------------------------------------------------------------------ the sums at their bound
@pytest.fixture(scope="module")
def top(orc, chains):
    m = chains["TOP"]
    o = orc.Oracle(pc.N11, m)
    sk = o.secret_key(7)
    gk = o.galois_keys(sk, o.default_galois_elts(), 9)
    return m, o, gk


def test_invariant_ciphertext(orc, top):
    m, o, gk = top
    inv = pc.invariant_ct(orc, m, 3, pc.N11, 2.0**40)
    for step in (1, 683):
        r = o.rotate(inv, step, gk)
        assert np.array_equal(r.data, inv.data) and r.scale == inv.scale


@pytest.mark.parametrize("name,sign", [("half_lo", 1), ("half_hi", -1)])
def test_sums_reach_the_bound(orc, top, name, sign):
    """Every multiply_plain product of the invariant ciphertext with the half-residue plaintext is that residue, whose
    centred representative (what fp_mulmod returns) is +-(q - 1) / 2: bs of them sum to +-bs (q - 1) / 2 as an integer,
    at least 0.49 of 2^52 for bs = 1024 at a 42-bit prime, and the oracle's own 1024-term sum is that value mod q."""
    m, o, gk = top
    bs = 1024
    inv = pc.invariant_ct(orc, m, 3, pc.N11, 2.0**40)
    pt = pc.pattern_poly(m, 3, pc.N11, name)
    prod = o.multiply_plain(o.rotate(inv, 5, gk), pt, 2.0**40)
    acc = None
    for _ in range(bs):
        acc = prod if acc is None else o.add(acc, prod)
    for k in (1, 2):
        q = m[k]
        assert np.all(prod.data[0, k] == pt[k, 0]) and np.all(prod.data[1, k] == 0)
        c = pc.centred(pt[k, 0], q)
        assert c == sign * (q - 1) // 2
        total = bs * c
        assert abs(total) >= 0.49 * 2**52 and abs(total) < 2**52   # inside fp_canon's domain, and at its edge
        assert np.all(acc.data[0, k] == total % q)
        # the deferred tensor sum of matmul_diag_col at TB_MAX = 12 terms against its stated 1.6 q T
        assert 12 * abs(c) >= 0.3 * 1.6 * q * 12


# ------------------------------------------------------------------ the forward transform's magnitudes
@pytest.mark.parametrize("logN", [10, 13, 16])
def test_forward_magnitude_model(orc, logN):
    """The FP64 forward transform in exact integers (prime_classes.fp_forward_model) at the 42-, 41- and 30-bit primes:
    its canonical output is the oracle's, every value stays below the stated 10 q and below 2^45.4, and every fp_mulmod
    operand too.  A start of 2 q - 1 everywhere is the top of the range the fan-outs may hand over (|x| < 2 q).  At
    logN = 16 (the only size with 16 stages) every width runs on fewer patterns."""
    N = 1 << logN
    m = orc.Oracle.create_coeff_modulus(N, pc.NTT_BITS)
    o = orc.Oracle(N, m)
    rng = np.random.default_rng(logN)
    for i in (1, 2, 4):
        q = m[i]
        tw = pc.seal_twiddles(o, i, N)
        ins = pc.transform_inputs(o, i, N)
        names = ["qm1", "alt", "inv_of_alt"] if logN == 16 else list(ins)
        cases = [(n, ins[n], True) for n in names]
        cases.append(("random", rng.integers(0, q, N, dtype=np.uint64), True))
        cases.append(("2q-1 (fan-out range)", np.full(N, 2 * q - 1, dtype=object), False))
        for name, x, canonical_in in cases:
            out, peak, peak_y = pc.fp_forward_model(x, tw, q)
            if canonical_in:
                assert np.array_equal(out, o.ntt_fwd(i, x)), name
            frac = peak / q
            print(f"logN {logN} q {q.bit_length()} bits {name:>22}: max |X| / q = {frac:.3f}, "
                  f"max |Y| / q = {peak_y / q:.3f}, log2 max |X| = {np.log2(max(peak, 1)):.2f}")
            assert peak < 10 * q and peak_y < 10 * q, name
            assert peak < 2**45.4, name


def test_forward_model_unreduced_wide_digit(orc):
    """ALLFP's hoisted mod-up hands a 42-bit FP64-class digit to the 30- and 36-bit FP64 targets without a reduction
    (FanModUp::xf16's sdbl path): the start is then up to q_0 - 1 = 2^12 q_1, far above 2 q_1, and what keeps
    fp_mulmod exact is its absolute operand bound |y| < 2^45.4.  The model on words of q_0 - 1, on alternating 0 and
    q_0 - 1 and on uniform words below q_0: the oracle's transform of the reduced words, every value below 2^45.4."""
    N = pc.N11
    m = orc.Oracle.create_coeff_modulus(N, pc.CHAINS["ALLFP"])
    o = orc.Oracle(N, m)
    rng = np.random.default_rng(3)
    wide = pc.boundary_words(m[0], N)
    for i in (1, 2):
        q = m[i]
        tw = pc.seal_twiddles(o, i, N)
        rnd = rng.integers(0, m[0], N, dtype=np.uint64)
        for name, x in (("qm1", wide["qm1"]), ("alt", wide["alt"]), ("random", rnd)):
            out, peak, peak_y = pc.fp_forward_model(x, tw, q)
            assert np.array_equal(out, o.ntt_fwd(i, x % np.uint64(q))), (i, name)
            print(f"target {q.bit_length()} bits, digit {name}: max |X| = 2^{np.log2(peak):.2f} = {peak / q:.0f} q")
            assert peak < 2**45.4 and peak_y < 2**45.4
            assert peak > 2 * q  # outside the range the kernel's comment used to name


def test_forward_model_one_bit_above_the_class_limit(orc):
    """The class limit has slack: at the 43-bit prime the same model still returns the oracle's transform with every
    value an exact double (below 2^53), which is why moving the limit to 2^43 changes no output word (the limit stays
    at 2^42, the width the bounds in hec_device.h are written for)."""
    N = 1 << 16
    m = orc.Oracle.create_coeff_modulus(N, pc.NTT_BITS)
    o = orc.Oracle(N, m)
    q = m[3]
    assert q.bit_length() == 43
    tw = pc.seal_twiddles(o, 3, N)
    for x in (pc.boundary_words(q, N)["qm1"], np.random.default_rng(4).integers(0, q, N, dtype=np.uint64)):
        out, peak, peak_y = pc.fp_forward_model(x, tw, q)
        assert np.array_equal(out, o.ntt_fwd(3, x))
        assert peak < 10 * q and peak < 2**53
