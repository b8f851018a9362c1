"""The inputs of test_gpu_long_chain.py checked on the CPU with the oracle alone: the 33-prime chains are what the GPU
tests take them for, the decode levels sit on both sides of every word-count class of the decoder's CRT, the oracle's
key switch at l = 32 equals the big-integer restatement (also on the input whose lazy sums are the largest), those
sums stay inside the bounds the kernels state, the oracle decodes the monomial grid within half of the decoder's
tolerance of the closed form, and a chain of 34 primes is refused."""
from fractions import Fraction

import numpy as np
import pytest

import long_chain as lc
import prime_classes as pc
from test_gpu_decode import tol_of
from test_oracle_keyswitch import py_switch_key, random_ct

N = lc.N10


@pytest.fixture(scope="module")
def chains(orc):
    return {k: orc.Oracle.create_coeff_modulus(N, bits) for k, bits in lc.CHAINS.items()}


# ------------------------------------------------------------------ 1. the chains
def test_chains(chains):
    for name, bits in lc.CHAINS.items():
        q = chains[name]
        assert len(q) == lc.MAXL + 1 == 33 and len(set(q)) == 33, name
        assert [x.bit_length() for x in q] == bits, name
        assert [x < pc.FP_LIMIT for x in q] == [b <= 42 for b in bits], name
    assert not any(x < pc.FP_LIMIT for x in chains["ALL60"])
    assert [x < pc.FP_LIMIT for x in chains["FP42"]] == [False] + [True] * 31 + [False]
    assert all(x < pc.FP_LIMIT for x in chains["ALLFP42"])
    assert min(chains["FP42"][1:32]) > 0.999 * 2**42   # the FP64 class at its widest, all 31 of them


# ------------------------------------------------------------------ 2. the decoder's word-count classes
def test_decode_levels_sit_on_every_class_edge(chains):
    m = chains["ALL60"]
    words = {level: lc.crt_words(m, level) for level in lc.DECODE_LEVELS + lc.REJECT_LEVELS}
    assert [words[level] for level in lc.DECODE_LEVELS] == [1, 4, 5, 8, 9, 11, 12, 17, 17]
    assert [lc.wm_class(words[level]) for level in lc.DECODE_LEVELS] == [4, 4, 8, 8, 11, 11, 17, 17, 17]
    for wm in lc.WM_CLASSES:  # the last word count of each class and the first of the next are both decoded
        assert wm in words.values() and (wm == 17 or wm + 1 in words.values())
    assert words[19] == 18 and words[32] == 31
    assert all(lc.wm_class(words[level]) is None for level in lc.REJECT_LEVELS)
    assert lc.crt_words(m, 18) == 17 and lc.modulus(m, 18).bit_length() > 1024   # level 18: 17 words, past a double


# ------------------------------------------------------------------ 3. the oracle's key switch at l = 32
@pytest.mark.parametrize("chain", ["ALL60", "FP42"])
def test_oracle_switch_key_l32(orc, chains, chain):
    m = chains[chain]
    o = orc.Oracle(N, m)
    rk = o.relin_key(o.secret_key(31), 32)
    assert rk.shape == (32, 2, 33, N)
    ct = orc.Ct(random_ct(m, 2, 32, 33), 2.0**40)
    target = random_ct(m, 1, 32, 34)[0]
    assert np.array_equal(o.switch_key(ct, target, rk).data, py_switch_key(o, m, ct, target, rk))
    wt, wk = lc.worst_switch(m, 32, N)
    for J in (0, 31):   # the coefficient form the GPU suite relies on: -1 at coefficient 0, N - 1 zeros
        co = o.ntt_inv(J, wt[J])
        assert co[0] == m[J] - 1 and not co[1:].any()
    assert np.array_equal(o.switch_key(ct, wt, wk).data, py_switch_key(o, m, ct, wt, wk))


# ------------------------------------------------------------------ 4. the sums at l = 32 against their bounds
def test_sum_fractions(chains):
    """Integer targets (k_bmac, k_hmacm, ks_mac): 128-bit lazy sums of l products v k with v < 4 q (the lazy digit
    word) and k < q: below 2^127 at l = 32 for any primes below 2^60; the canonical worst case (every operand reduced)
    reaches 2^125.0 of the accumulator's 2^128.  FP64 targets: sums of l (k_bmac) or l + 2 (k_hmacm, with the two
    correction terms) exact products in [-0.53 q, 0.53 q], which fp_canon takes below 2^52."""
    l = 32
    m = chains["ALL60"]
    qmax = max(m)
    assert l * (4 * qmax - 1) * (qmax - 1) < 1 << 127          # the kernel's own operands, the lazy digit included
    worst = max(lc.worst_sum(m, l, I) for I in list(range(l)) + [32])
    assert worst < 1 << 128
    frac = Fraction(worst, 1 << 128)
    print(f"ALL60 l = 32: canonical worst-case sum = 2^{np.log2(float(worst)):.2f}, {float(frac):.4f} of 2^128, "
          f"{float(Fraction(worst, 1 << 127)):.4f} of the lazy bound 2^127")
    assert Fraction(1, 16) < frac < Fraction(1, 8)              # 2^124 .. 2^125: 32 products of (q - 1)^2, q < 2^60
    for name in ("FP42", "ALLFP42"):
        m = chains[name]
        fp = [q for q in m if q < pc.FP_LIMIT]
        q = max(fp)
        bound = Fraction(53, 100) * (l + 2) * q
        assert bound < 1 << 52
        # what the worst-case input reaches at an FP64 target: l centred residues of ((q_J - 1) mod q_I) (q_I - 1)
        reach = 0
        for I in [i for i in range(33) if m[i] < pc.FP_LIMIT]:
            qI = m[I]
            terms = [abs(pc.centred(((m[J] - 1) % qI if J != I else qI - 1) * (qI - 1), qI)) for J in range(l)]
            assert all(t <= Fraction(53, 100) * qI for t in terms)
            reach = max(reach, Fraction(sum(terms), qI))
        print(f"{name} l = 32: FP64 bound 0.53 q (l + 2) = 2^{np.log2(float(bound)):.2f} = {float(bound / 2**52):.4f} "
              f"of 2^52; the worst-case input sums to {float(reach):.2f} q of the bound's {0.53 * (l + 2):.2f} q")
        assert reach <= Fraction(53, 100) * (l + 2)
        # the GPU suite's `halves` input (target words 1, key words (q_I - 1) / 2): every digit at every target is the
        # constant 1, so each of the l products is +(q_I - 1) / 2, its own centred residue
        halves = max(Fraction(l * pc.centred((qI - 1) // 2, qI), qI) for qI in fp)
        print(f"{name} l = 32: the halves input sums to {float(halves):.2f} q, "
              f"{float(halves / (Fraction(53, 100) * (l + 2))):.3f} of the bound")
        assert Fraction(88, 100) * Fraction(53, 100) * (l + 2) < halves <= Fraction(53, 100) * (l + 2)


# ------------------------------------------------------------------ 5. the oracle's decode of the monomial grid
@pytest.mark.parametrize("level", lc.DECODE_LEVELS)
def test_oracle_decodes_the_monomial_grid(orc, chains, level):
    """the same requirement as test_oracle_decode.py: the reference side alone uses at most half of the tolerance"""
    m = chains["ALL60"]
    o = orc.Oracle(N, m)
    cs = lc.grid(m, level)
    half = (lc.modulus(m, level) - 1) // 2
    assert all(abs(c) <= half and abs(c) < 1 << 1020 for c in cs) and len(set(cs)) == len(cs)
    assert (half in cs and -half in cs) == (level != 18)
    worst = 0.0
    for idx, c in enumerate(cs):
        k, scale = lc.grid_k(idx, N), lc.grid_scale(c)
        ref = lc.monomial_slots(c, scale, k, N)
        got = o.decode(lc.monomial_plain(o, m, level, c, k, N), scale)
        err = float(np.linalg.norm(got.astype(np.clongdouble) - ref))
        tol = float(tol_of(ref, N))
        assert np.isfinite(tol) and tol > 0
        assert err <= tol / 2, (level, c, k, err, tol)
        worst = max(worst, err / tol)
    print(f"oracle decode of the monomial grid, level {level} ({len(cs)} monomials): max error / tol {worst:.3f}")


# ------------------------------------------------------------------ 6. one prime too many
def test_chain_of_34_primes_is_refused(hecdna):
    """hec_context_create checks its arguments before it touches a device"""
    m = hecdna.create_coeff_modulus(N, [42] * 34)
    assert len(m) == 34
    with pytest.raises(hecdna.InvalidArgument, match="coeff_modulus size is invalid"):
        hecdna.Context(N, m)
