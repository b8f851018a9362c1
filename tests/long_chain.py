"""Shared by test_long_chain.py (CPU) and test_gpu_long_chain.py: the modulus chains of the greatest length the engine
accepts (HEC_MAXL + 1 = 33 primes), the decode levels on both sides of every word-count class of the decoder's CRT
(dec_wmax, hec_decode.hip), the monomial plaintexts c X^k whose decoding is known in closed form, and the key-switch
input whose lazy sums are the largest the kernels can meet.  N = 2^10, the smallest context the engine accepts."""
import numpy as np

N10 = 1 << 10
MAXL = 32                                  # HEC_MAXL: levels per context; K = MAXL + 1 primes
CHAINS = {
    "ALL60": [60] * 33,                    # every digit and target integer-class: 32-summand 128-bit sums, widest CRT
    "FP42": [60] + [42] * 31 + [60],       # 31 FP64-class targets summing 32 exact products of the widest FP64 primes
    "ALLFP42": [42] * 33,                  # q_0 and the special prime in the FP64 class at full length
}
SCALE = {"ALL60": 2.0**40, "FP42": 2.0**40, "ALLFP42": 2.0**30}

WM_CLASSES = (4, 8, 11, 17)                # the instantiations of k_dec_crt_upper<TS, WM>
DECODE_LEVELS = (1, 4, 5, 8, 9, 11, 12, 17, 18)   # on ALL60: both sides of every class edge
REJECT_LEVELS = (19, 32)                   # the first level past the last class, and the top of the chain


def modulus(m, level):
    Q = 1
    for q in m[:level]:
        Q *= int(q)
    return Q


def crt_words(m, level):
    """64-bit words of level Q: the decoder's composition sum_i y_i (Q / q_i) is below it"""
    return -(-(level * modulus(m, level)).bit_length() // 64)


def wm_class(words):
    """dec_wmax restated: the smallest class that holds the words, None past the last"""
    return next((w for w in WM_CLASSES if words <= w), None)


# ------------------------------------------------------------------ monomial plaintexts
def grid(m, level):
    """The coefficients c of the monomial grid at a level: +-2^e and +-(2^(e + 1) - 1) for e in {0, 1, 52, 53, 63,
    64, 65} and e = 64 w - 1, 64 w, 64 w + 1 (w = 1 .. 16), wherever |c| <= (Q - 1) / 2 and |c| < 2^1020, and
    +-(Q - 1) / 2 itself where that is below 2^1020 (every level but 18 on ALL60).  Every word of the accumulator,
    every carry of mw_mac and every borrow of mw_sub / mw_rsub decides one of these."""
    Q = modulus(m, level)
    half = (Q - 1) // 2
    es = {0, 1, 52, 53, 63, 64, 65}
    for w in range(1, 17):
        es |= {64 * w - 1, 64 * w, 64 * w + 1}
    mags = set()
    for e in sorted(es):
        mags |= {1 << e, (1 << (e + 1)) - 1}
    mags = {c for c in mags if c <= half and c < 1 << 1020}
    if half < 1 << 1020:
        mags.add(half)
    return [s * c for c in sorted(mags) for s in (1, -1)]


def grid_scale(c):
    """a power of two that brings |c| / scale into [1, 2^20): its square sums without overflow in the tolerance"""
    return 2.0 ** max(0, abs(int(c)).bit_length() - 20)


def grid_k(idx, N):
    """the monomial's degree for grid entry idx: 0 (the constant), then odd and even degrees across the ring"""
    return 0 if idx == 0 else (idx * 37 + (idx & 1)) % N


def monomial_plain(o, m, level, c, k, N):
    """u64[level][N], NTT form: the polynomial c X^k, limb i holding c mod q_i at coefficient k"""
    out = np.zeros((level, N), dtype=np.uint64)
    for i in range(level):
        co = np.zeros(N, dtype=np.uint64)
        co[k] = int(c) % int(m[i])
        out[i] = o.ntt_fwd(i, co)
    return out


def _longdouble(c):
    """|c| to np.longdouble: the top 64 bits, exactly, in two 32-bit halves (2^-63 relative)"""
    c = abs(int(c))
    sh = max(0, c.bit_length() - 64)
    top = c >> sh
    v = np.longdouble(top >> 32) * np.longdouble(2.0**32) + np.longdouble(top & 0xffffffff)
    return v, sh


def monomial_slots(c, scale, k, N):
    """The exact decoding of c X^k at a power-of-two scale: slot j = (c / scale) exp(i pi ((3^j mod 2N) k mod 2N) / N),
    j < N / 2 (the generator of the slot order is 3), in np.longdouble with the exponent reduced as an integer"""
    mant, sh = _longdouble(c)
    e = int(np.log2(scale))
    assert 2.0**e == scale
    amp = np.ldexp(mant, sh - e) * (-1 if c < 0 else 1)
    pos = np.empty(N // 2, dtype=np.int64)
    g = 1
    for j in range(N // 2):
        pos[j] = g
        g = g * 3 % (2 * N)
    pi = np.longdouble("3.14159265358979323846264338327950288")
    ang = ((pos * k) % (2 * N)).astype(np.longdouble) * (pi / np.longdouble(N))
    return amp * np.cos(ang) + 1j * (amp * np.sin(ang))


# ------------------------------------------------------------------ the key switch whose sums are largest
def worst_switch(m, l, N):
    """(target u64[l][N], key u64[K - 1][2][K][N]): every NTT word of limb J of the target is q_J - 1 and every word
    of the key at prime I is q_I - 1.  The target's coefficient form is -1 at coefficient 0 and N - 1 zeros, so digit J
    at target I is the constant (q_J - 1) mod q_I, and the sum at I is (q_I - 1) sum_J ((q_J - 1) mod q_I)."""
    K = len(m)
    target = np.stack([np.full(N, int(m[J]) - 1, dtype=np.uint64) for J in range(l)])
    key = np.empty((K - 1, 2, K, N), dtype=np.uint64)
    for I in range(K):
        key[:, :, I, :] = int(m[I]) - 1
    return target, key


def worst_sum(m, l, I):
    """the canonical (every operand reduced) integer sum of that key switch at the prime of index I of the chain"""
    qI = int(m[I])
    return (qI - 1) * sum((int(m[J]) - 1) % qI if J != I else qI - 1 for J in range(l))
