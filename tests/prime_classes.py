"""Shared by test_prime_classes.py (CPU) and test_gpu_prime_classes.py: the modulus chains that sit on the edges of the
two arithmetic classes (FP64 for q < 2^42, integer otherwise), the boundary residues, the ciphertext that every rotation
leaves unchanged, and the exact-integer model of the FP64 forward transform."""
import numpy as np

FP_LIMIT = 1 << 42        # hec_context_create: p.fp = q < 2^42
C30_LIMIT = 1 << 32       # FanDivRound: the split reduction (c30 != 0) only above 2^32
N11 = 1 << 11

CHAINS = {
    "TOP": [60, 42, 42, 60],               # the FP64 class at its widest
    "EDGE": [60, 42, 43, 60],              # the two classes one bit apart, each feeding the other's targets
    "INT": [59, 43, 59, 60],               # an integer-class digit (not q_0) that needs Barrett at a 43-bit target
    "ALLFP": [42, 30, 36, 42],             # q_0 and the special prime in the FP64 class, a prime <= 2^32
    "LONG": [60] + [42] * 10 + [60],       # eleven digits per key MAC, ten of them 42-bit
}
SCALE = {"TOP": 2.0**40, "EDGE": 2.0**40, "INT": 2.0**40, "ALLFP": 2.0**30, "LONG": 2.0**42}
NTT_BITS = [60, 42, 41, 43, 30, 60]

PATTERNS = ("zero", "one", "qm1", "half_lo", "half_hi", "alt", "first", "last")


def boundary_words(q, N):
    """name -> u64[N]: the residues where fp_canon's sign branch, rint at a tie and the csub edges decide the bits"""
    q = int(q)
    w = {
        "zero": np.zeros(N, np.uint64),
        "one": np.ones(N, np.uint64),
        "qm1": np.full(N, q - 1, np.uint64),
        "half_lo": np.full(N, (q - 1) // 2, np.uint64),
        "half_hi": np.full(N, (q + 1) // 2, np.uint64),
        "alt": np.zeros(N, np.uint64),
        "first": np.zeros(N, np.uint64),
        "last": np.zeros(N, np.uint64),
    }
    w["alt"][1::2] = q - 1
    w["first"][0] = q - 1
    w["last"][N - 1] = q - 1
    assert tuple(w) == PATTERNS
    return w


def transform_inputs(o, i, N):
    """the boundary words of limb i, and the oracle's ntt_inv / ntt_fwd preimages of the constant ones: a forward
    (inverse) transform of those lands exactly on 0, 1, q - 1 and the two halves"""
    q = int(o.moduli[i])
    w = boundary_words(q, N)
    out = dict(w)
    for name in ("one", "qm1", "half_lo", "half_hi", "alt"):
        out["inv_of_" + name] = o.ntt_inv(i, w[name])
        out["fwd_of_" + name] = o.ntt_fwd(i, w[name])
    return out


def pattern_poly(m, level, N, name):
    """u64[level][N]: the named pattern in every limb"""
    return np.stack([boundary_words(m[i], N)[name] for i in range(level)])


def pattern_ct(orc, m, size, level, N, names, scale):
    """a ciphertext whose poly p holds pattern names[p % len(names)] in every limb"""
    return orc.Ct(np.stack([pattern_poly(m, level, N, names[p % len(names)]) for p in range(size)]), scale)


def invariant_ct(orc, m, level, N, scale):
    """c0 = 1 in every NTT word, c1 = 0: the Galois map permutes NTT words and the key switch of the zero polynomial
    is zero, so every rotation returns it unchanged"""
    return pattern_ct(orc, m, 2, level, N, ["one", "zero"], scale)


def centred(x, q):
    """the representative fp_mulmod leaves: x mod q in [-(q - 1) / 2, (q - 1) / 2]"""
    x = int(x) % int(q)
    return x - int(q) if x > (int(q) - 1) // 2 else x


# ------------------------------------------------------------------ the FP64 forward transform in exact integers
def seal_twiddles(o, i, N):
    """tw[bitrev(k)] = psi^k: the table order of the engine and of SEAL"""
    q, psi = int(o.moduli[i]), o.root(i)
    logN = N.bit_length() - 1
    tw = [0] * N
    pw = 1
    for k in range(N):
        tw[int(format(k, f"0{logN}b")[::-1], 2)] = pw
        pw = pw * psi % q
    return tw


def fp_mulmod_model(y, w, q, qinv):
    """hec_device.h fp_mulmod over object arrays of Python integers: y w - k q with k = rint(fl(y w) * fl(1 / q)), the
    only floating step; the kernel's TwoProduct and FMA are exact by its own argument, so the rest is integer"""
    h = y.astype(np.float64) * w.astype(np.float64)
    k = np.rint(h * qinv)
    assert np.all(np.abs(k) < 2.0**62)
    return y * w - k.astype(np.int64).astype(object) * q


def fp_forward_model(x, tw, q):
    """The forward transform as k_ntt / k_fan2 schedule it for an FP64-class prime: the Cooley-Tukey network in SEAL's
    table order over logN stages, inputs converted once (u2d), no canonicalisation between the rounds or between pass
    A and pass B (the words between the passes are the doubles' bits), fp_canon at the output only.
    Returns (canonical output, max |X| over every stage's outputs, max |Y| over every fp_mulmod operand)."""
    N = len(x)
    q = int(q)
    qinv = 1.0 / float(q)
    a = np.array([int(v) for v in x], dtype=object)
    twa = np.array(tw, dtype=object)
    peak = int(max(abs(v) for v in a))
    peak_y = 0
    m, t = 1, N
    while m < N:
        t >>= 1
        v = a.reshape(m, 2, t)
        X, Y = v[:, 0, :], v[:, 1, :]
        w = np.repeat(twa[m:2 * m], t).reshape(m, t)
        peak_y = max(peak_y, int(np.max(np.abs(Y))))
        T = fp_mulmod_model(Y.reshape(-1), w.reshape(-1), q, qinv).reshape(m, t)
        a = np.stack([X + T, X - T], axis=1).reshape(N)
        peak = max(peak, int(np.max(np.abs(a))))
        m <<= 1
    return np.array([int(v) % q for v in a], dtype=np.uint64), peak, peak_y
