"""The reference's he::fft schedules (src/core/he_fft.cpp:13-223) restated over the CPU oracle's evaluator: plain
compositions of Oracle.encode / encode_scalar, multiply_plain, rescale, rotate, add and sub, in the reference's
order.  The twiddles and diagonals are the doubles of hecdna.fft_twiddles / hecdna.bfft_diagonal (host only, the
reference's own libstdc++ expressions), the one source of these values.  This is what hec_fft / hec_bfft must equal
word for word."""
import numpy as np


def _times(o, ct, pt):
    """rescale(ct (*) pt), pt encoded at ct's level and scale"""
    return o.rescale(o.multiply_plain(ct, pt, ct.scale))


def _scale_by_inv_n(o, ct, n):
    return _times(o, ct, o.encode_scalar(1.0 / n, ct.scale, ct.level))


def fft(o, hec, cts, inverse=False):
    """he::fft::fft / ifft: the recursion of he_fft.cpp:13-68 in iterative form (bit-reversed working array)"""
    n = len(cts)
    lg = n.bit_length() - 1
    assert n == 1 << lg
    w = [cts[int(format(j, "0%db" % lg)[::-1], 2) if lg else 0].copy() for j in range(n)]
    slots = o.N // 2
    m = 2
    while m <= n:
        h = m // 2
        lvl, sc = w[0].level, w[0].scale
        tw = hec.fft_twiddles(m, inverse)
        one = o.encode(np.full(slots, complex(1, 0)), sc, lvl)
        pts = [o.encode(np.full(slots, tw[k]), sc, lvl) for k in range(h)]
        nxt = [None] * n
        for b0 in range(0, n, m):
            for k in range(h):
                t = _times(o, w[b0 + h + k], pts[k])
                e = _times(o, w[b0 + k], one)
                nxt[b0 + k] = o.add(e, t)
                nxt[b0 + h + k] = o.sub(e, t)
        w = nxt
        m *= 2
    if inverse:
        w = [_scale_by_inv_n(o, c, float(n)) for c in w]
    return w


def bfft(o, hec, ct, n, gk, inverse=False):
    """he::fft::bfft / ibfft (he_fft.cpp:166-223) on one ciphertext"""
    slots = o.N // 2
    lg = n.bit_length() - 1
    assert n == 1 << lg and n <= slots
    y = ct.copy()
    for i in range(1, lg + 1):
        k = 1 << i
        steps = n // k

        def diag(d, like):
            return o.encode(np.tile(hec.bfft_diagonal(d, k, n, inverse), slots // n), like.scale, like.level)
        y0 = _times(o, y, diag(0, y))
        y1 = o.rotate(y, steps, gk)
        y1 = _times(o, y1, diag(1, y1))
        if i != 1:
            y2 = o.rotate(y, -steps, gk)
            y2 = _times(o, y2, diag(2, y2))
            y = o.add(o.add(y0, y1), y2)
        else:
            y = o.add(y0, y1)
    if inverse:
        y = _scale_by_inv_n(o, y, float(n))
    return y


def bitrev_perm(n):
    lg = n.bit_length() - 1
    return np.array([int(format(j, "0%db" % lg)[::-1], 2) if lg else 0 for j in range(n)])
