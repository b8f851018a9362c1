"""TEST INFRASTRUCTURE: the Paterson-Stockmeyer schedule of hec_math_poly restated per operation over
oracle_py.Oracle.  Every step is one oracle call (multiply / square, relinearize, rescale, mod_switch, multiply_plain of
a scalar encode, add, add_plain); "scale := S" is an assignment to Ct.scale.  The engine's batched call must give these
bits, level and scale; the planner must give this level, scale, block size and these counts."""
import math


def clog2(j):
    return (j - 1).bit_length()


def default_bs(d):
    return 1 << min(4, max(1, -(-clog2(d + 1) // 2)))


def trim(c):
    c = [float(v) for v in c]
    while len(c) > 1 and c[-1] == 0:
        c.pop()
    return c


class Poly:
    """One evaluation: run() returns the result; nprod counts the relinearised products (powers included), nleaf the
    leaves (rescaled sums of scalar multiples)"""

    def __init__(self, o, rk, x, coeffs, bs=None):
        self.c = trim(coeffs)
        if any(not math.isfinite(v) for v in self.c):
            raise ValueError("coefficients must be finite")
        if len(self.c) < 2:
            raise ValueError("polynomial must not be constant")
        self.bs = default_bs(len(self.c) - 1) if not bs else bs
        if self.bs not in (2, 4, 8, 16):
            raise ValueError("bs must be a power of two in [2, 16]")
        self.o, self.rk, self.x = o, rk, x
        self.q = [int(v) for v in o.moduli]
        self.pw = {1: x}
        self.nprod = self.nleaf = 0

    def lam(self, j):
        return self.x.level - clog2(j)

    def down(self, ct, level):
        while ct.level > level:
            ct = self.o.mod_switch(ct)
        return ct

    def prod(self, a, b, square=False):
        t = self.o.square(a) if square else self.o.multiply(a, b)
        self.nprod += 1
        return self.o.rescale(self.o.relinearize(t, self.rk))

    def power(self, j):
        if j not in self.pw:
            a, b = (j + 1) // 2, j // 2
            A, B = self.power(a), self.power(b)
            lv = min(A.level, B.level)
            self.pw[j] = self.prod(self.down(A, lv), self.down(B, lv), a == b)
            assert self.pw[j].level == self.lam(j)
        return self.pw[j]

    def split(self, p):
        g = self.bs
        while 2 * g <= len(p) - 1:
            g *= 2
        return g, p[g:], p[:g]

    def need(self, p):
        p = trim(p)
        if len(p) - 1 < self.bs:
            return min(self.lam(j) for j in range(1, len(p)) if p[j] != 0) - 1
        g, quo, rem = self.split(p)
        v = self.lam(g) - 1
        if any(quo[1:]):
            v = min(v, self.need(quo) - 1)
        if any(rem[1:]):
            v = min(v, self.need(rem))
        return v

    def ev(self, p, Lt, St):
        o = self.o
        p = trim(p)
        e = len(p) - 1
        if e < self.bs:
            T = St * self.q[Lt]
            acc = None
            for j in range(1, e + 1):
                if p[j] == 0:
                    continue
                v = self.down(self.power(j), Lt + 1)
                ps = T / v.scale
                t = o.multiply_plain(v, o.encode_scalar(p[j], ps, Lt + 1), ps)
                t.scale = T
                acc = t if acc is None else o.add(acc, t)
            r = o.rescale(acc)
            r.scale = St
            self.nleaf += 1
            if p[0] != 0:
                r = o.add_plain(r, o.encode_scalar(p[0], St, Lt), St)
            return r
        g, quo, rem = self.split(p)
        X = self.down(self.power(g), Lt + 1)
        if any(quo[1:]):
            r = self.prod(self.ev(quo, Lt + 1, St * self.q[Lt] / X.scale), X)
        else:
            ps = St * self.q[Lt] / X.scale
            r = o.rescale(o.multiply_plain(X, o.encode_scalar(quo[0], ps, Lt + 1), ps))
        r.scale = St
        if any(rem[1:]):
            r = o.add(r, self.ev(rem, Lt, St))
        elif rem[0] != 0:
            r = o.add_plain(r, o.encode_scalar(rem[0], St, Lt), St)
        return r

    def run(self):
        L = self.need(self.c)
        if L < 1:
            raise ValueError("end of modulus switching chain reached")
        r = self.ev(self.c, L, self.x.scale)
        assert r.level == L
        return r


def poly(o, rk, x, coeffs, bs=None):
    return Poly(o, rk, x, coeffs, bs).run()
