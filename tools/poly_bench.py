#!/usr/bin/env python3
"""he::math polynomial evaluation on the GPU: the batched call (hec_math_poly) against the same Paterson-Stockmeyer
schedule composed from the per-ciphertext binding calls (encode_scalar, multiply_plain, multiply /
square, relinearize, rescale_to_next, mod_switch_to_next, add, add_plain) looped over the batch, in one process,
alternated, timed with HIP events on the context's stream.  The per-ciphertext interface has no scale setter, so the
composed path assigns a scale ("scale := S") with the calls it has: an export of the words to a device buffer and an
import with the new scale, two device copies, included in its time.

Cases, at N = 2^15, {60, 40 x 9, 60}, level 10, scale 2^40, on uniform synthetic ciphertexts and a uniform relin key:
dense polynomials of degree 7, 15 and 31 (default block size), each at B = 128 and at B = 1.  The two results of a case
must be equal word for word, or the script fails.  Every case runs in a child process of its own under `timeout` (one
process on the GPU at a time), and the script stops at the first that fails.  Prints one JSON line: per case and B both
times (median of the repetitions), their ratio, the spread (max - min over the median) of each, and every he::math
kernel class's GB/s on its algorithmic bytes from a separate profiled run of the batched call.

    python tools/poly_bench.py [--b 128] [--reps 3] [--limit 600] [--out profiles/poly_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

DEGREES = (7, 15, 31)


def coeffs_of(d):
    c = np.random.default_rng(d).uniform(-1, 1, d + 1)
    c[d] = 0.5 if abs(c[d]) < 0.1 else c[d]
    return [float(v) for v in c]


def clog2(j):
    return (j - 1).bit_length()


class Composed:
    """The schedule, one binding call per operation (every call works in place on its first argument)"""

    def __init__(self, ctx, rk, q, buf, x, coeffs, bs):
        self.ctx, self.rk, self.q, self.buf, self.x, self.c, self.bs = ctx, rk, q, buf, x, coeffs, bs
        self.l0 = x.info()[1]
        self.pw = {1: x}

    def lam(self, j):
        return self.l0 - clog2(j)

    def assign(self, ct, scale):
        size, level, _ = ct.info()
        ct.export_device(self.buf.p.value)
        ct.import_device(self.buf.p.value, size, level, scale)

    def down(self, ct, level):
        ct = ct.copy()
        while ct.info()[1] > level:
            self.ctx.mod_switch_to_next(ct)
        return ct

    def prod(self, a, b, square):
        t = self.ctx.square(a) if square else self.ctx.multiply(a, b)
        return self.ctx.rescale_to_next(self.ctx.relinearize(t, self.rk))

    def power(self, j):
        if j not in self.pw:
            a, b = (j + 1) // 2, j // 2
            A, B = self.power(a), self.power(b)
            lv = min(A.info()[1], B.info()[1])
            self.pw[j] = self.prod(self.down(A, lv), None if a == b else self.down(B, lv), a == b)
        return self.pw[j]

    def split(self, p):
        g = self.bs
        while 2 * g <= len(p) - 1:
            g *= 2
        return g, p[g:], p[:g]

    def need(self, p):
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
        ctx = self.ctx
        while len(p) > 1 and p[-1] == 0:
            p = p[:-1]
        e = len(p) - 1
        if e < self.bs:
            T = St * self.q[Lt]
            acc = None
            for j in range(1, e + 1):
                if p[j] == 0:
                    continue
                v = self.down(self.power(j), Lt + 1)
                ctx.multiply_plain(v, ctx.encode_scalar(p[j], T / v.info()[2], Lt + 1))
                self.assign(v, T)
                acc = v if acc is None else ctx.add(acc, v)
            ctx.rescale_to_next(acc)
            self.assign(acc, St)
            if p[0] != 0:
                ctx.add_plain(acc, ctx.encode_scalar(p[0], St, Lt))
            return acc
        g, quo, rem = self.split(p)
        X = self.down(self.power(g), Lt + 1)
        ps = St * self.q[Lt] / X.info()[2]
        if any(quo[1:]):
            r = self.prod(self.ev(quo, Lt + 1, ps), X, False)
        else:
            r = ctx.rescale_to_next(ctx.multiply_plain(X, ctx.encode_scalar(quo[0], ps, Lt + 1)))
        self.assign(r, St)
        if any(rem[1:]):
            ctx.add(r, self.ev(rem, Lt, St))
        elif rem[0] != 0:
            ctx.add_plain(r, ctx.encode_scalar(rem[0], St, Lt))
        return r

    def run(self):
        return self.ev(self.c, self.need(self.c), self.x.info()[2])


def child(d, B, reps):
    import torch
    torch.cuda.is_available()  # one HIP runtime for torch and the engine
    from _helpers import load_hecdna
    hec = load_hecdna()
    N, level, scale = 1 << 15, 10, 2.0**40
    q = hec.create_coeff_modulus(N, [60] + [40] * 9 + [60])
    ctx = hec.Context(N, q)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    rk = ctx.relin_key(seed=99)
    cts = [hec.Ciphertext(ctx).fill_uniform(2, level, scale, 1000 + i) for i in range(B)]
    coeffs = coeffs_of(d)
    lv, sc, bs, nprod, nleaf = hec.math_poly_plan(q, coeffs, level, scale)
    buf = hec.DeviceBuffer(ctx, 2 * level * N * 8)

    def new():
        return ctx.poly(cts, coeffs, rk)

    def composed():
        return [Composed(ctx, rk, [int(v) for v in q], buf, c, coeffs, bs).run() for c in cts]

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ctx.synchronize()
        e0.record(stream)
        res = fn()
        e1.record(stream)
        e1.synchronize()
        return res, e0.elapsed_time(e1)

    def stats(ms):
        med = float(np.median(ms))
        return {"ms": round(med, 3), "spread": round((max(ms) - min(ms)) / med, 4), "runs_ms": [round(v, 3) for v in ms]}

    new()
    composed()  # warm-up of both: workspace, buffers
    tn, tc, res, ref = [], [], None, None
    for _ in range(reps):  # alternated
        res, ms = timed(new)
        tn.append(ms)
        ref, ms = timed(composed)
        tc.append(ms)
    equal = all(x.info() == y.info() and np.array_equal(x.download(), y.download()) for x, y in zip(res, ref))
    out = {"degree": d, "B": B, "bs": bs, "products": nprod, "leaves": nleaf, "level_out": res[0].info()[1],
           "new": stats(tn), "composed": stats(tc), "equal": equal and res[0].info()[1:] == (lv, sc)}
    out["composed_over_new"] = round(out["composed"]["ms"] / out["new"]["ms"], 3)
    del ref
    ctx.profile(2)  # a separate profiled run of the batched call
    new()
    ctx.synchronize()
    kern = {}
    for cls in ctx.profile_classes():
        ms, scopes, nbytes, kl = ctx.profile_read_ex(cls)
        if "/math" in cls:
            kern[cls] = {"ms": round(ms, 4), "scopes": scopes, "launches": kl,
                         "GBps": round(nbytes / (ms * 1e-3) / 1e9, 1) if ms and nbytes else None}
    ctx.profile(0)
    out["kernels"] = kern
    print("RESULT " + json.dumps(out))
    return 0 if out["equal"] else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--b", type=int, default=128)
    ap.add_argument("--reps", type=int, default=3, help="timed runs of each path, alternated (at least 3)")
    ap.add_argument("--limit", type=int, default=600, help="seconds a case may take")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--child", nargs=2, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    reps = max(3, args.reps)
    if args.child:
        return child(int(args.child[0]), int(args.child[1]), reps)
    result = {"N": 1 << 15, "moduli_bits": [60] + [40] * 9 + [60], "level": 10, "scale_log2": 40, "reps": reps,
              "cases": []}
    for B in (args.b, 1):
        for d in DEGREES:
            cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--reps", str(reps),
                   "--child", str(d), str(B)]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if lines:
                result["cases"].append(json.loads(lines[-1][7:]))
            if p.returncode != 0 or not lines:  # the first failure ends the run
                print(json.dumps(result))
                print("poly_bench: degree %d B=%d failed (exit %d)" % (d, B, p.returncode), file=sys.stderr)
                return 1
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
