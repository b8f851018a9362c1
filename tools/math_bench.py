#!/usr/bin/env python3
"""he::math on the GPU: the batched calls (hec_math_signed_inv / inv_sqrt_twice / abs) against the same schedules
composed from the per-ciphertext binding calls (encode_scalar, multiply_plain, multiply / square, relinearize,
rescale_to_next, add_plain / sub_plain, sub) looped over the batch, in one process, alternated, timed with HIP events
on the context's stream.

Cases, at N = 2^15, {60, 40 x 9, 60}, level 10, scale 2^40, on uniform synthetic ciphertexts and a uniform relin key:
  signed_inv(0.01, 7)      level 10 -> 2  (the reference's own call, server.cpp:289, math_operations.cpp:360)
  inv_sqrt_twice(0.01, 4)  level 10 -> 3
  abs(1.0, 4)              level 10 -> 1
each at B = 128 and at B = 1.  The two results of a case must be equal word for word, or the script fails.  Every
case runs in a child process of its own under `timeout` (one process on the GPU at a time), and the script stops at
the first that fails.  Prints one JSON line: per case and B both times (median of the repetitions), their ratio, the
spread (max - min over the median) of each, and every new kernel's GB/s on its algorithmic bytes from a separate
profiled run of the batched call.

    python tools/math_bench.py [--b 128] [--reps 3] [--limit 600] [--out profiles/math_bench.json]
"""
import argparse
import json
import math
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = {"signed_inv": (0.01, 7, 2), "inv_sqrt_twice": (0.01, 4, 3), "abs": (1.0, 4, 1)}  # a, iters, final level


# ---- the per-operation schedules (he_math.cpp:22-269), one binding call per reference call, in place on copies
def scalar(ctx, value, like):
    _, level, scale = like.info()
    return ctx.encode_scalar(value, scale, level)


def times_const(ctx, ct, c):
    return ctx.rescale_to_next(ctx.multiply_plain(ct, scalar(ctx, c, ct)))


def times_ct(ctx, rk, a, b=None):
    return ctx.rescale_to_next(ctx.relinearize(ctx.square(a) if b is None else ctx.multiply(a, b), rk))


def composed_signed_inv(ctx, rk, x, a, iters):
    y = ctx.rescale_to_next(ctx.multiply_plain(x.copy(), scalar(ctx, -a * a, x)))
    ctx.add_plain(y, scalar(ctx, 2 * a, y))
    if iters == 1:
        return y
    e = ctx.rescale_to_next(ctx.multiply_plain(x.copy(), scalar(ctx, a, x)))
    one = scalar(ctx, 1.0, e)
    ctx.sub_plain(e, one)
    ctx.rescale_to_next(ctx.multiply_plain(y, one))
    for _ in range(1, iters):
        times_ct(ctx, rk, e)
        term = ctx.add_plain(e.copy(), scalar(ctx, 1.0, e))
        times_ct(ctx, rk, y, term)
    return y


def composed_inv_sqrt_twice(ctx, rk, x, a, iters):
    x = x.copy()
    y = ctx.rescale_to_next(ctx.multiply_plain(x.copy(), scalar(ctx, -a * a * a, x)))
    ctx.add_plain(y, scalar(ctx, 3.0 / 2 * a, y))
    for i in range(1, iters):
        yp = y.copy()
        times_const(ctx, y, 3.0 / 2)
        times_const(ctx, y, 1.0)
        for _ in range(2 if i > 1 else 1):
            times_const(ctx, x, 1.0)
        xy = times_ct(ctx, rk, x.copy(), yp)
        times_ct(ctx, rk, yp)
        times_ct(ctx, rk, yp, xy)
        ctx.sub(y, yp)
    return y


def composed_abs(ctx, rk, x, a, iters):
    sq = times_ct(ctx, rk, x.copy())
    y = composed_inv_sqrt_twice(ctx, rk, sq, 1 / a / math.sqrt(2), iters)
    times_const(ctx, sq, math.sqrt(2))
    while sq.info()[1] > y.info()[1]:
        times_const(ctx, sq, 1.0)
    return times_ct(ctx, rk, y, sq)


COMPOSED = {"signed_inv": composed_signed_inv, "inv_sqrt_twice": composed_inv_sqrt_twice, "abs": composed_abs}


def child(name, B, reps):
    import torch
    torch.cuda.is_available()  # one HIP runtime for torch and the engine
    from _helpers import load_hecdna
    hec = load_hecdna()
    N, level, scale = 1 << 15, 10, 2.0**40
    ctx = hec.Context(N, hec.create_coeff_modulus(N, [60] + [40] * 9 + [60]))
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    rk = ctx.relin_key(seed=99)
    cts = [hec.Ciphertext(ctx).fill_uniform(2, level, scale, 1000 + i) for i in range(B)]
    a, iters, final = CASES[name]

    def new():
        return getattr(ctx, name)(cts, a, iters, rk)

    def composed():
        return [COMPOSED[name](ctx, rk, c, a, iters) for c in cts]

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
    out = {"case": name, "B": B, "a": a, "iters": iters, "level_out": res[0].info()[1], "new": stats(tn),
           "composed": stats(tc), "equal": equal and res[0].info()[1] == final}
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
        return child(args.child[0], int(args.child[1]), reps)
    result = {"N": 1 << 15, "moduli_bits": [60] + [40] * 9 + [60], "level": 10, "reps": reps, "cases": []}
    for B in (args.b, 1):
        for name in CASES:
            cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--reps", str(reps),
                   "--child", name, str(B)]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
            if lines:
                result["cases"].append(json.loads(lines[-1][7:]))
            if p.returncode != 0 or not lines:  # the first failure ends the run
                print(json.dumps(result))
                print("math_bench: case %s B=%d failed (exit %d)" % (name, B, p.returncode), file=sys.stderr)
                return 1
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
