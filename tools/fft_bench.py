#!/usr/bin/env python3
"""he::fft on the GPU: the stage-batched calls (hec_fft, hec_bfft) against the same schedules composed from the
per-ciphertext binding calls (encode, multiply_plain, rescale_to_next, add, sub, rotate_vector), in one process and
run, timed with HIP events on the context's stream.

Cases, at N = 2^15, {60, 40 x 9, 60}, on uniform synthetic ciphertexts and keys (fill_uniform):
  fft   n = 256:           8 stages, level 10 -> 2
  bfft  B = 128, n = 512:  9 stages, level 10 -> 1
The two results of a case must be equal word for word.  Prints one JSON line: both times and their ratio per case,
and every new kernel's GB/s on its algorithmic bytes (from one profiled run of the new call).

    python tools/fft_bench.py [--fft-n 256] [--bfft-b 128] [--bfft-n 512] [--reps 3] [--out profiles/fft_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def bitrev(j, lg):
    return int(format(j, "0%db" % lg)[::-1], 2) if lg else 0


def composed_fft(hec, ctx, cts, inverse=False):
    """he_fft.cpp:13-87 in iterative form, one binding call per reference call; a stage's plaintexts encoded once"""
    n, slots = len(cts), ctx.N // 2
    lg = n.bit_length() - 1
    w = [cts[bitrev(j, lg)].copy() for j in range(n)]
    m = 2
    while m <= n:
        h = m // 2
        _, level, scale = w[0].info()
        tw = hec.fft_twiddles(m, inverse)
        one = ctx.encode(np.full(slots, complex(1, 0)), scale, level)
        pts = [ctx.encode(np.full(slots, tw[k]), scale, level) for k in range(h)]
        for b0 in range(0, n, m):
            for k in range(h):
                t = ctx.rescale_to_next(ctx.multiply_plain(w[b0 + h + k], pts[k]))
                e = ctx.rescale_to_next(ctx.multiply_plain(w[b0 + k], one))
                w[b0 + h + k] = ctx.sub(e.copy(), t)
                w[b0 + k] = ctx.add(e, t)
        m *= 2
    if inverse:
        _, level, scale = w[0].info()
        pt = ctx.encode_scalar(1.0 / n, scale, level)
        w = [ctx.rescale_to_next(ctx.multiply_plain(c, pt)) for c in w]
    return w


def composed_bfft(hec, ctx, cts, n, gk, inverse=False):
    """he_fft.cpp:166-223 per ciphertext; a stage's three diagonals encoded once for the batch"""
    slots = ctx.N // 2
    lg = n.bit_length() - 1
    ys = [c.copy() for c in cts]
    for i in range(1, lg + 1):
        k, steps = 1 << i, n >> i
        _, level, scale = ys[0].info()
        d = [ctx.encode(np.tile(hec.bfft_diagonal(t, k, n, inverse), slots // n), scale, level)
             for t in range(3 if i > 1 else 2)]
        for j, y in enumerate(ys):
            y1 = ctx.rescale_to_next(ctx.multiply_plain(ctx.rotate_vector(y.copy(), steps, gk), d[1]))
            y2 = None
            if i > 1:
                y2 = ctx.rescale_to_next(ctx.multiply_plain(ctx.rotate_vector(y.copy(), -steps, gk), d[2]))
            y0 = ctx.rescale_to_next(ctx.multiply_plain(y, d[0]))
            ctx.add(y0, y1)
            if y2 is not None:
                ctx.add(y0, y2)
            ys[j] = y0
    if inverse:
        _, level, scale = ys[0].info()
        pt = ctx.encode_scalar(1.0 / n, scale, level)
        ys = [ctx.rescale_to_next(ctx.multiply_plain(c, pt)) for c in ys]
    return ys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fft-n", type=int, default=256)
    ap.add_argument("--bfft-b", type=int, default=128)
    ap.add_argument("--bfft-n", type=int, default=512)
    ap.add_argument("--reps", type=int, default=3, help="timed runs of each new call (the composed path runs once)")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()

    import torch
    torch.cuda.is_available()  # one HIP runtime for torch and the engine
    from _helpers import load_hecdna
    hec = load_hecdna()

    N, level, scale = 1 << 15, 10, 2.0**40
    moduli = hec.create_coeff_modulus(N, [60] + [40] * 9 + [60])
    ctx = hec.Context(N, moduli)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ctx.synchronize()
        e0.record(stream)
        res = fn()
        e1.record(stream)
        e1.synchronize()
        return res, e0.elapsed_time(e1)

    def equal(a, b):
        return all(x.info() == y.info() and np.array_equal(x.download(), y.download()) for x, y in zip(a, b))

    def case(new, composed):
        new()  # warm-up: workspace, encoder tables, key tables
        best, res = None, None
        for _ in range(args.reps):
            res, ms = timed(new)
            best = ms if best is None else min(best, ms)
        ref, cms = timed(composed)
        return {"new_ms": round(best, 3), "composed_ms": round(cms, 3), "composed_over_new": round(cms / best, 2),
                "equal": equal(res, ref)}

    def kernels(fn):
        ctx.profile(2)
        fn()
        ctx.synchronize()
        out = {}
        for cls in ctx.profile_classes():
            ms, scopes, nbytes, kl = ctx.profile_read_ex(cls)
            if cls.startswith("k:") or cls in ("fft_stage", "bfft_stage", "fft_encode"):
                out[cls] = {"ms": round(ms, 4), "scopes": scopes, "launches": kl,
                            "GBps": round(nbytes / (ms * 1e-3) / 1e9, 1) if ms and nbytes else None}
        ctx.profile(0)
        return out

    result = {"N": N, "moduli_bits": [60] + [40] * 9 + [60], "level": level}

    n = args.fft_n
    cts = [hec.Ciphertext(ctx).fill_uniform(2, level, scale, 1000 + i) for i in range(n)]
    result["fft"] = dict(n=n, **case(lambda: ctx.fft(cts), lambda: composed_fft(hec, ctx, cts)))
    result["fft"]["kernels"] = kernels(lambda: ctx.fft(cts))
    del cts

    B, n = args.bfft_b, args.bfft_n
    lg = n.bit_length() - 1
    steps = sorted({n >> i for i in range(1, lg + 1)} | {-(n >> i) for i in range(2, lg + 1)})
    gk = ctx.galois_keys(uniform_elts=[ctx.elt_from_step(s) for s in steps], seed=77)
    cts = [hec.Ciphertext(ctx).fill_uniform(2, level, scale, 5000 + i) for i in range(B)]
    result["bfft"] = dict(B=B, n=n, **case(lambda: ctx.bfft(cts, n, gk), lambda: composed_bfft(hec, ctx, cts, n, gk)))
    result["bfft"]["kernels"] = kernels(lambda: ctx.bfft(cts, n, gk))

    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if result["fft"]["equal"] and result["bfft"]["equal"] else 1


if __name__ == "__main__":
    sys.exit(main())
