#!/usr/bin/env python3
"""he::linalg's batched element-wise calls on the GPU (hec_multiply_relin_rescale_many, hec_sum_elems_many) against the
same schedules composed from the per-ciphertext binding calls (multiply / square, relinearize, rescale_to_next;
rotate_vector, add) looped over the batch, and the fused rotate-accumulate epilogue (option "rot_add" = 1) against
the separate k_ew_add launch ("rot_add" = 0): all sides in one process, alternated, timed with HIP events on the
context's stream.

Cases, at N = 2^15, {60, 40 x 9, 60}, scale 2^40, on uniform synthetic ciphertexts and uniform keys:
  sum      sum_elems with dim 4096 (the 12 steps 2048 .. 1)
  product  rescale(relin(a[i] * b[i]))
each at levels 10 and 3 and at B = 128 and B = 1.  The results of a case must be equal word for word, or the script
fails.  Every case runs in a child process of its own under `timeout` (one process on the GPU at a time), and the
script stops at the first that fails.  Prints one JSON line: per case both (three) times (median of the repetitions),
their ratios, the spread (max - min over the median) of each, and every kernel class's GB/s on its algorithmic bytes
from separate profiled runs of the batched call.

    python tools/linalg_bench.py [--b 128] [--reps 3] [--limit 300] [--out profiles/linalg_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

DIM = 4096


# ---- the per-operation schedules, one binding call per call of cpp/src/he_linalg.cpp's loops
def composed_product(ctx, rk, a, b):
    return ctx.rescale_to_next(ctx.relinearize(ctx.multiply(a.copy(), b), rk))


def composed_sum(ctx, gk, x, dim):
    bvec, to_sum = x.copy(), x.copy()
    window, have = 1, False
    if dim & 1:
        have = True
        ctx.rotate_vector(to_sum, window, gk)
    bits = dim >> 1
    while bits:
        window <<= 1
        if bits & 1:
            steps = window >> 1
            acc = ctx.add(to_sum.copy(), ctx.rotate_vector(to_sum.copy(), steps, gk))
            steps >>= 1
            while steps:
                ctx.add(acc, ctx.rotate_vector(acc.copy(), steps, gk))
                steps >>= 1
            if have:
                ctx.add(bvec, acc)
            else:
                bvec, have = acc, True
            if bits != 1:
                ctx.rotate_vector(to_sum, window, gk)
        bits >>= 1
    return bvec


def child(name, level, B, reps):
    import torch
    torch.cuda.is_available()  # one HIP runtime for torch and the engine
    from _helpers import load_hecdna
    hec = load_hecdna()
    N, scale = 1 << 15, 2.0**40
    ctx = hec.Context(N, hec.create_coeff_modulus(N, [60] + [40] * 9 + [60]))
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    xs = [hec.Ciphertext(ctx).fill_uniform(2, level, scale, 1000 + i) for i in range(B)]
    if name == "product":
        rk = ctx.relin_key(seed=99)
        ys = [hec.Ciphertext(ctx).fill_uniform(2, level, scale, 5000 + i) for i in range(B)]
        sides = {"batched": lambda: ctx.multiply_relin_rescale(xs, ys, rk),
                 "composed": lambda: [composed_product(ctx, rk, a, b) for a, b in zip(xs, ys)]}
    else:
        gk = ctx.galois_keys(uniform_elts=[ctx.elt_from_step(s) for s in hec.sum_elems_plan(DIM)], seed=77)

        def batched(mode):
            ctx.set_option("rot_add", mode)
            try:
                return ctx.sum_elems(xs, DIM, gk)
            finally:
                ctx.set_option("rot_add", 1)
        sides = {"batched": lambda: batched(1), "batched_rot_add0": lambda: batched(0),
                 "composed": lambda: [composed_sum(ctx, gk, x, DIM) for x in xs]}

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

    for fn in sides.values():  # warm-up of every side: workspace, buffers
        fn()
    times = {k: [] for k in sides}
    res = {}
    for _ in range(reps):  # alternated
        for k, fn in sides.items():
            res[k], ms = timed(fn)
            times[k].append(ms)
    ref = [(g.info(), g.download()) for g in res["composed"]]
    equal = all(g.info() == i and np.array_equal(g.download(), d)
                for k in sides if k != "composed" for g, (i, d) in zip(res[k], ref))
    out = {"case": name, "level": level, "B": B, "equal": bool(equal)}
    for k in sides:
        out[k] = stats(times[k])
    out["composed_over_batched"] = round(out["composed"]["ms"] / out["batched"]["ms"], 3)
    if name == "sum":
        out["rot_add0_over_rot_add1"] = round(out["batched_rot_add0"]["ms"] / out["batched"]["ms"], 4)
    del res, ref
    out["kernels"] = {}
    for k in [s for s in sides if s != "composed"]:  # separate profiled runs of the batched call
        ctx.profile(2)
        sides[k]()
        ctx.synchronize()
        kern = {}
        for cls in ctx.profile_classes():
            ms, scopes, nbytes, kl = ctx.profile_read_ex(cls)
            if cls.startswith("k:"):
                kern[cls] = {"ms": round(ms, 4), "scopes": scopes, "launches": kl,
                             "GBps": round(nbytes / (ms * 1e-3) / 1e9, 1) if ms and nbytes else None}
        ctx.profile(0)
        out["kernels"][k] = kern
    print("RESULT " + json.dumps(out))
    return 0 if out["equal"] else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--b", type=int, default=128)
    ap.add_argument("--reps", type=int, default=3, help="timed runs of each side, alternated (at least 3)")
    ap.add_argument("--limit", type=int, default=300, help="seconds a case may take")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--child", nargs=3, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    reps = max(3, args.reps)
    if args.child:
        return child(args.child[0], int(args.child[1]), int(args.child[2]), reps)
    result = {"N": 1 << 15, "moduli_bits": [60] + [40] * 9 + [60], "dim": DIM, "reps": reps, "cases": []}
    for B in (args.b, 1):
        for level in (10, 3):
            for name in ("sum", "product"):
                cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--reps",
                       str(reps), "--child", name, str(level), str(B)]
                p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
                lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
                if lines:
                    result["cases"].append(json.loads(lines[-1][7:]))
                if p.returncode != 0 or not lines:  # the first failure ends the run
                    print(json.dumps(result))
                    print("linalg_bench: case %s level %d B=%d failed (exit %d)" % (name, level, B, p.returncode),
                          file=sys.stderr)
                    return 1
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
