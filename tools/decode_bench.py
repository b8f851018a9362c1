#!/usr/bin/env python3
"""The client half on the GPU: decrypt + decode throughput (hec_decrypt_decode) at cfg3's output shape, N = 2^15,
level 9, size 2, for batches of 1 and 128, in one process and run.

Per case: wall time of the whole C call hec_decrypt_decode into preallocated host arrays (pointer lists up, k_decrypt,
inverse NTT, CRT + transform, gather, slots back to the host; the Python binding's own wall time, which also
allocates and assembles the complex array, is given beside it), the device time of its two phases (profile classes
dec_decrypt / dec_decode), ciphertexts/s, and the achieved GB/s on the compulsory bytes, 2 level N 8 read + (N/2) 16 written per ciphertext.  The CPU oracle's
decode(decrypt()) is timed for the same inputs on the same box, and its slots are the check: the GPU's must lie
within the tolerance of tests/test_gpu_decode.py.  Also records whether one batch of 128 beats 128 single calls per
ciphertext.  No figure is fixed in advance.  Prints one JSON line.

    python tools/decode_bench.py [--reps 5] [--oracle-cts 4] [--out profiles/decode_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="timed runs per case (the best is reported)")
    ap.add_argument("--oracle-cts", type=int, default=4, help="ciphertexts the CPU oracle decrypts and decodes")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()

    import ctypes as C

    import torch
    torch.cuda.is_available()  # one HIP runtime for torch and the engine
    from _helpers import load_hecdna, load_oracle
    hec, orc = load_hecdna(), load_oracle()

    N, level, scale, B = 1 << 15, 9, 2.0**40, 128
    bits = [60] + [40] * 9 + [60]
    moduli = hec.create_coeff_modulus(N, bits)
    ctx = hec.Context(N, moduli)
    o = orc.Oracle(N, moduli)
    sk_h = o.secret_key(2024)
    sk = ctx.secret_key(sk_h)
    # uniform synthetic ciphertexts (RLWE ciphertexts are pseudo-uniform): the decoded values are of order Q / scale,
    # which changes no instruction count
    cts = [hec.Ciphertext(ctx).fill_uniform(2, level, scale, 9000 + i) for i in range(B)]
    bytes_per_ct = 2 * level * N * 8 + (N // 2) * 16

    def wall(fn):
        ctx.synchronize()
        t0 = time.perf_counter()
        res = fn()
        return res, (time.perf_counter() - t0) * 1e3

    def device_ms(fn):
        ctx.profile(2)
        fn()
        ctx.synchronize()
        out = {cls: round(ctx.profile_read_ex(cls)[0], 4) for cls in ("dec_decrypt", "dec_decode")}
        ctx.profile(0)
        return out

    def case(batch):
        n, nv = len(batch), N // 2
        re, im = np.zeros((n, nv)), np.zeros((n, nv))
        arr = (C.c_void_p * n)(*[c.h.value for c in batch])
        dp = C.POINTER(C.c_double)

        def fn():
            hec._check(hec.lib().hec_decrypt_decode(ctx.h, sk.h, arr, n, nv, re.ctypes.data_as(dp),
                                                    im.ctypes.data_as(dp)))
        fn()  # warm-up: workspace, decoder tables
        best, bind = None, None
        for _ in range(args.reps):
            _, ms = wall(fn)
            best = ms if best is None else min(best, ms)
            res, ms = wall(lambda: ctx.decrypt_decode(sk, batch))
            bind = ms if bind is None else min(bind, ms)
        assert np.array_equal(res.real, re) and np.array_equal(res.imag, im)
        dev = device_ms(fn)
        dev_total = sum(dev.values())
        return res, {"batch": n, "wall_ms": round(best, 3), "binding_wall_ms": round(bind, 3),
                     "cts_per_s": round(n / (best * 1e-3), 1),
                     "GBps_wall": round(n * bytes_per_ct / (best * 1e-3) / 1e9, 2), "device_ms": dev,
                     "cts_per_s_device": round(n / (dev_total * 1e-3), 1),
                     "GBps_device": round(n * bytes_per_ct / (dev_total * 1e-3) / 1e9, 2)}

    result = {"N": N, "moduli_bits": bits, "level": level, "size": 2, "bytes_per_ciphertext": bytes_per_ct,
              "timing": f"best of {args.reps}: host clock around the call, which ends in a stream synchronise"}
    one, result["batch_1"] = case(cts[:1])
    many, result["batch_128"] = case(cts)
    # 128 single calls against one call of 128, both through the binding
    _, singles_ms = wall(lambda: [ctx.decrypt_decode(sk, [c]) for c in cts])
    result["singles_128_wall_ms"] = round(singles_ms, 3)
    result["batch_128_over_singles"] = round(singles_ms / result["batch_128"]["binding_wall_ms"], 2)
    result["batch_128_beats_128_singles"] = bool(result["batch_128"]["binding_wall_ms"] < singles_ms)
    assert np.array_equal(one[0], many[0])

    # the oracle on the same inputs, same box: time and check
    u = 2.0**-53
    k = max(1, min(args.oracle_cts, B))
    worst, t_orc = 0.0, 0.0
    for i in range(k):
        ct = orc.Ct(cts[i].download(), scale)
        t0 = time.perf_counter()
        ref = o.decode(o.decrypt(sk_h, ct), scale)
        t_orc += time.perf_counter() - t0
        tol = (10 * np.log2(N) + 16) * u * np.sqrt(2 * np.sum(np.abs(ref) ** 2))
        worst = max(worst, float(np.linalg.norm(many[i] - ref) / tol))
    result["oracle"] = {"ciphertexts": k, "ms_per_ciphertext": round(t_orc / k * 1e3, 2),
                        "cts_per_s": round(k / t_orc, 2)}
    result["gpu_batch_128_over_oracle"] = round(result["batch_128"]["cts_per_s"] / result["oracle"]["cts_per_s"], 1)
    result["max_error_over_tol"] = round(worst, 4)
    result["within_tolerance"] = bool(worst <= 1.0)

    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if result["within_tolerance"] else 1


if __name__ == "__main__":
    sys.exit(main())
