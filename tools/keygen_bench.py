#!/usr/bin/env python3
"""KeyGenerator / Encryptor on the GPU at cfg3's shape (N = 2^15, {60, 40 x 9, 60}): the default GaloisKeys set (29 keys
of 57.7 MB, 1.67 GB of RLWE samples), the relin key, and Encryptor::encrypt for a batch of 128 level-10 plaintexts.

Per case: the wall time of the C call (which ends in a stream synchronise) and the device time of its kernel classes
from HIP event pairs (profile mode 2: k:k_prng/*, k:k_sample/*, k:k_ntt/keygen, k:k_rlwe/*, ...), each class with its
algorithmic bytes and the GB/s they give.  For context only, the CPU oracle makes the same number of Galois keys on a
pool of 16 threads.  These are records, not thresholds.  Prints one JSON line.

    python tools/keygen_bench.py [--reps 3] [--oracle-keys 29] [--out profiles/keygen_bench.json]
"""
import argparse
import hashlib
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3, help="timed runs per case (the best wall time is reported)")
    ap.add_argument("--oracle-keys", type=int, default=29, help="Galois keys the CPU oracle makes (0: skip)")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()

    import torch
    torch.cuda.is_available()  # one HIP runtime for torch and the engine
    from _helpers import load_hecdna, load_oracle
    hec, orc = load_hecdna(), load_oracle()

    N, B, scale = 1 << 15, 128, 2.0**40
    bits = [60] + [40] * 9 + [60]
    moduli = hec.create_coeff_modulus(N, bits)
    K, L = len(moduli), len(moduli) - 1
    ctx = hec.Context(N, moduli)
    seed = lambda tag: hashlib.blake2b(tag.encode(), digest_size=64).digest()  # noqa: E731
    sk = ctx.keygen_secret(seed("bench sk"))
    pk = ctx.keygen_public(sk, seed("bench pk"))
    elts = ctx.default_galois_elts()
    key_bytes = L * 2 * K * N * 8

    def timed(fn, out_bytes):
        fn(0)  # warm-up: workspace, allocations
        best = None
        for r in range(args.reps):
            ctx.synchronize()
            t0 = time.perf_counter()
            fn(1 + r)
            ms = (time.perf_counter() - t0) * 1e3
            best = ms if best is None else min(best, ms)
        ctx.profile(2)
        fn(99)
        ctx.synchronize()
        classes = {}
        for cls in ctx.profile_classes():
            ms, scopes, nbytes, launches = ctx.profile_read_ex(cls)
            if cls.startswith("k:") and ms > 0:
                classes[cls] = {"ms": round(ms, 4), "launches": int(launches), "alg_bytes": int(nbytes),
                                "GBps": round(nbytes / (ms * 1e-3) / 1e9, 1)}
        ctx.profile(0)
        dev = sum(c["ms"] for c in classes.values())
        return {"wall_ms": round(best, 3), "device_ms": round(dev, 3), "output_bytes": out_bytes,
                "output_GBps_wall": round(out_bytes / (best * 1e-3) / 1e9, 2),
                "output_GBps_device": round(out_bytes / (dev * 1e-3) / 1e9, 2) if dev else None, "classes": classes}

    result = {"N": N, "moduli_bits": bits, "galois_keys": len(elts), "key_bytes": key_bytes,
              "timing": f"wall: best of {args.reps}, host clock around the call (ends in a stream synchronise); "
                        "device: HIP event pairs per kernel class, one further run"}
    result["keygen_galois_default"] = timed(lambda r: ctx.keygen_galois(sk, None, seed(f"gk {r}")), len(elts) * key_bytes)
    result["keygen_relin"] = timed(lambda r: ctx.keygen_relin(sk, seed(f"rk {r}")), key_bytes)
    rng = np.random.default_rng(0)
    pts = ctx.encode(rng.uniform(-1, 1, (B, N // 2)), scale)
    out = [hec.Ciphertext(ctx) for _ in range(B)]
    result["encrypt_B128"] = timed(lambda r: ctx.encrypt(pk, pts, seed(f"enc {r}"), out=out), B * 2 * L * N * 8)
    result["encrypt_B128"]["cts_per_s_wall"] = round(B / (result["encrypt_B128"]["wall_ms"] * 1e-3), 1)
    result["encrypt_symmetric_B128"] = timed(lambda r: ctx.encrypt_symmetric(sk, pts, seed(f"sym {r}"), out=out),
                                             B * 2 * L * N * 8)

    # a sanity check of what was timed: the last symmetric batch decrypts to its plaintexts' values
    got = ctx.decrypt_decode(sk, out[:2], real=True)
    exp = ctx.decode(pts[:2], real=True)
    result["decrypts"] = bool(np.max(np.abs(got - exp)) <= 21.5 * N / scale)

    if args.oracle_keys > 0:  # context only: the CPU oracle's keys on 16 threads of the same box
        o = orc.Oracle(N, moduli)
        sk_h = o.secret_key(7)
        k = min(args.oracle_keys, len(elts))
        t0 = time.perf_counter()
        with ThreadPoolExecutor(16) as pool:
            list(pool.map(lambda ie: o.galois_key(sk_h, ie[1], 100 + ie[0]), enumerate(elts[:k])))
        t = time.perf_counter() - t0
        result["oracle_galois_keys_16_threads"] = {"keys": k, "wall_ms": round(t * 1e3, 1)}
        result["gpu_over_oracle_galois"] = round(t * 1e3 / k * len(elts) / result["keygen_galois_default"]["wall_ms"], 1)

    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if result["decrypts"] else 1


if __name__ == "__main__":
    sys.exit(main())
