"""The decryption error of the baby-step giant-step matvec against the reference schedule's, on the CPU with the
oracle alone (no device): for five seeds, the max-abs error over the n output slots of the reference loop and of the
BSGS composition on the same matrix, vectors, keys and encryptions.
  --form pt   the oracle's matmul_diagpt_col_set against rotate, multiply_plain, add, rescale in the schedule's order;
              tests/test_gpu_bsgs.py bounds the GPU result's error by m times the reference schedule's
  --form ct   the oracle's matmul_diag_col against rotate, multiply, add, relinearize, rotate, add, rescale; the BSGS
              diagonals encrypt the rolled slot vectors with the seeds of the natural ones; tests/test_gpu_bsgs_ctct.py
              bounds the error likewise
m = twice the worst ratio printed here.

    python tools/bsgs_error.py --form pt  # N = 2^11, [50, 36, 36, 50], n = 24, bs = 8, p = 3, default Galois keys
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from _helpers import col_vector, diag_vectors, load_oracle  # noqa: E402

N, BITS, n, bs, p, SCALE = 1 << 11, [50, 36, 36, 50], 24, 8, 3, 2.0**40


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--form", choices=("ct", "pt"), required=True,
                    help="pt: plaintext diagonals, ct: ciphertext diagonals")
    ct = ap.parse_args().form == "ct"
    orc = load_oracle()
    m = orc.Oracle.create_coeff_modulus(N, BITS)
    o = orc.Oracle(N, m)
    L, slots = len(m) - 1, N // 2
    G = -(-n // bs)
    pairs = []
    for seed in range(5):
        rng = np.random.default_rng(100 + seed)
        sk = o.secret_key(seed + 1)
        rk = o.relin_key(sk, seed + 30) if ct else None
        gk = o.galois_keys(sk, o.default_galois_elts(), seed + 50)
        M = rng.uniform(-1, 1, (n, n))
        xs = rng.uniform(-1, 1, (p, n))
        D = diag_vectors(M, slots)
        X = [o.encrypt(sk, o.encode(col_vector(x, slots), SCALE, L), SCALE, 900 + 10 * seed + i)
             for i, x in enumerate(xs)]
        rolled = [np.roll(D[j], (j // bs) * bs) for j in range(n)]  # the BSGS form of the diagonals
        if ct:
            enc = lambda d, j: o.encrypt(sk, o.encode(d, SCALE, L), SCALE, 5000 + 100 * seed + j)  # noqa: E731
            Db = [enc(rolled[j], j) for j in range(n)]
            ref = o.matmul_diag_col([enc(D[j], j) for j in range(n)], X, rk, gk)
            term = lambda r, d: o.multiply(r, d)  # noqa: E731
        else:
            Db = [o.encode(d, SCALE, L) for d in rolled]
            ref = o.matmul_diagpt_col_set([o.encode(d, SCALE, L) for d in D], SCALE, list(range(n)), X, gk)
            term = lambda r, d: o.multiply_plain(r, d, SCALE)  # noqa: E731
        e_ref = e_bsgs = 0.0
        for i, x in enumerate(X):
            rots = [x] + [o.rotate(x, k, gk) for k in range(1, bs)]
            acc = None
            for g in range(G):
                inner = None
                for k in range(bs):
                    if g * bs + k >= n:
                        break
                    t = term(rots[k], Db[g * bs + k])
                    inner = t if inner is None else o.add(inner, t)
                r = o.relinearize(inner, rk) if ct else inner
                r = r if g == 0 else o.rotate(r, g * bs, gk)
                acc = r if acc is None else o.add(acc, r)
            out = o.rescale(acc)
            want = M @ xs[i]
            e_bsgs = max(e_bsgs, float(np.max(np.abs(o.decode(o.decrypt(sk, out), out.scale)[:n] - want))))
            e_ref = max(e_ref, float(np.max(np.abs(o.decode(o.decrypt(sk, ref[i]), ref[i].scale)[:n] - want))))
        pairs.append({"seed": seed, "reference": e_ref, "bsgs": e_bsgs, "ratio": e_bsgs / e_ref})
        print(json.dumps(pairs[-1]))
    worst = max(q["ratio"] for q in pairs)
    print(json.dumps({"worst_ratio": worst, "m": 2 * worst}))


if __name__ == "__main__":
    main()
