"""The decryption error of the baby-step giant-step matvec against the reference schedule's, on the CPU with the
oracle alone (no device): for five seeds, the max-abs error over the n output slots of the reference loop and of the
BSGS composition on the same matrix, vectors, keys and encryptions.
  --form pt   the oracle's matmul_diagpt_col_set against rotate, multiply_plain, add, rescale in the schedule's order;
              tests/test_gpu_bsgs.py bounds the GPU result's error by m times the reference schedule's
  --form ct   the oracle's matmul_diag_col against rotate, multiply, add, relinearize, rotate, add, rescale; the BSGS
              diagonals encrypt the rolled slot vectors with the seeds of the natural ones; tests/test_gpu_bsgs_ctct.py
              bounds the error likewise
  --form colcolT  the col x col^T product of hec_matmul_col_colT_bsgs at the shape of tests/test_gpu_colcolt_bsgs.py
              (n = 6 columns, p = 11 outputs, bs = 4), two ratios per seed: (a) the composition of its
              definition against the oracle's matmul_col_colT, for both output forms, the max-abs error over the p
              outputs and all slots; (b) the chain "form-1 output -> BSGS ct x ct matvec" against "matmul_col_colT ->
              matmul_diag_col" for a d = 8 matrix and two vectors
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


def colcolt_compose(o, A, B, p_, bs_, form, rk, gk):
    """hec_matmul_col_colT_bsgs's definition from the oracle's operations"""
    G_ = -(-p_ // bs_)
    Bb = [[b] + [o.rotate(b, k, gk) for k in range(1, bs_)] for b in B]
    Ag = [[a] + [o.rotate(a, -g * bs_, gk) for g in range(1, G_)] for a in A]
    outs = []
    for i in range(p_):
        g, b = divmod(i, bs_)
        acc = None
        for j in range(len(A)):
            t = o.multiply(Bb[j][b], Ag[j][g])
            acc = t if acc is None else o.add(acc, t)
        r = o.rescale(o.relinearize(acc, rk))
        outs.append(o.rotate(r, g * bs_, gk) if form == 0 and g else r)
    return outs


def matvec_compose(o, D, X, bs_, rk, gk):
    """hec_matmul_diag_col_bsgs's definition from the oracle's operations (D in BSGS form)"""
    G_ = -(-len(D) // bs_)
    outs = []
    for x in X:
        rots = [x] + [o.rotate(x, k, gk) for k in range(1, bs_)]
        acc = None
        for g in range(G_):
            inner = None
            for k in range(bs_):
                if g * bs_ + k >= len(D):
                    break
                t = o.multiply(rots[k], D[g * bs_ + k])
                inner = t if inner is None else o.add(inner, t)
            r = o.relinearize(inner, rk)
            r = r if g == 0 else o.rotate(r, g * bs_, gk)
            acc = r if acc is None else o.add(acc, r)
        outs.append(o.rescale(acc))
    return outs


def colcolt(o, L, slots):
    cn, cp, cbs, d, sc2 = 6, 11, 4, 8, 2.0**36
    rows = []
    for seed in range(5):
        rng = np.random.default_rng(300 + seed)
        sk = o.secret_key(seed + 1)
        rk = o.relin_key(sk, seed + 30)
        gk = o.galois_keys(sk, o.default_galois_elts(), seed + 50)
        err = lambda ct, want: float(np.max(np.abs(o.decode(o.decrypt(sk, ct), ct.scale)[:len(want)] - want)))  # noqa: E731
        a = rng.uniform(-1, 1, (cn, slots))
        b = rng.uniform(-1, 1, (cn, slots))
        A = [o.encrypt(sk, o.encode(a[j], SCALE, L), SCALE, 7000 + 100 * seed + j) for j in range(cn)]
        B = [o.encrypt(sk, o.encode(b[j], SCALE, L), SCALE, 7050 + 100 * seed + j) for j in range(cn)]
        want = [sum(np.roll(b[j], -i) * a[j] for j in range(cn)) for i in range(cp)]
        ref = o.matmul_col_colT(A, B, cp, rk, gk)
        e_ref = max(err(ref[i], want[i]) for i in range(cp))
        row = {"seed": seed, "reference": e_ref}
        for form in (0, 1):
            out = colcolt_compose(o, A, B, cp, cbs, form, rk, gk)
            w = want if form == 0 else [np.roll(want[i], (i // cbs) * cbs) for i in range(cp)]
            e_b = max(err(out[i], w[i]) for i in range(cp))
            row[f"bsgs_form{form}"] = e_b
            row[f"ratio_a_form{form}"] = e_b / e_ref
        # (b) the chain: the columns of a d x d matrix as A = B, then the matvec with two vectors at level L - 1
        M = rng.uniform(-1, 1, (d, d))
        xs = rng.uniform(-1, 1, (2, d))
        cols = [o.encrypt(sk, o.encode(col_vector(M[:, j], slots), sc2, L), sc2, 7500 + 100 * seed + j)
                for j in range(d)]
        X = [o.encrypt(sk, o.encode(col_vector(x, slots), sc2, L - 1), sc2, 7600 + 100 * seed + i)
             for i, x in enumerate(xs)]
        chain = matvec_compose(o, colcolt_compose(o, cols, cols, d, cbs, 1, rk, gk), X, cbs, rk, gk)
        chain_ref = o.matmul_diag_col(o.matmul_col_colT(cols, cols, d, rk, gk), X, rk, gk)
        wants = [M @ M.T @ x for x in xs]
        row["chain_reference"] = max(err(chain_ref[i], wants[i]) for i in range(2))
        row["chain_bsgs"] = max(err(chain[i], wants[i]) for i in range(2))
        row["ratio_b"] = row["chain_bsgs"] / row["chain_reference"]
        rows.append(row)
        print(json.dumps(row))
    worst_a = max(max(r["ratio_a_form0"], r["ratio_a_form1"]) for r in rows)
    worst_b = max(r["ratio_b"] for r in rows)
    print(json.dumps({"worst_ratio_a": worst_a, "m_a": 2 * worst_a, "worst_ratio_b": worst_b, "m_b": 2 * worst_b}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--form", choices=("ct", "pt", "colcolT"), required=True,
                    help="pt: plaintext diagonals, ct: ciphertext diagonals, colcolT: the col x col^T product")
    form = ap.parse_args().form
    ct = form == "ct"
    orc = load_oracle()
    m = orc.Oracle.create_coeff_modulus(N, BITS)
    o = orc.Oracle(N, m)
    L, slots = len(m) - 1, N // 2
    if form == "colcolT":
        return colcolt(o, L, slots)
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
