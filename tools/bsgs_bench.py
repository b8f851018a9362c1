#!/usr/bin/env python3
"""The baby-step giant-step matvec against the reference schedule at cfg3: N = 2^15, {60, 40 x 9, 60}, level 10,
n = 4096, scale 2^40, on uniform synthetic diagonals, ciphertexts and keys.  --form pt: hec_matmul_diagpt_col_bsgs
against hec_matmul_diagpt_col (plaintext diagonals); --form ct: hec_matmul_diag_col_bsgs against hec_matmul_diag_col
(ciphertext diagonals, a relinearisation key).  Sides, all in one process, alternated, timed with HIP events on the
context's stream after a warm-up of every side:
  bsgs32 / bsgs64 / bsgs128 [/ bsgs256 for ct]   that bs with a Galois key for every planned step
  bsgs64_default                                  bs = 64 on the default (power-of-two) key set: NAF chains
  reference                                       the reference schedule on the default key set
The sides do not share their ciphertext bits (tests/test_gpu_bsgs.py and tests/test_gpu_bsgs_ctct.py check each against
the oracle), so nothing is compared here but the tile variants of the form's inner-sum kernel with the default tile,
word for word on three outputs.
Prints one JSON line: matvec/s per side (median of the repetitions, spread = (max - min) / median), the key switches
per input vector from the plans (ct: rotations + relinearisations), the per-class table of bs = 64 from a separate
profiled run (each kernel class's ms, GB/s on its algorithmic bytes and share of the call; ct: also the inner and
relinearisation scopes), and the inner-sum kernel's time per tile (options "bsgs_bg", "bsgs_gg" or "bsgs_ct_bg",
"bsgs_ct_gg", and "bsgs_order") from profiled runs of their own.

    python tools/bsgs_bench.py --form pt [--b 128] [--n 4096] [--reps 3] [--out profiles/bsgs_bench.json]
    python tools/bsgs_bench.py --form ct [--b 128] [--n 4096] [--reps 3] [--out profiles/bsgs_ctct_bench.json]

--form colcolT: hec_matmul_col_colT_bsgs against hec_matmul_col_colT for n columns and p = n output diagonals at the
default bs, on uniform synthetic ciphertexts and keys.  Sides: both output forms with a Galois key per planned step and
on the default key set (--jchunk: in passes of that many columns), and the comparator on the default key set
(--no-reference leaves it out: its one key switch
over all n columns takes at most 65,535 / (l (l + 1)) of them, 595 at level 10).  Prints one JSON line: ms per side
(median, spread), the key switches of each side from the plans, the per-class table of the form-1 call from a profiled
run, and k_colcolt_inner's time per tile (options "cct_tb", "cct_tg", "bsgs_order").  --append adds the line to --out.

    python tools/bsgs_bench.py --form colcolT --n 256 [--reps 3] [--out profiles/colcolt_bsgs_bench.json --append]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

N, BITS, SCALE = 1 << 15, [60] + [40] * 9 + [60], 2.0**40
# per form: the log prefix, the block sizes, the inner-sum kernel, the tile options and the tiles (bg, gg, order), the
# default tile first
FORMS = {
    "pt": dict(tag="bsgs_bench", block_sizes=(32, 64, 128), kernel="k_bsgs_inner",
               opts=("bsgs_bg", "bsgs_gg", "bsgs_order"),
               tiles=[(2, 8, 1), (2, 8, 0), (2, 4, 1), (2, 2, 1), (1, 8, 1), (4, 4, 1), (4, 8, 1)]),
    "ct": dict(tag="bsgs_ctct_bench", block_sizes=(32, 64, 128, 256), kernel="k_bsgs_inner_ct",
               opts=("bsgs_ct_bg", "bsgs_ct_gg", "bsgs_order"),
               tiles=[(2, 8, 1), (2, 8, 0), (2, 4, 1), (2, 2, 1), (1, 2, 1), (1, 4, 1), (1, 8, 1)]),
}


def default_key_switches(n, bs):
    """Rotation key switches per input vector on the default key set: the distinct prefixes of the babies' NAF chains
    (the rotation trie) and every element of the giants' chains."""
    from _helpers import rotation_seq
    pre = set()
    for i in range(1, min(bs, n)):
        s = tuple(rotation_seq(N, i))
        pre |= {s[:k] for k in range(1, len(s) + 1)}
    eff = min(bs, n)
    return len(pre) + sum(len(rotation_seq(N, g * eff)) for g in range(1, -(-n // eff)))


def step_seq(step):
    """SEAL's key-switch sequence for rotate(x, step) under the default Galois keys, negative steps included: one key
    for +-2^i, else the NAF terms least significant first, +-N/2 skipped"""
    v = abs(step)
    if v & (v - 1) == 0:
        return [step] if step else []
    res, i = [], 0
    while v:
        z = (2 - (v & 3)) if v & 1 else 0
        v = (v - z) >> 1
        if z and abs(z << i) != N // 2:
            res.append((-z if step < 0 else z) << i)
        i += 1
    return res


def trie_nodes(steps):
    """key switches of the rotation prefix trie over these steps on the default key set"""
    pre = set()
    for st in steps:
        q = tuple(step_seq(st))
        pre |= {q[:k] for k in range(1, len(q) + 1)}
    return len(pre)


def colcolt_main(args):
    tag, kernel, opts = "colcolt_bsgs_bench", "k_colcolt_inner", ("cct_tb", "cct_tg", "bsgs_order")
    tiles = [(4, 2, 1), (4, 2, 0), (2, 4, 1), (4, 4, 1), (2, 2, 1), (1, 4, 1), (4, 1, 1), (1, 1, 1)]
    reps, n = max(3, args.reps), args.n
    p = n
    import torch
    if not torch.cuda.is_available():
        print(f"{tag}: no GPU", file=sys.stderr)
        return 1
    from _helpers import load_hecdna
    hec = load_hecdna()
    ctx = hec.Context(N, hec.create_coeff_modulus(N, BITS))
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    ctx.set_option("cct_jchunk", args.jchunk)
    L = len(BITS) - 1
    A = [hec.Ciphertext(ctx).fill_uniform(2, L, SCALE, 20000 + j) for j in range(n)]
    Bc = [hec.Ciphertext(ctx).fill_uniform(2, L, SCALE, 40000 + j) for j in range(n)]
    bs, steps0 = hec.colcolT_bsgs_plan(p, None, 0)
    _, steps1 = hec.colcolT_bsgs_plan(p, None, 1)
    G = -(-p // bs)
    gk_steps = ctx.galois_keys(uniform_elts=[ctx.elt_from_step(st) for st in steps0], seed=77)
    gk_def = ctx.galois_keys(uniform_elts=ctx.default_galois_elts(), seed=78)
    rk = ctx.relin_key(seed=79)
    outs = {}

    def side(name, fn):
        outs[name] = [hec.Ciphertext(ctx) for _ in range(p)]
        return lambda: fn(outs[name])

    sides, ks = {}, {}
    for form in (0, 1):
        for kname, gk in (("steps", gk_steps), ("default", gk_def)):
            name = f"bsgs_form{form}_{kname}"
            sides[name] = side(name, lambda o, gk=gk, form=form: ctx.matmul_col_colT_bsgs(A, Bc, p, rk, gk,
                                                                                          bsgs_form=form, out=o))
            if kname == "steps":
                rot = n * ((bs - 1) + (G - 1)) + (p - bs if form == 0 else 0)
            else:
                rot = n * (trie_nodes(range(bs)) + trie_nodes([-g * bs for g in range(G)]))
                if form == 0:
                    rot += sum(len(step_seq(g * bs)) * min(bs, p - g * bs) for g in range(1, G))
            ks[name] = {"rotations": rot, "relinearisations": p}
    if not args.no_reference:
        sides["reference"] = side("reference", lambda o: ctx.matmul_col_colT(A, Bc, p, rk, gk_def))
        ks["reference"] = {"rotations": n * trie_nodes(range(p)), "relinearisations": p}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ctx.synchronize()
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    for k, fn in sides.items():  # warm-up of every side: workspace, output buffers, per-key tables
        fn()
        ctx.synchronize()
        print(f"{tag}: warmed {k}", file=sys.stderr, flush=True)
    times = {k: [] for k in sides}
    for _ in range(reps):  # alternated
        for k, fn in sides.items():
            times[k].append(timed(fn))
            print(f"{tag}: {k} {times[k][-1]:.1f} ms", file=sys.stderr, flush=True)
    result = {"form": "colcolT", "N": N, "moduli_bits": BITS, "level": L, "n": n, "p": p, "bs": bs, "G": G,
              "cct_jchunk": args.jchunk, "reps": reps, "sides": {}}
    for k, ms in times.items():
        med = float(np.median(ms))
        result["sides"][k] = {"ms": round(med, 2), "spread": round((max(ms) - min(ms)) / med, 4),
                              "runs_ms": [round(v, 2) for v in ms], "key_switches": ks[k]}
    if "reference" in sides:
        ref = result["sides"]["reference"]["ms"]
        for k in sides:
            result["sides"][k]["speedup_over_reference"] = round(ref / result["sides"][k]["ms"], 2)

    def profiled(fn):
        ctx.profile(2)
        ms = timed(fn)
        tab = {cls: ctx.profile_read_ex(cls) for cls in ctx.profile_classes()}
        ctx.profile(0)
        return ms, tab

    main_side = "bsgs_form1_steps"
    call_ms, tab = profiled(sides[main_side])
    result["form1_classes"] = {"call_ms": round(call_ms, 2), "kernels": {
        cls: {"ms": round(ms, 3), "launches": kl, "share": round(ms / call_ms, 4),
              "GBps": round(nb / (ms * 1e-3) / 1e9, 1) if ms and nb else None}
        for cls, (ms, _scopes, nb, kl) in sorted(tab.items()) if cls.startswith("k:")},
        "scopes": {cls: round(tab[cls][0], 3) for cls in ("cct_inner", "cct_relin", "cct_giants") if cls in tab}}
    idx = (0, p // 2, p - 1)
    want = [outs[main_side][i].download() for i in idx]
    result["tiles"], equal = [], True
    for tile in ([] if args.no_tiles else tiles):
        for k, v in zip(opts, tile):
            ctx.set_option(k, v)
        runs = []
        for _ in range(reps):
            ms_call, t = profiled(sides[main_side])
            ms, _scopes, nb, kl = t["k:" + kernel]
            runs.append((ms, nb, kl, ms_call))
        ms, nb, kl, ms_call = sorted(runs)[len(runs) // 2]
        equal = equal and all(np.array_equal(outs[main_side][i].download(), w) for i, w in zip(idx, want))
        print(f"{tag}: tile {tile[0]}x{tile[1]} order {tile[2]}: {kernel} {ms:.2f} ms", file=sys.stderr, flush=True)
        result["tiles"].append({"tb": tile[0], "tg": tile[1], "order": tile[2], kernel + "_ms": round(ms, 3),
                                "launches": kl, "GBps": round(nb / (ms * 1e-3) / 1e9, 1), "call_ms": round(ms_call, 2),
                                "spread": round((max(r[0] for r in runs) - min(r[0] for r in runs)) / ms, 4)})
    for k, v in zip(opts, tiles[0]):
        ctx.set_option(k, v)
    result["tiles_equal"] = bool(equal)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "a" if args.append else "w") as f:
            f.write(line + "\n")
    return 0 if equal else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--form", choices=sorted(FORMS) + ["colcolT"], required=True,
                    help="pt: plaintext diagonals, ct: ciphertext diagonals, colcolT: the col x col^T product")
    ap.add_argument("--b", type=int, default=128, help="input vectors per call")
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=3, help="timed runs of each side, alternated (at least 3)")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--append", action="store_true", help="colcolT: append to --out")
    ap.add_argument("--no-reference", action="store_true", help="colcolT: leave hec_matmul_col_colT out")
    ap.add_argument("--no-tiles", action="store_true", help="colcolT: leave the tile A/B out")
    ap.add_argument("--jchunk", type=int, default=0, help="colcolT: option \"cct_jchunk\", columns per pass (0 automatic)")
    args = ap.parse_args()
    if args.form == "colcolT":
        return colcolt_main(args)
    reps, B, n = max(3, args.reps), args.b, args.n
    ct = args.form == "ct"
    form = FORMS[args.form]
    tag, block_sizes, kernel, opts, tiles = (form[k] for k in ("tag", "block_sizes", "kernel", "opts", "tiles"))

    import torch
    if not torch.cuda.is_available():  # one HIP runtime for torch and the engine; no device, no measurement
        print(f"{tag}: no GPU", file=sys.stderr)
        return 1
    from _helpers import load_hecdna, rotation_trie_stats
    hec = load_hecdna()
    ctx = hec.Context(N, hec.create_coeff_modulus(N, BITS))
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    L = len(BITS) - 1
    if ct:
        diags = [hec.Ciphertext(ctx).fill_uniform(2, L, SCALE, 20000 + j) for j in range(n)]
    else:
        diags = [hec.Plaintext(ctx, None, SCALE).fill_uniform(L, SCALE, 20000 + j) for j in range(n)]
    xs = [hec.Ciphertext(ctx).fill_uniform(2, L, SCALE, 1000 + i) for i in range(B)]
    steps = sorted({s for bs in block_sizes for s in hec.bsgs_plan(n, bs)[1]})
    gk_steps = ctx.galois_keys(uniform_elts=[ctx.elt_from_step(s) for s in steps], seed=77)  # a key per step of all
    gk_def = ctx.galois_keys(uniform_elts=ctx.default_galois_elts(), seed=78)
    if ct:
        rk = ctx.relin_key(seed=79)
        bsgs = lambda gk, bs, o: ctx.matmul_diag_col_bsgs(diags, xs, rk, gk, bs=bs, out=o)  # noqa: E731
        reference = lambda o: ctx.matmul_diag_col(diags, xs, rk, gk_def, out=o)  # noqa: E731
    else:
        bsgs = lambda gk, bs, o: ctx.matmul_diagpt_col_bsgs(diags, xs, gk, bs=bs, out=o)  # noqa: E731
        reference = lambda o: ctx.matmul_diagpt_col(diags, xs, gk_def, out=o)  # noqa: E731
    outs = {}  # every side writes into its own outputs: no allocation in the timed calls

    def side(name, fn):
        outs[name] = [hec.Ciphertext(ctx) for _ in range(B)]
        return lambda: fn(outs[name])

    sides = {f"bsgs{bs}": side(f"bsgs{bs}", lambda o, bs=bs: bsgs(gk_steps, bs, o)) for bs in block_sizes}
    sides["bsgs64_default"] = side("bsgs64_default", lambda o: bsgs(gk_def, 64, o))
    sides["reference"] = side("reference", reference)
    # ct: one relinearisation per giant group on top of the rotations, one for the reference
    relins = (lambda bs: -(-n // min(bs, n))) if ct else (lambda bs: 0)
    ks = {f"bsgs{bs}": len(hec.bsgs_plan(n, bs)[1]) + relins(bs) for bs in block_sizes}
    ks["bsgs64_default"] = default_key_switches(n, 64) + relins(64)
    ks["reference"] = rotation_trie_stats(N, n)[0] + (1 if ct else 0)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ctx.synchronize()
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    for k, fn in sides.items():  # warm-up of every side: workspace, output buffers, per-key tables
        fn()
        ctx.synchronize()
        print(f"{tag}: warmed {k}", file=sys.stderr, flush=True)
    times = {k: [] for k in sides}
    for _ in range(reps):  # alternated
        for k, fn in sides.items():
            times[k].append(timed(fn))
            print(f"{tag}: {k} {times[k][-1]:.1f} ms", file=sys.stderr, flush=True)
    result = {"N": N, "moduli_bits": BITS, "level": L, "n": n, "B": B, "reps": reps, "sides": {}}
    for k, ms in times.items():
        med = float(np.median(ms))
        result["sides"][k] = {"ms": round(med, 2), "matvec_per_s": round(B / (med * 1e-3), 2),
                              "spread": round((max(ms) - min(ms)) / med, 4), "runs_ms": [round(v, 2) for v in ms],
                              "key_switches": ks[k]}
    ref = result["sides"]["reference"]["matvec_per_s"]
    for k in sides:
        result["sides"][k]["over_reference"] = round(result["sides"][k]["matvec_per_s"] / ref, 2)

    def profiled(fn):
        """A run of its own under the asynchronous profile: (call ms, {class: (ms, scopes, bytes, launches)})."""
        ctx.profile(2)
        ms = timed(fn)
        tab = {cls: ctx.profile_read_ex(cls) for cls in ctx.profile_classes()}
        ctx.profile(0)
        return ms, tab

    call_ms, tab = profiled(sides["bsgs64"])
    result["bsgs64_classes"] = {"call_ms": round(call_ms, 2), "kernels": {
        cls: {"ms": round(ms, 3), "launches": kl, "share": round(ms / call_ms, 4),
              "GBps": round(nb / (ms * 1e-3) / 1e9, 1) if ms and nb else None}
        for cls, (ms, _scopes, nb, kl) in sorted(tab.items()) if cls.startswith("k:")}}
    if ct:
        result["bsgs64_classes"]["scopes"] = {cls: round(tab[cls][0], 3) for cls in ("bsgs_inner_ct", "bsgs_relin")
                                              if cls in tab}

    # the inner-sum kernel per tile at bs = 64, and the outputs of every tile against the default tile's
    want = [outs["bsgs64"][i].download() for i in (0, B // 2, B - 1)]
    result["tiles"], equal = [], True
    for tile in tiles:
        for k, v in zip(opts, tile):
            ctx.set_option(k, v)
        sides["bsgs64"]()  # warm-up: the tile changes the workspace
        runs = []
        for _ in range(reps):
            ms_call, t = profiled(sides["bsgs64"])
            ms, _scopes, nb, kl = t["k:" + kernel]
            runs.append((ms, nb, kl, ms_call))
        ms, nb, kl, ms_call = sorted(runs)[len(runs) // 2]
        equal = equal and all(np.array_equal(outs["bsgs64"][i].download(), w) for i, w in zip((0, B // 2, B - 1), want))
        print(f"{tag}: tile {tile[0]}x{tile[1]} order {tile[2]}: {kernel} {ms:.2f} ms", file=sys.stderr, flush=True)
        result["tiles"].append({"bg": tile[0], "gg": tile[1], "order": tile[2], kernel + "_ms": round(ms, 3),
                                "launches": kl, "GBps": round(nb / (ms * 1e-3) / 1e9, 1), "call_ms": round(ms_call, 2),
                                "spread": round((max(r[0] for r in runs) - min(r[0] for r in runs)) / ms, 4)})
    for k, v in zip(opts, tiles[0]):
        ctx.set_option(k, v)
    result["tiles_equal"] = bool(equal)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if equal else 1


if __name__ == "__main__":
    sys.exit(main())
