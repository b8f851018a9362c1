"""Record the launch ledger tests/golden/launch_ledger.json: for a fixed list of engine calls, every profile class the
call touches with its number of scopes, its kernel launches and its algorithmic bytes.  The ledger is recorded at the
commit BEFORE a change that must not alter the launch sequence and checked after it (tests/test_gpu_launch_ledger.py).

Only the Python binding is used: the inputs and the keys come from the engine's uniform fills, so nothing is checked
about the words here.  Each call runs once unprofiled (the first-use tables are built), then once under profile(2).

Usage (on the GPU): python tests/golden/make_launch_ledger.py [--out tests/golden/launch_ledger.json]
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "launch_ledger.json")
sys.path.insert(0, os.path.join(HERE, ".."))

N = 1 << 11
BITS = [60, 40, 40, 40, 40, 60]
LEVEL = 4
SCALE = 2.0**40
STEPS = (1, 2, 4, 8, -1, -2, -4)


class Env:
    def __init__(self, hecdna):
        self.ctx = hecdna.Context(N, hecdna.create_coeff_modulus(N, BITS))
        self.rk = self.ctx.relin_key(seed=11)
        self.gk = self.ctx.galois_keys(uniform_elts=[self.ctx.elt_from_step(s) for s in STEPS], seed=5)
        self.seed = 100
        self.client = None

    def cts(self, count, level=LEVEL, size=2, scale=SCALE):
        out = []
        for _ in range(count):
            self.seed += 1
            out.append(self.ctx.ciphertext().fill_uniform(size, level, scale, self.seed))
        return out

    def pts(self, count, level=LEVEL, scale=SCALE):
        out = []
        for _ in range(count):
            self.seed += 1
            out.append(self.ctx.plaintext(None, scale).fill_uniform(level, scale, self.seed))
        return out

    def client_keys(self):
        """(sk, pk) of the client-half calls, generated once from fixed seeds on first use (outside any profile when
        the call's unprofiled run comes first, as record() runs it)"""
        if self.client is None:
            sk = self.ctx.keygen_secret(seed=_seed(1))
            self.client = (sk, self.ctx.keygen_public(sk, seed=_seed(2)))
        return self.client


def _seed(k):
    """a fixed 64-byte seed: the generating calls are pure functions of it, the uniform sampler's redraws included"""
    return [k, 2, 3, 4, 5, 6, 7, 8]


def _chunked(fn):
    def run(e):
        e.ctx.set_option("math_chunk", 2)
        try:
            fn(e)
        finally:
            e.ctx.set_option("math_chunk", 0)
    return run


def _bsgs_small(gg_option, fn):
    """the call with 2 giants per tile and 2 input vectors per pass: G = 3 in tiles {0, 1} and {2}, p = 3 in passes of
    2 and 1"""
    def run(e):
        e.ctx.set_option(gg_option, 2)
        e.ctx.set_option("bsgs_chunk", 2)
        try:
            fn(e)
        finally:
            e.ctx.set_option(gg_option, 8)
            e.ctx.set_option("bsgs_chunk", 0)
    return run


# n = 10, bs = 4: G = 3, step 3 is a NAF chain on the keys of STEPS; p = 3 leaves a partial batch group at BG = 2
def _bsgs_pt(e):
    e.ctx.matmul_diagpt_col_bsgs(e.pts(10), e.cts(3), e.gk, bs=4)


def _bsgs_ct(e):
    e.ctx.matmul_diag_col_bsgs(e.cts(10), e.cts(3), e.rk, e.gk, bs=4)


def _partial_finish(e):
    A, X = e.cts(10), e.cts(2)
    acc = e.ctx.matmul_diag_col_partial(A, 0, 10, X, e.gk)
    e.ctx.matmul_finish(acc, e.rk)


def _mixed_product(e):
    a = e.cts(2) + e.cts(1, level=3)
    b = e.cts(2) + e.cts(1, level=3)
    e.ctx.multiply_relin_rescale(a, b, e.rk)


def _square(e):
    a = e.cts(3)
    e.ctx.multiply_relin_rescale(a, a, e.rk)


# 3 columns, p = 5, bs = 2: G = 3, baby step 1, giants -2 and -4 (the natural form rotates by +2 and +4 as well), all of
# them keys of STEPS
def _cct(bsgs_form):
    def run(e):
        e.ctx.matmul_col_colT_bsgs(e.cts(3), e.cts(3), 5, e.rk, e.gk, bs=2, bsgs_form=bsgs_form)
    return run


def _jchunk2(fn):
    """the call in passes of 2 columns and 1 column: the assigning launch and the accumulating launch"""
    def run(e):
        e.ctx.set_option("cct_jchunk", 2)
        try:
            fn(e)
        finally:
            e.ctx.set_option("cct_jchunk", 0)
    return run


def _multiply(e):
    a, b = e.cts(2)
    e.ctx.multiply(a, b)


# The client half.  hec_encode and hec_encode_scalar record no profile class, so they have no entry here (the bit-exact
# suites carry them); every generating call takes a fixed seed
def _keygen_galois(e):
    sk, _ = e.client_keys()
    e.ctx.keygen_galois(sk, elts=[e.ctx.elt_from_step(1), e.ctx.elt_from_step(2)], seed=_seed(4))


def _decrypt(e):
    e.ctx.decrypt(e.client_keys()[0], e.cts(2))


def _decrypt_decode(e):
    e.ctx.decrypt_decode(e.client_keys()[0], e.cts(2), n_values=8)


def _encrypt_symmetric(e):
    e.ctx.encrypt_symmetric(e.client_keys()[0], e.pts(2), seed=_seed(5))


def _encrypt(e):
    e.ctx.encrypt(e.client_keys()[1], e.pts(2), seed=_seed(6))


# name -> call; the inputs are made inside the call (fills carry no profile scope)
CALLS = {
    "sum_elems_B3_dim7": lambda e: e.ctx.sum_elems(e.cts(3), 7, e.gk),
    "sum_elems_B3_dim8": lambda e: e.ctx.sum_elems(e.cts(3), 8, e.gk),
    "sum_elems_B1_dim1": lambda e: e.ctx.sum_elems(e.cts(1), 1, e.gk),
    "product_B3_levels_4_4_3": _mixed_product,
    "product_square_B3": _square,
    "product_square_B3_chunk2": _chunked(_square),
    "signed_inv_B2_iters1": lambda e: e.ctx.signed_inv(e.cts(2), 1.0, 1, e.rk),
    "signed_inv_B2_iters2": lambda e: e.ctx.signed_inv(e.cts(2), 1.0, 2, e.rk),
    "abs_B2_iters1": lambda e: e.ctx.abs(e.cts(2), 1.0, 1, e.rk),
    "drop_chain_levels_B2_by1": lambda e: e.ctx.drop_chain_levels(e.cts(2), 1),
    "fft_n4": lambda e: e.ctx.fft(e.cts(4)),
    "bfft_B2_n4_inverse": lambda e: e.ctx.bfft(e.cts(2), 4, e.gk, inverse=True),
    "matmul_diag_col_n10_p2": lambda e: e.ctx.matmul_diag_col(e.cts(10), e.cts(2), e.rk, e.gk),
    "matmul_partial_then_finish_n10_p2": _partial_finish,
    "matmul_col_colT_n6_p5": lambda e: e.ctx.matmul_col_colT(e.cts(6), e.cts(6), 5, e.rk, e.gk),
    "matrix_matmul_2x2": lambda e: e.ctx.matrix_matmul(e.cts(4), 2, 2, 0, e.cts(4), 2, 2, 0, e.rk),
    "relinearize_inplace": lambda e: e.ctx.relinearize(e.cts(1, size=3)[0], e.rk),
    "rescale_to_next_inplace": lambda e: e.ctx.rescale_to_next(e.cts(1)[0]),
    "bsgs_pt_n10_p3_bs4": _bsgs_pt,
    "bsgs_ct_n10_p3_bs4": _bsgs_ct,
    "bsgs_pt_n10_p3_bs4_gg2_chunk2": _bsgs_small("bsgs_gg", _bsgs_pt),
    "bsgs_ct_n10_p3_bs4_gg2_chunk2": _bsgs_small("bsgs_ct_gg", _bsgs_ct),
    "cct_bsgs_n3_p5_bs2_natural": _cct(False),
    "cct_bsgs_n3_p5_bs2_bsgs_form": _cct(True),
    "cct_bsgs_n3_p5_bs2_natural_jchunk2": _jchunk2(_cct(False)),
    "cct_bsgs_n3_p5_bs2_bsgs_form_jchunk2": _jchunk2(_cct(True)),
    "rotate_vector_step3_inplace": lambda e: e.ctx.rotate_vector(e.cts(1)[0], 3, e.gk),  # 3 = 4 - 1: a NAF chain
    "apply_galois_inplace": lambda e: e.ctx.apply_galois(e.cts(1)[0], e.ctx.elt_from_step(1), e.gk),
    # multiply and square carry no profile scope: their entries are empty and must stay so
    "multiply_inplace": _multiply,
    "square_inplace": lambda e: e.ctx.square(e.cts(1)[0]),
    # no communicator: the world of one, in this process (planner, partials, finish)
    "matmul_diag_col_sharded_world1_n10_p2": lambda e: e.ctx.matmul_diag_col_sharded(e.cts(10), e.cts(2), e.rk, e.gk),
    "keygen_secret": lambda e: e.ctx.keygen_secret(seed=_seed(1)),
    "keygen_public": lambda e: e.ctx.keygen_public(e.client_keys()[0], seed=_seed(2)),
    "keygen_relin": lambda e: e.ctx.keygen_relin(e.client_keys()[0], seed=_seed(3)),
    "keygen_galois_2elts": _keygen_galois,
    "encrypt_symmetric_B2": _encrypt_symmetric,
    "encrypt_B2": _encrypt,
    "decrypt_B2": _decrypt,
    "decode_B2_nv8": lambda e: e.ctx.decode(e.pts(2), n_values=8),
    "decrypt_decode_B2_nv8": _decrypt_decode,
}


def record(hecdna):
    """{call: {class: [scopes, kernel_launches, alg_bytes]}} on a fresh context"""
    e = Env(hecdna)
    ledger = {}
    for name, call in CALLS.items():
        call(e)
        e.ctx.profile(2)
        try:
            call(e)
            ledger[name] = {}
            for cls in e.ctx.profile_classes():
                _, scopes, nbytes, launches = e.ctx.profile_read_ex(cls)
                ledger[name][cls] = [scopes, launches, nbytes]
        finally:
            e.ctx.profile(0)
    e.ctx.close()
    return ledger


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=FIXTURE)
    args = ap.parse_args()
    import torch
    torch.cuda.is_available()  # one HIP runtime for torch and the engine (tests/conftest.py)
    from _helpers import load_hecdna
    led = record(load_hecdna())
    with open(args.out, "w") as f:
        json.dump(led, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(led)} calls, {sum(len(v) for v in led.values())} classes -> {args.out}")
