"""hec_matmul_diag_col_bsgs relinearises a tile's inner sums as one key switch over its GG Bc slots while that fits the
65,535 y-blocks of an NTT launch, GG Bc <= 65535 / ((l + 1) l), and one slot at a time past it.  The bit-exact suite
(tests/test_gpu_bsgs_ctct.py) runs at level 3, where the limit is thousands of columns, so it only sees the merged
branch.  Here level 10 puts the limit at 595: the default tile's 8 x 75 = 600 slots of a 75-column call exceed it
(one by one), and the same call in passes of 25 columns (8 x 25 = 200) merges.  Both must give the same words."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N11, BITS = 1 << 11, [60] + [40] * 9 + [60]
L, SCALE = 10, 2.0**40
n, bs, p = 6, 2, 75  # G = 3: steps 1 (baby), 2 and 4 (giants), all in the default key set


def test_one_by_one_relinearisation_equals_merged(hecdna):
    assert 8 * p > 65535 // ((L + 1) * L) >= 8 * 25
    ctx = hecdna.Context(N11, hecdna.create_coeff_modulus(N11, BITS))
    diags = [hecdna.Ciphertext(ctx).fill_uniform(2, L, SCALE, 30000 + j) for j in range(n)]
    cols = [hecdna.Ciphertext(ctx).fill_uniform(2, L, SCALE, 900 + i) for i in range(p)]
    rk = ctx.relin_key(seed=5)
    gk = ctx.galois_keys(uniform_elts=ctx.default_galois_elts(), seed=6)
    plain = ctx.matmul_diag_col_bsgs(diags, cols, rk, gk, bs=bs)
    ctx.set_option("bsgs_chunk", 25)
    try:
        chunked = ctx.matmul_diag_col_bsgs(diags, cols, rk, gk, bs=bs)
    finally:
        ctx.set_option("bsgs_chunk", 0)
    assert len(plain) == len(chunked) == p
    for a, b in zip(plain, chunked):
        assert a.info() == b.info() and np.array_equal(a.download(), b.download())
    ctx.close()
