"""hec_bsgs_plan and the BSGS form of the diagonals (host only, no device): the rotation steps the baby-step
giant-step ct x pt matvec issues, and the slot convention its plaintexts follow."""
import numpy as np
import pytest

from _helpers import col_vector, diag_vectors


def plan_ref(n, bs):
    """The definition restated: bs_eff = min(bs, n) (None: the smallest power of two >= sqrt(n)), the babies
    1 .. bs_eff - 1, then the giants g * bs_eff for 1 <= g < ceil(n / bs_eff)."""
    if bs is None:
        bs = 1
        while bs * bs < n:
            bs *= 2
    eff = min(bs, n)
    G = -(-n // eff)
    return eff, list(range(1, eff)) + [g * eff for g in range(1, G)]


@pytest.mark.parametrize("n,bs", [(1, 1), (24, 1), (24, 5), (24, 8), (24, 24), (24, 32), (4096, None), (4096, 64)])
def test_plan_matches_definition(hecdna, n, bs):
    assert hecdna.bsgs_plan(n, bs) == plan_ref(n, bs)


@pytest.mark.parametrize("bs", [None, 64])
def test_plan_cfg3_counts(hecdna, bs):
    eff, steps = hecdna.bsgs_plan(4096, bs)
    assert eff == 64 and len(steps) == 126 and len(set(steps)) == 126


def test_plan_errors(hecdna):
    with pytest.raises(hecdna.InvalidArgument):
        hecdna.bsgs_plan(0, 1)
    with pytest.raises(hecdna.InvalidArgument):
        hecdna.bsgs_plan(2048, 1025)
    assert hecdna.bsgs_plan(2048, 1024)[0] == 1024  # the cap itself is allowed
    assert hecdna.bsgs_plan(1000, 4096)[0] == 1000  # bs_eff, not bs, is what the cap bounds


@pytest.mark.parametrize("slots", [1008, 1024])
@pytest.mark.parametrize("bs", [1, 5, 8, 24])
def test_bsgs_diagonals_convention(hecdna, bs, slots):
    """sum_g roll(sum_i P'[g bs + i] * roll(x, -i), -g bs) is the slot-replicated M @ x.  Over 1,008 = 42 x 24 slots
    the replication is seamless and every slot equals M @ x.  24 does not divide 1,024 slots, so there the replication
    has a seam at the wrap: a slot s whose window s .. s + n - 1 crosses it reads x out of phase, under this schedule
    as under the reference loop's sum_j diag_j * roll(x, -j); M @ x is then compared on the slots whose window does
    not wrap.  Every slot is compared against the reference schedule in both cases."""
    n = 24
    rng = np.random.default_rng(11)
    M = rng.uniform(-1, 1, (n, n))
    x = rng.uniform(-1, 1, n)
    P = hecdna.bsgs_diagonals(np.stack(diag_vectors(M, slots)), bs)
    xs = col_vector(x, slots)
    eff, _ = hecdna.bsgs_plan(n, bs)
    acc = np.zeros(slots)
    for g in range(-(-n // eff)):
        inner = np.zeros(slots)
        for i in range(eff):
            if g * eff + i < n:
                inner += P[g * eff + i] * np.roll(xs, -i)
        acc += np.roll(inner, -g * eff)
    whole = slots if slots % n == 0 else slots - n + 1
    assert np.max(np.abs(acc - col_vector(M @ x, slots))[:whole]) < 1e-9
    D = diag_vectors(M, slots)
    assert np.max(np.abs(acc - sum(D[j] * np.roll(xs, -j) for j in range(n)))) < 1e-9
