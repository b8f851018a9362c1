"""hec_sum_elems_plan (host only): the rotation steps of BatchedVector::sum_elems_inplace, against a restatement of
the rotations that the drop-in's own loop issues (cpp/src/he_linalg.cpp, sum_elems_inplace)."""
import pytest


def loop_rotations(dim):
    """every `<<` of the loop, in order; to_sum's in-place rotations are by `window`"""
    rot = []
    window = 1
    if dim & 1:
        rot.append(window)  # to_sum <<= window
    bits = dim >> 1
    while bits:
        window <<= 1
        if bits & 1:
            steps = window >> 1
            rot.append(steps)  # tmp = to_sum << steps
            steps >>= 1
            while steps:
                rot.append(steps)  # tmp = acc << steps
                steps >>= 1
            if bits != 1:
                rot.append(window)  # to_sum <<= window
        bits >>= 1
    return rot


@pytest.mark.parametrize("dim", list(range(1, 65)) + [4096])
def test_plan_equals_the_loop(hecdna, dim):
    assert hecdna.sum_elems_plan(dim) == loop_rotations(dim)


def test_known_plans(hecdna):
    assert hecdna.sum_elems_plan(8) == [4, 2, 1]
    assert hecdna.sum_elems_plan(4096) == [2048 >> k for k in range(12)]
    assert hecdna.sum_elems_plan(1) == [1]  # rotated once, the result discarded
    assert hecdna.sum_elems_plan(6) == [1, 2, 2, 1]


def test_dim_zero_raises(hecdna):
    with pytest.raises(hecdna.InvalidArgument, match="dim must be positive"):
        hecdna.sum_elems_plan(0)


def test_small_cap_reports_the_count(hecdna):
    """a buffer of 2 for the 4 steps of dim 6: the first two are written, the count is 4, the word behind the cap is
    untouched (the binding raises if it is not)"""
    assert hecdna.sum_elems_plan(6, cap=2) == ([1, 2], 4)
    assert hecdna.sum_elems_plan(6, cap=0) == ([], 4)
    assert hecdna.sum_elems_plan(6, cap=7) == ([1, 2, 2, 1], 4)
