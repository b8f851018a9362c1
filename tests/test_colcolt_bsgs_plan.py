"""hec_colcolT_bsgs_plan and hec_matmul_col_colT_bsgs at the drop-in boundary (host only, no device): the rotation
steps the baby-step giant-step col x col^T product issues for each output form, the planner's cap / count convention
and errors, and the C, Python and C++ surfaces over the two entries."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest


def plan_ref(p, bs, form):
    """The definition restated: bs_eff = min(bs, p) (None: the smallest power of two >= sqrt(p)), the babies
    1 .. bs_eff - 1, the negative giants -g bs_eff for 1 <= g < ceil(p / bs_eff), then for form 0 the positive ones."""
    if bs is None:
        bs = 1
        while bs * bs < p:
            bs *= 2
    eff = min(bs, p)
    G = -(-p // eff)
    steps = list(range(1, eff)) + [-g * eff for g in range(1, G)]
    if form == 0:
        steps += [g * eff for g in range(1, G)]
    return eff, steps


@pytest.mark.parametrize("p,bs,form,want", [
    (11, 4, 0, (4, [1, 2, 3, -4, -8, 4, 8])),
    (11, 4, 1, (4, [1, 2, 3, -4, -8])),
    (11, None, 1, (4, [1, 2, 3, -4, -8])),
    (11, 16, 0, (11, list(range(1, 11)))),  # one block: no giants
    (1, None, 0, (1, [])),
])
def test_plan(hecdna, p, bs, form, want):
    assert hecdna.colcolT_bsgs_plan(p, bs, form) == want == plan_ref(p, bs, form)


@pytest.mark.parametrize("p,bs,form", [(1024, None, 0), (1024, 32, 1), (24, 1, 0), (24, 5, 1), (4096, 64, 0)])
def test_plan_matches_definition(hecdna, p, bs, form):
    assert hecdna.colcolT_bsgs_plan(p, bs, form) == plan_ref(p, bs, form)


def test_plan_default_form_is_natural(hecdna):
    assert hecdna.colcolT_bsgs_plan(11, 4) == hecdna.colcolT_bsgs_plan(11, 4, hecdna.DIAG_NATURAL)
    assert (hecdna.DIAG_NATURAL, hecdna.DIAG_BSGS) == (0, 1)


def test_plan_cap_and_count(hecdna):
    """*count is the number of steps whatever the cap; min(cap, *count) steps are written and nothing behind them;
    steps may be null only with cap = 0; bs_eff is optional."""
    fn = hecdna.lib().hec_colcolT_bsgs_plan
    cnt, eff = C.c_uint64(), C.c_uint64()
    assert fn(11, 4, 0, None, 0, C.byref(cnt), C.byref(eff)) == 0
    assert (cnt.value, eff.value) == (7, 4)
    buf = (C.c_int * 8)(*([99] * 8))
    assert fn(11, 4, 0, buf, 3, C.byref(cnt), None) == 0
    assert cnt.value == 7 and list(buf) == [1, 2, 3] + [99] * 5
    assert fn(11, 4, 0, buf, 8, C.byref(cnt), C.byref(eff)) == 0
    assert cnt.value == 7 and list(buf) == [1, 2, 3, -4, -8, 4, 8, 99]
    assert fn(11, 4, 0, None, 3, C.byref(cnt), None) != 0  # null steps with a cap
    assert fn(11, 4, 0, buf, 8, None, None) != 0  # null count


def test_plan_errors(hecdna):
    for p, bs, form in [(0, 1, 0), (1 << 30, 4, 0), (11, 4, 2), (11, 4, -1)]:
        with pytest.raises(hecdna.InvalidArgument):
            hecdna.colcolT_bsgs_plan(p, bs, form)
    assert hecdna.colcolT_bsgs_plan((1 << 30) - 1, 1 << 15, 1)[0] == 1 << 15  # the largest p is allowed
    with pytest.raises(hecdna.InvalidArgument):
        hecdna.colcolT_bsgs_plan(11, 0)


def test_symbols_exported_and_declared(hecdna):
    out = subprocess.check_output(["nm", "-D", "--defined-only", hecdna.LIB_PATH]).decode()
    for s in ("hec_colcolT_bsgs_plan", "hec_matmul_col_colT_bsgs"):
        assert re.search(r" T " + s + "$", out, re.M)
        assert s in hecdna.exported_symbols()
    txt = re.sub(r"\s+", " ", open(hecdna.HEADER_PATH).read())
    assert "#define HEC_DIAG_NATURAL 0" in txt and "#define HEC_DIAG_BSGS 1" in txt
    assert ("int hec_colcolT_bsgs_plan(uint64_t p, uint64_t bs, int form, int *steps, uint64_t cap, uint64_t *count, "
            "uint64_t *bs_eff);") in txt
    assert ("int hec_matmul_col_colT_bsgs(hec_context *ctx, const hec_ciphertext *const *A, uint64_t n, "
            "const hec_ciphertext *const *B, uint64_t p, uint64_t bs, int form, const hec_kswitch_key *rk, "
            "const hec_galois_keys *gk, hec_ciphertext *const *out);") in txt


def test_python_binding(hecdna):
    vp, u64 = C.c_void_p, C.c_uint64
    L = hecdna.lib()
    # ctx, A, n, B, p, bs, form, rk, gk, out
    assert L.hec_matmul_col_colT_bsgs.argtypes == [vp, vp, u64, vp, u64, u64, C.c_int, vp, vp, vp]
    # p, bs, form, steps, cap, count, bs_eff
    assert L.hec_colcolT_bsgs_plan.argtypes == [u64, u64, C.c_int, C.POINTER(C.c_int), u64, C.POINTER(u64),
                                                C.POINTER(u64)]
    sig = inspect.signature(hecdna.Context.matmul_col_colT_bsgs)
    assert list(sig.parameters) == ["self", "A", "B", "p", "rk", "gk", "bs", "bsgs_form", "out"]
    assert sig.parameters["bs"].default is None and sig.parameters["out"].default is None
    assert sig.parameters["bsgs_form"].default is False
    sig = inspect.signature(hecdna.colcolT_bsgs_plan)
    assert list(sig.parameters) == ["p", "bs", "form"]
    assert sig.parameters["bs"].default is None and sig.parameters["form"].default == 0


def test_null_context_is_refused(hecdna):
    """A null context is HEC_EINVAL on the host path, as for every entry."""
    assert hecdna.lib().hec_matmul_col_colT_bsgs(None, None, 1, None, 1, 1, 0, None, None, None) != 0


def test_cpp_drop_in_declares_the_calls(hecdna):
    hpp = os.path.join(os.path.dirname(hecdna.LIB_PATH), "cpp", "include", "hecdna", "seal_compat.hpp")
    txt = open(hpp).read()
    assert "colcolT_bsgs_steps(std::size_t p" in txt
    assert "matmul_col_colT_bsgs(const Evaluator &eval" in txt
