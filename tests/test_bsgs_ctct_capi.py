"""hec_matmul_diag_col_bsgs at the drop-in boundary (no device): the symbol is exported with the documented signature
and the Python and C++ surfaces over it exist.  The 512 cap needs a context, and a context needs a device, so it is
tested in tests/test_gpu_bsgs_ctct.py."""
import ctypes as C
import inspect
import os
import re
import subprocess


def test_symbol_exported_and_declared(hecdna):
    out = subprocess.check_output(["nm", "-D", "--defined-only", hecdna.LIB_PATH]).decode()
    assert re.search(r" T hec_matmul_diag_col_bsgs$", out, re.M)
    assert "hec_matmul_diag_col_bsgs" in hecdna.exported_symbols()
    txt = re.sub(r"\s+", " ", open(hecdna.HEADER_PATH).read())
    assert ("int hec_matmul_diag_col_bsgs(hec_context *ctx, const hec_ciphertext *const *diags, uint64_t n, "
            "uint64_t bs, const hec_ciphertext *const *cols, uint64_t p, const hec_kswitch_key *rk, "
            "const hec_galois_keys *gk, hec_ciphertext *const *out);") in txt


def test_python_binding(hecdna):
    fn = hecdna.lib().hec_matmul_diag_col_bsgs
    vp, u64 = C.c_void_p, C.c_uint64
    assert fn.argtypes == [vp, vp, u64, u64, vp, u64, vp, vp, vp]  # ctx, diags, n, bs, cols, p, rk, gk, out
    sig = inspect.signature(hecdna.Context.matmul_diag_col_bsgs)
    assert list(sig.parameters) == ["self", "diags", "cols", "rk", "gk", "bs", "out"]
    assert sig.parameters["bs"].default is None and sig.parameters["out"].default is None
    assert list(inspect.signature(hecdna.Context.bsgs_rotate_diagonals).parameters) == ["self", "diags", "bs", "gk"]


def test_null_arguments_are_refused_before_anything_runs(hecdna):
    """A null context is HEC_EINVAL on the host path, as for every entry."""
    assert hecdna.lib().hec_matmul_diag_col_bsgs(None, None, 1, 1, None, 1, None, None, None) != 0


def test_cpp_drop_in_declares_the_call(hecdna):
    hpp = os.path.join(os.path.dirname(hecdna.LIB_PATH), "cpp", "include", "hecdna", "seal_compat.hpp")
    txt = open(hpp).read()
    assert "matmul_diag_col_bsgs(const Evaluator &eval" in txt
    assert "bsgs_rotate_diagonals(const Evaluator &eval" in txt
