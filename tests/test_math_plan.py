"""CPU: hec_math_plan, the host planner of the batched he::math calls (hecdna.math_plan), against the restatement of
the reference's schedules over the CPU oracle (oracle/he_math_ref.py) at N = 2^10: the level and the scale double of
every result (compared with ==), and the message of the first check the per-operation sequence fails.  The planner is
the code the device calls run before any device work, so this fixes their levels, scales and errors without a GPU."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import he_math_ref as hm  # noqa: E402

N = 1 << 10
FNS = {"signed_inv": (0, hm.signed_inv), "inv_sqrt_twice": (1, hm.inv_sqrt_twice), "sqrt": (2, hm.sqrt),
       "abs": (3, hm.abs_)}


@pytest.fixture(scope="module")
def env(orc):
    m = orc.Oracle.create_coeff_modulus(N, [60] + [40] * 10 + [60])
    o = orc.Oracle(N, m)
    sk = o.secret_key(5)
    rk = o.relin_key(sk, 6)
    x = np.random.default_rng(7).uniform(0.5, 1.5, N // 2)
    cache = {}

    def ct(level, scale):
        if (level, scale) not in cache:
            cache[level, scale] = o.encrypt(sk, o.encode(x, scale, level), scale, 8)
        return cache[level, scale]
    return orc, o, m, rk, ct


def ref(env, name, a, iters, level, scale):
    """(level, scale) of the restated schedule on the oracle, or its error message"""
    orc, o, m, rk, ct = env
    try:
        r = FNS[name][1](o, rk, ct(level, scale), a, iters)
    except orc.OracleError as e:
        return str(e)
    return r.level, r.scale


def plan(env, hecdna, name, a, iters, level, scale):
    orc, o, m, rk, ct = env
    try:
        return hecdna.math_plan(m, FNS[name][0], a, iters, level, scale)
    except hecdna.InvalidArgument as e:
        return e


LEVELS = {"signed_inv": [9, 7, 6, 5], "inv_sqrt_twice": [9, 7, 5, 3], "sqrt": [8, 6, 4, 2], "abs": [7, 5, 3, 1]}


@pytest.mark.parametrize("name", list(FNS))
def test_levels_and_scales(env, hecdna, name):
    for iters in (1, 2, 3, 4):
        a = 0.7 if name == "inv_sqrt_twice" else 1.0
        exp = ref(env, name, a, iters, 10, 2.0**40)
        assert exp[0] == LEVELS[name][iters - 1]
        got = plan(env, hecdna, name, a, iters, 10, 2.0**40)
        assert got == exp  # the level, and the scale double with ==


@pytest.mark.parametrize("name,iters,level,scale,msg,ok_level", [
    ("signed_inv", 3, 4, 2.0**40, "scale out of bounds", 5),
    ("abs", 2, 5, 2.0**40, "scale out of bounds", 6),
    ("signed_inv", 1, 1, 2.0**20, "end of modulus switching chain reached", 2)])
def test_first_failing_check(env, hecdna, name, iters, level, scale, msg, ok_level):
    exp = ref(env, name, 1.0, iters, level, scale)
    assert isinstance(exp, str) and msg in exp
    got = plan(env, hecdna, name, 1.0, iters, level, scale)
    assert isinstance(got, hecdna.InvalidArgument) and msg in str(got)
    exp = ref(env, name, 1.0, iters, ok_level, scale)
    assert exp[0] == 1  # one level more reaches level 1
    assert plan(env, hecdna, name, 1.0, iters, ok_level, scale) == exp


def test_constants(env, hecdna):
    for name in ("signed_inv", "inv_sqrt_twice"):
        exp = ref(env, name, float("nan"), 2, 10, 2.0**40)
        assert isinstance(exp, str) and "encoded value is too large" in exp
        got = plan(env, hecdna, name, float("nan"), 2, 10, 2.0**40)
        assert isinstance(got, hecdna.InvalidArgument) and "encoded value is too large" in str(got)
        for a in (0.0, -1.0, 1e8):
            exp = ref(env, name, a, 2, 10, 2.0**40)
            assert not isinstance(exp, str)
            assert plan(env, hecdna, name, a, 2, 10, 2.0**40) == exp


def test_arguments(env, hecdna):
    orc, o, m, rk, ct = env
    with pytest.raises(hecdna.InvalidArgument, match="iter_num must be positive"):
        hecdna.math_plan(m, 0, 1.0, 0, 10, 2.0**40)
    with pytest.raises(hecdna.InvalidArgument, match="not valid for encryption parameters"):
        hecdna.math_plan(m, 0, 1.0, 1, 12, 2.0**40)
    with pytest.raises(hecdna.InvalidArgument, match="unknown he::math function"):
        hecdna.math_plan(m, 4, 1.0, 1, 10, 2.0**40)
