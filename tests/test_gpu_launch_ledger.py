"""The launch ledger: for a fixed list of engine calls (tests/golden/make_launch_ledger.py: the batched he::linalg,
he::math and he::fft calls, the matvec family with both baby-step giant-step forms (whole, and in tiles of 2 giants and
passes of 2 vectors), the baby-step giant-step col x col^T product in both output forms (whole, and in passes of 2
columns), the sharded matvec on a world of one, the evaluator's relinearize, rescale, rotate_vector, apply_galois,
multiply and square, and the client half (keygen_*, encrypt*, decrypt, decode; encode records no class and has no
entry), at N = 2^11 over {60, 40, 40, 40, 40, 60}),
every profile class a call touches must show the scopes, kernel launches and algorithmic bytes recorded in
tests/golden/launch_ledger.json, and no other class.  The fixture is recorded at the commit before a change that must
leave the launch sequence alone, so a moved, lost or doubled launch fails here even where the words stay right.

What it does not see: the device copies of the gathers and of the output stores carry no profile scope, so the ledger
does not cover them; the bit-exact suites do."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def ledgers(hecdna):
    spec = importlib.util.spec_from_file_location("make_launch_ledger", os.path.join(GOLDEN, "make_launch_ledger.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(mod.FIXTURE) as f:
        return mod.record(hecdna), json.load(f), list(mod.CALLS)


def test_every_call_is_recorded(ledgers):
    got, want, calls = ledgers
    assert sorted(got) == sorted(want) == sorted(calls)


def test_launch_ledger(ledgers):
    got, want, calls = ledgers
    for call in calls:
        assert sorted(got[call]) == sorted(want[call]), call  # the set of class names
        for cls, rec in want[call].items():
            # alg_bytes is a double computed from integers, so == holds
            assert got[call][cls] == rec, (call, cls)
