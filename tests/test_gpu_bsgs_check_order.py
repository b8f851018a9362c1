"""The order of the argument checks of the two baby-step giant-step matvecs, on calls with two faults at once: the
answer names the fault that the call's own order meets first.  hec_matmul_diagpt_col_bsgs runs the aliasing rule
before the scale checks; hec_matmul_diag_col_bsgs runs the scale checks, the relinearisation key and the planned
rotations first, the aliasing rule after them and the rule that no diagonal is an output last; its cap on bs comes
before everything.  In both, an output is checked as an object in the loop that looks for duplicates.  Uniform
synthetic objects: no call here gets as far as a launch."""
import pytest

pytestmark = pytest.mark.gpu

N11, BITS, L, SCALE = 1 << 11, [60, 40, 40, 60], 3, 2.0**40
n, bs, p = 4, 2, 3  # steps 1 (baby) and 2 (giant)


class Env:
    def __init__(self, hec):
        self.hec = hec
        self.ctx = hec.Context(N11, hec.create_coeff_modulus(N11, BITS))
        self.other = hec.Context(N11, hec.create_coeff_modulus(N11, BITS))
        ctx = self.ctx
        self.cols = [ctx.ciphertext().fill_uniform(2, L, SCALE, 100 + i) for i in range(p)]
        self.cts = [ctx.ciphertext().fill_uniform(2, L, SCALE, 200 + j) for j in range(n)]
        self.pts = [ctx.plaintext(None, SCALE).fill_uniform(L, SCALE, 300 + j) for j in range(n)]
        # the last diagonal at another scale: "scale mismatch" at the first column
        self.cts_scale = self.cts[:-1] + [ctx.ciphertext().fill_uniform(2, L, 2.0**30, 250)]
        self.pts_scale = self.pts[:-1] + [ctx.plaintext(None, 2.0**30).fill_uniform(L, 2.0**30, 350)]
        self.rk = ctx.relin_key(seed=5)
        self.gk = ctx.galois_keys(uniform_elts=ctx.default_galois_elts(), seed=6)
        self.gk_step1 = ctx.galois_keys(uniform_elts=[ctx.elt_from_step(1)], seed=7)  # no key for the giant step
        self.rk_other = self.other.relin_key(seed=8)
        self.gk_other = self.other.galois_keys(uniform_elts=self.other.default_galois_elts(), seed=9)
        self.foreign = self.other.ciphertext()

    def outs(self):
        return [self.ctx.ciphertext() for _ in range(p)]

    def pt(self, match, out, pdiags=None, gk=None):
        with pytest.raises(self.hec.InvalidArgument, match=match):
            self.ctx.matmul_diagpt_col_bsgs(pdiags or self.pts, self.cols, gk or self.gk, bs=bs, out=out)

    def ct(self, match, out, diags=None, rk=None, gk=None, bs=bs):
        with pytest.raises(self.hec.InvalidArgument, match=match):
            self.ctx.matmul_diag_col_bsgs(diags or self.cts, self.cols, rk or self.rk, gk or self.gk, bs=bs, out=out)


@pytest.fixture(scope="module")
def env(hecdna):
    e = Env(hecdna)
    yield e
    e.ctx.close()
    e.other.close()


def twice(e):
    o = e.outs()
    return [o[0], o[0], o[2]]


def test_alias_against_scale(env):
    env.pt("alias", twice(env), pdiags=env.pts_scale)
    env.ct("scale mismatch", twice(env), diags=env.cts_scale)


def test_alias_against_missing_galois_key(env):
    env.pt("alias", twice(env), gk=env.gk_step1)
    env.ct("Galois key not present", twice(env), gk=env.gk_step1)


def test_alias_against_relin_key(env):
    env.ct("relin_keys is not valid", twice(env), rk=env.rk_other)


def test_output_object_check_is_interleaved_with_duplicates(env):
    o = env.outs()
    for call in (env.pt, env.ct):
        call("alias", [o[0], o[0], env.foreign])
        call("encrypted is not valid", [env.foreign, o[1], o[2]])
        call("encrypted is not valid", [o[0], env.foreign, o[0]])


def test_diagonal_as_output_comes_last(env):
    o = env.outs()
    env.ct("alias", [env.cts[1], o[1], o[2]])
    env.ct("encrypted is not valid", [env.cts[1], o[1], env.foreign])  # the outputs' loop runs before the diagonals'
    env.ct("alias", [o[1], env.cols[0], o[2]])  # another entry's input


def test_ct_cap_comes_first(env):
    env.ct("bs must be at most 512", env.outs(), diags=[env.cts[0]] * 513, gk=env.gk_other, bs=513)
    env.ct("galois_keys is not valid", env.outs(), gk=env.gk_other)
