"""KeyGenerator / Encryptor on the GPU (hec_keygen_*, hec_encrypt_symmetric, hec_encrypt) against the
independent Python restatement tests/keygen_ref.py: every key and ciphertext word for word, the structure of the keys
with no tolerance, the seeded wire format, decode bounds, one GPU-only pipeline, seeds and errors.

Shapes: N = 2^10 and 2^11 with {60, 40, 40, 60} (both arithmetic classes of the NTT); N = 2^13 crosses several PRNG
buffers per limb.  The pure-Python BLAKE2b runs only at N = 2^10; elsewhere the streams come from the library's host
BLAKE2Xb, which test_keygen_ref.py and test_seal_format.py pin to it.

Decode bounds (per slot; a slot is a sum of N coefficients times unit roots, divided by scale):
  symmetric:   (21 + 0.5) N / scale: |e| <= 21 per coefficient and 0.5 for the encoder's rounding;
  asymmetric:  that + N ((N + 1) / 2 + 1 + 21 (2N + 1) / q_last) / scale: after the division by q_last the noise
               u e_pk + e_0 + e_1 s is at most 21 (2N + 1) / q_last per coefficient, and the rounding of the two
               polynomials leaves 1/2 + |s|_1 / 2 <= (N + 1) / 2, + 1 for the two roundings' own half units;
  + the decoder's own tolerance as test_gpu_decode.py derives it: (10 log2 N + 16) 2^-53 sqrt(2 sum |v_i|^2)."""
import hashlib
import os
import sys

import numpy as np
import pytest

import keygen_ref as kr

pytestmark = pytest.mark.gpu
BITS = [60, 40, 40, 60]
Q0_REDRAW = 0x0F0F0F0F0F0F7001  # prime, = 1 mod 2^12, 60 bits: one word in 17.000 is redrawn
U = 2.0 ** -53


def seed(tag: str) -> bytes:
    return hashlib.blake2b(tag.encode(), digest_size=64).digest()


class KEnv:
    def __init__(self, orc, hecdna, logN, pure=False, q0=None, bits=None):
        self.orc, self.hec = orc, hecdna
        self.N = 1 << logN
        self.m = orc.Oracle.create_coeff_modulus(self.N, bits or BITS)
        if q0:
            self.m[0] = q0
        self.o = orc.Oracle(self.N, self.m)
        self.K, self.L = len(self.m), len(self.m) - 1
        self.ctx = hecdna.Context(self.N, self.m)
        self.ref = kr.Ref(self.o, kr.Streams(None if pure else hecdna))
        self.sd = seed(f"secret {logN} {q0}")
        self.sk = self.ctx.keygen_secret(self.sd)
        self.s = self.ref.secret(self.sd)

    def pt(self, level, scale, k=0):
        rng = np.random.default_rng(100 * level + k)
        v = rng.uniform(-1, 1, self.N // 2) + 1j * rng.uniform(-1, 1, self.N // 2)
        h = self.o.encode(v, scale, level)
        return v, h, self.ctx.plaintext(h, scale)


_envs = {}


@pytest.fixture(scope="module")
def kenv(orc, hecdna):
    def get(logN, pure=False, q0=None):
        key = (logN, pure, q0)
        if key not in _envs:
            _envs[key] = KEnv(orc, hecdna, logN, pure, q0)
        return _envs[key]
    yield get
    _envs.clear()


class poisoned:
    def __init__(self, ctx):
        self.ctx = ctx

    def __enter__(self):
        self.ctx.set_option("poison", 1)

    def __exit__(self, *a):
        self.ctx.set_option("poison", 0)


# ------------------------------------------------------------------------------- keys, bit-exact ----
@pytest.mark.parametrize("logN,pure", [(10, True), (11, False), (13, False)])
def test_secret_and_public_key_bitexact(kenv, logN, pure):
    e = kenv(logN, pure)
    with poisoned(e.ctx):
        sd = seed("public")
        assert np.array_equal(e.ctx.keygen_secret(e.sd).download(), e.s)
        pk = e.ctx.keygen_public(e.sk, sd)
        assert np.array_equal(pk.download(), e.ref.public(e.s, sd))
    assert np.array_equal(e.sk.download(), e.s)
    again = e.ctx.public_key(pk.download())
    assert np.array_equal(again.download(), pk.download())


@pytest.mark.parametrize("logN", [10, 11])
def test_relin_key_bitexact(kenv, logN):
    e = kenv(logN)
    sd = seed("relin")
    with poisoned(e.ctx):
        rk = e.ctx.keygen_relin(e.sk, sd)
        assert np.array_equal(rk.download(), e.ref.relin(e.s, sd))


@pytest.mark.parametrize("logN", [10, 11])
def test_galois_keys_bitexact_alone_and_in_a_set(kenv, logN):
    e = kenv(logN)
    sd = seed("galois")
    elts = [3, e.o.elt_from_step(-1), 2 * e.N - 1]
    with poisoned(e.ctx):
        gk = e.ctx.keygen_galois(e.sk, elts, sd)
        for elt in elts:
            assert gk.has(elt)
            exp = e.ref.galois(e.s, elt, sd)
            assert np.array_equal(gk.download(elt), exp), elt
            alone = e.ctx.keygen_galois(e.sk, [elt], sd)
            assert not alone.has(elts[0] if elt != elts[0] else elts[1])
            assert np.array_equal(alone.download(elt), exp), elt
    # regenerating into the same set replaces the key (as hec_galois_keys_add does)
    e.ctx.keygen_galois(e.sk, [3], seed("galois 2"), gk=gk)
    assert np.array_equal(gk.download(3), e.ref.galois(e.s, 3, seed("galois 2")))


def test_default_galois_set(kenv):
    """n == 0 makes the set of hec_default_galois_elts; one of its keys word for word"""
    e = kenv(10)
    sd = seed("default set")
    gk = e.ctx.keygen_galois(e.sk, None, sd)
    elts = e.ctx.default_galois_elts()
    assert len(elts) == 2 * 10 - 1 and all(gk.has(x) for x in elts)
    assert np.array_equal(gk.download(elts[4]), e.ref.galois(e.s, elts[4], sd))


@pytest.mark.parametrize("group", [1, 3, 16])
def test_generator_group_sizes_draw_the_same_words(kenv, group):
    """k_prng with 1, 3 (a short last group) and 16 buffers per wavefront, roots shared through LDS: the same keys, word
    for word; at these sizes the launcher itself picks 1"""
    e = kenv(11)
    sd = seed("group")
    e.ctx.set_option("prng_group", group)
    try:
        with poisoned(e.ctx):
            assert np.array_equal(e.ctx.keygen_secret(e.sd).download(), e.s)
            assert np.array_equal(e.ctx.keygen_relin(e.sk, sd).download(), e.ref.relin(e.s, sd))
            pk = e.ctx.keygen_public(e.sk, sd)
            _, h, g = e.pt(2, 2.0 ** 30)
            got = e.ctx.encrypt(pk, [g, g, g], sd)[2].download()
            assert np.array_equal(got, e.ref.encrypt(e.orc, pk.download(), h, 2.0 ** 30, sd, 2))
    finally:
        e.ctx.set_option("prng_group", 0)
    with pytest.raises(e.hec.InvalidArgument):
        e.ctx.set_option("prng_group", 17)


# ------------------------------------------------------------------------------- encryption, bit-exact ----
def test_encrypt_symmetric_mixed_batch_bitexact(kenv):
    e = kenv(11)
    sd = seed("symmetric")
    levels = [1, 3, 2, 3, 1]
    scales = [2.0 ** 30, 2.0 ** 40, 2.0 ** 35, 2.0 ** 40, 2.0 ** 25]
    pts = [e.pt(l, sc, k) for k, (l, sc) in enumerate(zip(levels, scales))]
    with poisoned(e.ctx):
        cts, ps = e.ctx.encrypt_symmetric(e.sk, [p[2] for p in pts], sd, public_seeds=True)
        for v, ct in enumerate(cts):
            assert ct.info() == (2, levels[v], scales[v])
            exp = e.ref.encrypt_symmetric(e.s, pts[v][1], sd, v)  # made alone from index v's own sub-streams
            assert np.array_equal(ct.download(), exp), v
            assert ps[v].tobytes() == e.ref.st.sub(sd, kr.CALL_SYM, kr.ROLE_A, v, 0)
        one = e.ctx.encrypt_symmetric(e.sk, pts[0][2], sd)  # a batch of one is index 0
        assert np.array_equal(one.download(), cts[0].download())


@pytest.mark.parametrize("logN", [10, 11])
def test_encrypt_public_key_bitexact(kenv, logN):
    """level L divides by the special prime, the lower levels by a data prime"""
    e = kenv(logN)
    sd, sdk = seed("asymmetric"), seed("asymmetric pk")
    pk_h = e.ref.public(e.s, sdk)
    levels = [e.L, 2, 1, e.L]
    pts = [e.pt(l, 2.0 ** 30, k) for k, l in enumerate(levels)]
    with poisoned(e.ctx):
        pk = e.ctx.keygen_public(e.sk, sdk)
        assert np.array_equal(pk.download(), pk_h)
        cts = e.ctx.encrypt(pk, [p[2] for p in pts], sd)
        for v, ct in enumerate(cts):
            assert ct.info() == (2, levels[v], 2.0 ** 30)
            assert np.array_equal(ct.download(), e.ref.encrypt(e.orc, pk_h, pts[v][1], 2.0 ** 30, sd, v)), v


# ------------------------------------------------------------------------------- redraws ----
def test_redraws_match_the_host_walk(kenv):
    """q_0 = 0x0f0f0f0f0f0f7001 redraws one word in 17: about 60 per 1,024 words, 3.5 of them redrawn again"""
    e = kenv(10, q0=Q0_REDRAW)
    sd = seed("redraw")
    stats = {}
    exp = e.ref.relin(e.s, sd, stats)  # L digits, each with a limb of q_0 in its `a`
    first = stats["first"]
    assert len(first) == e.L * e.K
    q0_limbs = [first[J * e.K] for J in range(e.L)]
    print("redraws per q_0 limb", q0_limbs, "redrawn again", stats["again"])
    assert all(x >= 1 for x in q0_limbs) and stats["again"] >= 1
    with poisoned(e.ctx):
        got = e.ctx.keygen_relin(e.sk, sd).download()
    assert np.array_equal(got[:, 1], exp[:, 1])  # every `a`, word for word
    assert np.array_equal(got, exp)
    assert np.array_equal(e.sk.download(), e.s)  # and a secret key (its own redraw path cannot be reached)


# ------------------------------------------------------------------------------- seeded wire format ----
@pytest.mark.parametrize("compr", [0, 2])
def test_seeded_round_trip(kenv, compr):
    e = kenv(11)
    sd = seed("seeded")
    pts = [e.pt(l, 2.0 ** 40, 7 + l) for l in (3, 1)]
    cts, ps = e.ctx.encrypt_symmetric(e.sk, [p[2] for p in pts], sd, public_seeds=True)
    for ct, sub in zip(cts, ps):
        d = ct.download()
        b = e.hec.seal_ciphertext_save_seeded(d[0], ct.scale, e.m, sub.tobytes(), compr=compr)
        full = ct.save_seal(compr=0)
        assert len(b) < len(full) // 2 + 256  # c0 and a seed
        back = e.ctx.ciphertext()
        assert back.load_seal(b) == len(b)
        assert back.info() == ct.info()
        assert np.array_equal(back.download(), d)


# ------------------------------------------------------------------------------- structure ----
def assert_noise(e, c0, c1, nl, sub=None, what=""):
    polys = e.ref.noise_of(c0, c1, e.s, nl, sub)
    assert all(p == polys[0] for p in polys), what  # one polynomial on every limb
    assert max(abs(x) for x in polys[0]) <= kr.CBD_MAX, what
    assert any(polys[0]), what


def test_structure_of_keys_and_ciphertexts(kenv):
    """c0 + c1 s - [I = J] P newkey is, on every limb, the same polynomial with coefficients in [-21, 21]"""
    e = kenv(10)
    P = e.m[-1]
    zero = np.zeros(e.N, dtype=np.uint64)
    pk = e.ctx.keygen_public(e.sk, seed("structure pk")).download()
    assert_noise(e, pk[0], pk[1], e.K, what="public key")
    s2 = [kr.u64(kr.obj(e.s[j]) * kr.obj(e.s[j]) % e.m[j]) for j in range(e.K)]
    rk = e.ctx.keygen_relin(e.sk, seed("structure rk")).download()
    keys = [("relin", rk, s2)]
    elts = [3, 2 * e.N - 1]
    gk = e.ctx.keygen_galois(e.sk, elts, seed("structure gk"))
    for elt in elts:
        keys.append((f"galois {elt}", gk.download(elt), e.o.apply_galois_ntt(e.s, elt).reshape(e.K, e.N)))
    for name, key, newkey in keys:
        for J in range(e.L):
            sub = [kr.u64(kr.obj(newkey[J]) * (P % e.m[J]) % e.m[J]) if j == J else zero for j in range(e.K)]
            assert_noise(e, key[J, 0], key[J, 1], e.K, sub, f"{name} digit {J}")
    for level in (1, e.L):
        _, h, g = e.pt(level, 2.0 ** 30)
        ct = e.ctx.encrypt_symmetric(e.sk, g, seed("structure ct")).download()
        assert_noise(e, ct[0], ct[1], level, h, f"ciphertext level {level}")


# ------------------------------------------------------------------------------- functional ----
def decoder_tol(v, N):
    return (10 * np.log2(N) + 16) * U * np.sqrt(2 * np.sum(np.abs(v) ** 2))


@pytest.mark.parametrize("logN", [10, 13])
def test_decrypt_decode_of_fresh_encryptions(kenv, logN):
    e = kenv(logN)
    N, scale = e.N, 2.0 ** 30
    pk = e.ctx.keygen_public(e.sk, seed("functional pk"))
    for level in (e.L, 1):
        rng = np.random.default_rng(level)
        v = rng.uniform(-1, 1, N // 2) + 1j * rng.uniform(-1, 1, N // 2)
        pt = e.ctx.encode(v, scale, level)
        sym = (kr.CBD_MAX + 0.5) * N / scale + decoder_tol(v, N)
        q_last = e.m[level]  # the prime encrypt divides by: q_level, or the special prime at level L
        asym = sym + N * ((N + 1) / 2 + 1 + kr.CBD_MAX * (2 * N + 1) / q_last) / scale
        got = e.ctx.decrypt_decode(e.sk, e.ctx.encrypt_symmetric(e.sk, pt, seed("functional sym")))
        err = np.max(np.abs(got - v))
        print(f"N=2^{logN} level {level} symmetric: error {err:.3e} bound {sym:.3e}")
        assert err <= sym
        got = e.ctx.decrypt_decode(e.sk, e.ctx.encrypt(pk, pt, seed("functional asym")))
        err = np.max(np.abs(got - v))
        print(f"N=2^{logN} level {level} asymmetric: error {err:.3e} bound {asym:.3e}")
        assert err <= asym


def test_pipeline_on_the_gpu_alone(orc, hecdna):
    """cfg1's shape (N = 2^13, {60, 40, 40, 60}, scale 2^40, the demo's 64 x 64 data, 16 of the columns as inputs):
    keygen, encode, encrypt, matmul_diag_col, decrypt_decode on the GPU against the clear product.  The bound is
    measured: the same pipeline on the oracle's own keys and ciphertexts gives eps_ref, and the GPU must stay within
    8 eps_ref: both are maxima over the slots of noise of the same width from different streams, while a wrong sign
    or key is off by many orders.  The inputs are encrypted symmetrically, as the oracle's are (the public-key path
    has a wider fresh noise and its own bound above)."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    from make_golden import CFG1, cfg1_expected_plain, cfg1_inputs
    n, N, scale, p = CFG1["n"], CFG1["N"], CFG1["scale"], 16
    clear = cfg1_expected_plain(n, N // 2)[:p]
    o, m, sk_h, rk_h, gk_h, cts_h = cfg1_inputs(orc)
    outs = o.matmul_diag_col(cts_h, cts_h[:p], rk_h, gk_h, nthreads=8)
    eps_ref = max(np.max(np.abs(o.decode(o.decrypt(sk_h, c), c.scale)[:n] - clear[i])) for i, c in enumerate(outs))

    ctx = hecdna.Context(N, m)
    sk = ctx.keygen_secret(seed("pipeline sk"))
    rk = ctx.keygen_relin(sk, seed("pipeline rk"))
    gk = ctx.keygen_galois(sk, None, seed("pipeline gk"))
    vals = np.array([[2 + n * c + (r % n) for r in range(N // 2)] for c in range(n)], dtype=np.float64)
    cts = ctx.encrypt_symmetric(sk, ctx.encode(vals, scale), seed("pipeline enc"))
    got = ctx.decrypt_decode(sk, ctx.matmul_diag_col(cts, cts[:p], rk, gk), n_values=n)
    eps = max(np.max(np.abs(got[i] - clear[i])) for i in range(p))
    print(f"pipeline: eps_ref {eps_ref:.3e} (oracle keys and ciphertexts), GPU {eps:.3e}, ratio {eps / eps_ref:.2f}")
    assert eps <= 8 * eps_ref


# ------------------------------------------------------------------------------- seeds, errors ----
def test_determinism_and_entropy(kenv):
    e = kenv(10)
    sd = seed("determinism")
    _, _, g = e.pt(2, 2.0 ** 30)
    a, b = (e.ctx.encrypt_symmetric(e.sk, g, sd).download() for _ in range(2))
    assert np.array_equal(a, b)
    a, b = (e.ctx.keygen_relin(e.sk, sd).download() for _ in range(2))
    assert np.array_equal(a, b)
    a, b = (e.ctx.encrypt_symmetric(e.sk, g, None).download() for _ in range(2))  # NULL: 64 bytes of OS entropy
    assert not np.array_equal(a, b) and not np.array_equal(a[1], b[1])
    a, b = (e.ctx.keygen_secret(None).download() for _ in range(2))
    assert not np.array_equal(a, b)


def test_errors_leave_outputs_unchanged(kenv, hecdna):
    e, f = kenv(10), kenv(11)
    sd = seed("errors")
    _, _, g = e.pt(2, 2.0 ** 30)
    out = e.ctx.encrypt_symmetric(e.sk, g, sd)
    before = out.download()
    with pytest.raises(hecdna.InvalidArgument, match="secret key is not valid for encryption parameters"):
        e.ctx.encrypt_symmetric(f.sk, g, sd, out=out)  # a foreign context's key
    with pytest.raises(hecdna.InvalidArgument, match="secret key is not valid for encryption parameters"):
        e.ctx.keygen_relin(f.sk, sd)
    with pytest.raises(hecdna.InvalidArgument, match="secret key is not valid for encryption parameters"):
        e.ctx.keygen_public(f.sk, sd)
    pk_f = f.ctx.keygen_public(f.sk, sd)
    with pytest.raises(hecdna.InvalidArgument, match="public key is not valid for encryption parameters"):
        e.ctx.encrypt(pk_f, g, sd, out=out)
    with pytest.raises(hecdna.InvalidArgument, match="public key is not valid for encryption parameters"):
        e.ctx.public_key(np.zeros((2, e.K, e.N + 1), dtype=np.uint64))  # a wrong-size upload
    _, _, g_f = f.pt(2, 2.0 ** 30)
    with pytest.raises(hecdna.InvalidArgument, match="plain is not valid for encryption parameters"):
        e.ctx.encrypt_symmetric(e.sk, [g, g_f], sd, out=[out, e.ctx.ciphertext()])
    assert out.info() == (2, 2, 2.0 ** 30) and np.array_equal(out.download(), before)
    gk = e.ctx.keygen_galois(e.sk, [3], sd)
    key3 = gk.download(3)
    with pytest.raises(hecdna.InvalidArgument, match="Galois element is not valid"):
        e.ctx.keygen_galois(e.sk, [5, 4], sd, gk=gk)  # an even element: nothing is made, not even the key of 5
    assert not gk.has(5) and np.array_equal(gk.download(3), key3)
