"""Object lifetime through the C-ABI (include/hecdna.h, csrc/hec_live.h): calls on objects whose context is gone,
destroys that arrive on another thread, handles of an earlier context at a reused address, and the one buffer growth
routine behind every ciphertext and plaintext result.  N = 2^10 or 2^11 over a {50, 36, 36, 50} chain throughout."""
import ctypes as C
import gc
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
BITS = [50, 36, 36, 50]
MSG = {k: f"{k} is not valid for encryption parameters"
       for k in ("encrypted", "plain", "secret key", "public key", "relin_keys", "galois_keys")}


def rand_polys(rng, m, shape_front, level, N):
    a = np.stack([rng.integers(0, m[i], (int(np.prod(shape_front)), N), dtype=np.uint64) for i in range(level)], axis=1)
    return np.ascontiguousarray(a.reshape(*shape_front, level, N))


def one_of_each(ctx, rng, elt):
    """An object of each of the six kinds, all holding device memory."""
    m, N = ctx.moduli, ctx.N
    sk = ctx.keygen_secret(bytes([1] * 64))
    return {"encrypted": ctx.ciphertext(rand_polys(rng, m, (2,), 3, N), 2.0 ** 30),
            "plain": ctx.plaintext(rand_polys(rng, m, (), 3, N), 2.0 ** 30),
            "secret key": sk,
            "public key": ctx.keygen_public(sk, bytes([2] * 64)),
            "relin_keys": ctx.keygen_relin(sk, bytes([3] * 64)),
            "galois_keys": ctx.keygen_galois(sk, [elt], bytes([4] * 64))}


def fresh_context_matches_oracle(orc, hecdna, N, m):
    """A new context (possibly at a destroyed one's address) reproduces the oracle's forward NTT word for word."""
    ctx = hecdna.Context(N, m)
    o = orc.Oracle(N, m)
    a = np.stack([np.stack([np.random.default_rng(9).integers(0, q, N, dtype=np.uint64) for q in m])])
    assert np.array_equal(ctx.ntt(a)[0], np.stack([o.ntt_fwd(i, a[0, i]) for i in range(len(m))]))


def test_calls_on_objects_of_a_closed_context_fail_cleanly(orc, hecdna):
    """Every call that takes an object and no context answers HEC_EINVAL with the kind's SEAL message once the context
    is gone, instead of reading the freed context; the objects are then destroyed after their context."""
    N = 1 << 10
    m = orc.Oracle.create_coeff_modulus(N, BITS)
    ctx = hecdna.Context(N, m)
    rng = np.random.default_rng(1)
    elt = ctx.elt_from_step(1)
    obj = one_of_each(ctx, rng, elt)
    ct, pt, gk = obj["encrypted"], obj["plain"], obj["galois_keys"]
    ct2 = ct.copy()
    data = ct.download()
    ctx.close()
    calls = [(kind, o.download) for kind, o in obj.items() if kind != "galois_keys"]
    calls += [("galois_keys", lambda: gk.download(elt)),
              ("galois_keys", lambda: gk.add_uniform(elt, 5)),
              ("encrypted", lambda: ct.upload(data, 2.0 ** 30)),
              ("encrypted", ct.copy),
              ("encrypted", lambda: hecdna._check(hecdna.lib().hec_ciphertext_copy(ct2.h, ct.h))),
              ("encrypted", lambda: ct.fill_uniform(2, 2, 2.0 ** 30, 3)),
              ("encrypted", ct.save_seal),
              ("plain", lambda: pt.fill_uniform(2, 2.0 ** 30, 3))]
    for kind, call in calls:
        with pytest.raises(hecdna.InvalidArgument) as err:
            call()
        assert str(err.value) == MSG[kind], kind
    del calls, ct, ct2, pt, gk, obj
    gc.collect()
    fresh_context_matches_oracle(orc, hecdna, N, m)


def test_destroys_from_another_thread_while_the_context_closes(orc, hecdna):
    """A finaliser may run on any thread: a worker destroys 32 objects of mixed kinds (ctypes releases the GIL in each
    call) while this thread closes their context.  One pass over the locked path, not a proof: the proof is
    tools/live_host_check.cpp under the sanitizers."""
    N = 1 << 10
    m = orc.Oracle.create_coeff_modulus(N, BITS)
    ctx = hecdna.Context(N, m)
    rng = np.random.default_rng(2)
    elt = ctx.elt_from_step(1)
    objs = []
    for _ in range(4):
        objs += list(one_of_each(ctx, rng, elt).values())
    objs += [ctx.ciphertext(rand_polys(rng, m, (2,), 2, N), 1.0) for _ in range(8)]
    assert len(objs) == 32
    started = threading.Event()

    def worker():
        for o in objs:
            o.__del__()  # the finaliser's body: the C destroy, then h = None
            started.set()

    t = threading.Thread(target=worker)
    t.start()
    started.wait(30)
    ctx.close()
    t.join(60)
    assert not t.is_alive()
    assert all(o.h is None for o in objs)
    fresh_context_matches_oracle(orc, hecdna, N, m)


def test_a_stale_handle_is_refused_by_a_later_context_at_its_address(orc, hecdna):
    """An object records its context's generation, not only its address: a context created where a destroyed one
    lived does not accept the destroyed one's objects (their buffers are sized for other parameters)."""
    N = 1 << 10
    m = orc.Oracle.create_coeff_modulus(N, BITS)
    old = hecdna.Context(N, m)
    rng = np.random.default_rng(3)
    stale_ct = old.ciphertext(rand_polys(rng, m, (2,), 3, N), 2.0 ** 30)
    stale_pt = old.plaintext(rand_polys(rng, m, (), 3, N), 2.0 ** 30)
    addr = old.h.value
    old.close()
    N2 = 1 << 11
    m2 = orc.Oracle.create_coeff_modulus(N2, BITS)
    later = []
    for _ in range(16):
        later.append(hecdna.Context(N2, m2))
        if later[-1].h.value == addr:
            break
    ctx = later[-1]
    if ctx.h.value != addr:
        pytest.skip("none of 16 later contexts was allocated at the closed context's address")
    a = ctx.ciphertext(rand_polys(rng, m2, (2,), 3, N2), 2.0 ** 30)
    for args in ((a, stale_ct), (stale_ct, a)):
        with pytest.raises(hecdna.InvalidArgument, match=MSG["encrypted"]):
            ctx.add(*args)
    with pytest.raises(hecdna.InvalidArgument, match=MSG["plain"]):
        ctx.add_plain(a, stale_pt)


@pytest.mark.parametrize("poison", [0, 1])
def test_every_growth_path_gives_the_oracles_bits(orc, hecdna, poison):
    """Each place a result outgrows its destination's buffer, at N = 2^10 and level 2: add of a size-3 ciphertext into
    a size-2 one (the growth that keeps the contents), multiply into a size-2 ciphertext, decrypt into an empty
    plaintext, encode and encode_scalar into a plaintext that holds a lower level.  With "poison" the new buffers start
    as 0xFF bytes: the words do not change."""
    N, level = 1 << 10, 2
    m = orc.Oracle.create_coeff_modulus(N, BITS)
    o = orc.Oracle(N, m)
    ctx = hecdna.Context(N, m)
    ctx.set_option("poison", poison)
    rng = np.random.default_rng(4)
    lib = hecdna.lib()

    def up(c):
        return ctx.ciphertext(c.data, c.scale)

    def same(g, c):
        assert g.info() == (c.size, c.level, c.scale)
        assert np.array_equal(g.download(), c.data)

    a, b = (orc.Ct(rand_polys(rng, m, (2,), level, N), 2.0 ** 30) for _ in range(2))
    c3 = orc.Ct(rand_polys(rng, m, (3,), level, N), 2.0 ** 30)
    same(ctx.add(up(a), up(c3)), o.add(a, c3))
    same(ctx.multiply(up(a), up(b)), o.multiply(a, b))

    sk_h = o.secret_key(5)
    vals = rng.uniform(-1, 1, N // 2)
    ct = o.encrypt(sk_h, o.encode(vals, 2.0 ** 30, level), 2.0 ** 30, 6)
    pt = ctx.decrypt(ctx.secret_key(sk_h), up(ct))
    assert pt.info() == (level, 2.0 ** 30)
    assert np.array_equal(pt.download(), o.decrypt(sk_h, ct))

    for scalar in (False, True):
        low = ctx.plaintext(rand_polys(rng, m, (), 1, N), 2.0 ** 30)  # holds level 1; the result has level 3
        if scalar:
            hecdna._check(lib.hec_encode_scalar(ctx.h, 0.75, 2.0 ** 30, 3, low.h))
            exp = o.encode_scalar(0.75, 2.0 ** 30, 3)
        else:
            dp = C.POINTER(C.c_double)
            hecdna._check(lib.hec_encode(ctx.h, vals.ctypes.data_as(dp), None, len(vals), 1, 2.0 ** 30, 3,
                                         (C.c_void_p * 1)(low.h.value)))
            exp = o.encode(vals, 2.0 ** 30, 3)
        assert low.info() == (3, 2.0 ** 30)
        assert np.array_equal(low.download(), exp)
