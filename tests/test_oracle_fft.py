"""CPU: he::fft's constants and the restatement of its two schedules (tests/fft_ref.py) over the oracle.
The twiddles and diagonals of hecdna.fft_twiddles / hecdna.bfft_diagonal (host only: the reference's own libstdc++
expressions, he_fft.cpp:40,55,92-149) agree with numpy's exact roots of unity to 1e-9: a wrong index or sign is off by
at least 2 pi / m (1.5e-3 at m = 4096), the libstdc++ log / polar form by at most 6.3e-14.  The restated schedules
decrypt to np.fft.fft along the ciphertext axis (fft) and to the bit-reversed np.fft.fft of every n-block of the slots
(bfft), the inverses to np.fft.ifft, within 1e-4: a wrong schedule errs at order 1, the schedules' own CKKS error is
at most 1e-5 at these shapes.  These fix the math of the restatement; hec_fft / hec_bfft are then checked bit for bit
against it (tests/test_gpu_fft.py)."""
import numpy as np
import pytest

import fft_ref

TOL = 1e-4


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("m", [2, 4, 8, 64, 4096])
def test_twiddles_match_numpy(hecdna, m, inverse):
    tw = hecdna.fft_twiddles(m, inverse)
    assert tw.shape == (m // 2,)
    exact = np.exp((2j if inverse else -2j) * np.pi * np.arange(m // 2) / m)
    assert np.max(np.abs(tw - exact)) < 1e-9
    assert tw[0].real == 1.0 and tw[0].imag == 0.0  # exactly 1 (its imaginary part is a signed zero)


def test_twiddle_argument_errors(hecdna):
    for m in (0, 1, 3, 12):
        with pytest.raises(hecdna.InvalidArgument):
            hecdna.fft_twiddles(m)
    for d, k, n in [(3, 2, 4), (2, 2, 4), (0, 8, 4), (0, 3, 8), (0, 2, 6), (-1, 2, 4)]:
        with pytest.raises(hecdna.InvalidArgument):
            hecdna.bfft_diagonal(d, k, n)


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("n", [2, 8, 64])
def test_diagonals_pattern_and_values(hecdna, n, inverse):
    lg = n.bit_length() - 1
    for i in range(1, lg + 1):
        k, g = 1 << i, n >> i
        w = np.exp((2j if inverse else -2j) * np.pi * np.arange(g) / (2 * g))
        one, zero = np.ones(g), np.zeros(g)
        d0 = np.concatenate([np.concatenate([one, -w])] * (k // 2))
        if k == 2:
            d1 = np.concatenate([one, w])
        else:
            d1 = np.concatenate([np.concatenate([one, zero])] * (k // 2))
        got0, got1 = hecdna.bfft_diagonal(0, k, n, inverse), hecdna.bfft_diagonal(1, k, n, inverse)
        assert got0.shape == got1.shape == (n,)
        assert np.max(np.abs(got0 - d0)) < 1e-9 and np.max(np.abs(got1 - d1)) < 1e-9
        # the ones and zeros are exact
        assert np.all(got0.reshape(k, g)[0::2] == 1.0)
        assert np.all(got1.reshape(k, g)[0::2] == 1.0)
        if k > 2:
            assert np.all(got1.reshape(k, g)[1::2] == 0.0)
            d2 = np.concatenate([np.concatenate([zero, w])] * (k // 2))
            got2 = hecdna.bfft_diagonal(2, k, n, inverse)
            assert got2.shape == (n,) and np.max(np.abs(got2 - d2)) < 1e-9
            assert np.all(got2.reshape(k, g)[0::2] == 0.0)


@pytest.fixture(scope="module")
def env(orc):
    N = 1 << 11
    m = orc.Oracle.create_coeff_modulus(N, [60] + [40] * 5 + [60])
    o = orc.Oracle(N, m)
    sk = o.secret_key(51)
    gk = o.galois_keys(sk, [o.elt_from_step(s) for s in (1, 2, 4, -1, -2)], 52)
    return N, o, sk, gk


def enc(o, sk, v, seed, level=6, scale=2.0**40):
    return o.encrypt(sk, o.encode(v, scale, level), scale, seed)


def dec(o, sk, ct):
    return o.decode(o.decrypt(sk, ct), ct.scale)


def test_fft_restatement_is_the_dft(env, hecdna):
    N, o, sk, _ = env
    rng = np.random.default_rng(53)
    n = 8
    x = rng.uniform(-1, 1, (n, N // 2)) + 1j * rng.uniform(-1, 1, (n, N // 2))
    out = fft_ref.fft(o, hecdna, [enc(o, sk, x[i], 60 + i) for i in range(n)])
    assert all(c.level == 3 and c.size == 2 for c in out)
    got = np.array([dec(o, sk, c) for c in out])
    assert np.max(np.abs(got - np.fft.fft(x, axis=0))) < TOL


def test_ifft_restatement_undoes_fft(env, hecdna):
    N, o, sk, _ = env
    rng = np.random.default_rng(54)
    n = 4
    x = rng.uniform(-1, 1, (n, N // 2)) + 1j * rng.uniform(-1, 1, (n, N // 2))
    fwd = fft_ref.fft(o, hecdna, [enc(o, sk, x[i], 70 + i) for i in range(n)])
    back = fft_ref.fft(o, hecdna, fwd, inverse=True)
    assert all(c.level == 6 - 2 - 3 for c in back)
    mid = np.array([dec(o, sk, c) for c in fwd])
    assert np.max(np.abs(mid - np.fft.fft(x, axis=0))) < TOL
    assert np.max(np.abs(np.array([dec(o, sk, c) for c in back]) - x)) < TOL
    # n = 1: the forward transform is a copy, the inverse still multiplies by 1 / 1 and rescales
    (c1,) = fft_ref.fft(o, hecdna, fwd[:1], inverse=True)
    assert c1.level == fwd[0].level - 1
    assert np.max(np.abs(dec(o, sk, c1) - mid[0])) < TOL


def test_bfft_restatement_is_the_blockwise_dft_bit_reversed(env, hecdna):
    N, o, sk, gk = env
    rng = np.random.default_rng(55)
    n = 8
    blk = rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)
    x = np.tile(blk, N // 2 // n)
    perm = fft_ref.bitrev_perm(n)
    y = fft_ref.bfft(o, hecdna, enc(o, sk, x, 80), n, gk)
    assert y.level == 3
    got = dec(o, sk, y)
    assert np.max(np.abs(got - np.tile(np.fft.fft(blk)[perm], N // 2 // n))) < TOL
    # the inverse schedule: the bit-reversed inverse DFT; applied to the forward result put back in natural order
    # (re-encrypted) it returns the input
    z = fft_ref.bfft(o, hecdna, enc(o, sk, x, 81), n, gk, inverse=True)
    assert z.level == 2
    assert np.max(np.abs(dec(o, sk, z) - np.tile(np.fft.ifft(blk)[perm], N // 2 // n))) < TOL
    nat = np.empty(n, dtype=complex)
    nat[perm] = got[:n]
    back = fft_ref.bfft(o, hecdna, enc(o, sk, np.tile(nat, N // 2 // n), 82), n, gk, inverse=True)
    und = np.empty(n, dtype=complex)
    und[perm] = dec(o, sk, back)[:n]
    assert np.max(np.abs(und - blk)) < TOL


def test_new_symbols_are_declared(hecdna):
    syms = hecdna.exported_symbols()
    for s in ("hec_fft", "hec_bfft", "hec_fft_twiddles", "hec_bfft_diagonal"):
        assert s in syms
    L = hecdna.lib()
    for s in ("hec_fft", "hec_bfft", "hec_fft_twiddles", "hec_bfft_diagonal"):
        assert getattr(L, s) is not None
