// Host-side constants of he::fft (reference src/core/he_fft.cpp:40,55 and :92-149): the twiddle factors of the
// FFT over ciphertexts and the three diagonals of one in-slot FFT stage, as doubles.  The reference computes
// them with std::exp and std::pow(std::complex<double>, size_t), which libstdc++ evaluates as polar(exp(k log|w|),
// k arg w), not as a repeated product, so pow(w, 0) is (1, -0) and the values are not the exactly rounded roots of
// unity.  The encoder turns these doubles into plaintext words, so every user (the engine, the C++ drop-in, the
// tests' restatement) takes them from this one file, built by the host compiler with -ffp-contract=off and no
// fast-math.  No device is needed.
#include <cmath>
#include <complex>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "hecdna.h"

namespace {
using Complex = std::complex<double>;

bool pow2(uint64_t x) { return x && !(x & (x - 1)); }

// exp(i s (-2 pi) / m), s = +1 forward, -1 inverse
Complex root(uint64_t m, int inverse)
{
    const int s = inverse ? -1 : 1;
    return std::exp(Complex(0, s * -2 * M_PI / m));
}
}  // namespace

extern "C" int hec_fft_twiddles(uint64_t m, int inverse, double *re, double *im)
{
    if (!pow2(m) || m < 2 || !re || !im) return HEC_EINVAL;
    const Complex w = root(m, inverse);
    for (std::size_t k = 0; k < m / 2; ++k) {
        const Complex p = std::pow(w, k);
        re[k] = p.real();
        im[k] = p.imag();
    }
    return HEC_OK;
}

extern "C" int hec_bfft_diagonal(int d, uint64_t k, uint64_t n, int inverse, double *re, double *im)
{
    if (!pow2(n) || !pow2(k) || k < 2 || k > n || d < 0 || d > 2 || (d == 2 && k == 2) || !re || !im)
        return HEC_EINVAL;
    const uint64_t g = n / k;  // run length: the stage rotates by g slots
    const Complex w = root(g * 2, inverse);
    std::vector<Complex> wp(g);
    for (std::size_t i = 0; i < g; ++i) wp[i] = std::pow(w, i);
    // runs of g slots, k of them: run r holds ones, zeros, w^i or -w^i
    enum Run { ZERO, ONE, W, NEGW };
    std::vector<Run> runs(k, ZERO);
    if (d == 0) {
        for (uint64_t r = 0; r < k; ++r) runs[r] = (r & 1) ? NEGW : ONE;
    } else if (d == 1) {
        for (uint64_t r = 0; r < k; r += 2) runs[r] = ONE;
        if (k == 2) runs[1] = W;
    } else {
        for (uint64_t r = 1; r < k; r += 2) runs[r] = W;
    }
    for (uint64_t r = 0; r < k; ++r)
        for (uint64_t i = 0; i < g; ++i) {
            Complex v(0, 0);
            if (runs[r] == ONE) v = Complex(1);
            else if (runs[r] == W) v = wp[i];
            else if (runs[r] == NEGW) v = -wp[i];
            re[r * g + i] = v.real();
            im[r * g + i] = v.imag();
        }
    return HEC_OK;
}
