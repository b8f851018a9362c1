#pragma once
// Drop-in for the reference's he::fft (include/he_fft.h:7-28) over hecdna types: the radix-2 FFT over a vector of
// ciphertexts and the in-slot ("batched") FFT of one ciphertext.  Each function is one engine call (hec_fft /
// hec_bfft, include/hecdna.h) that runs the reference's sequence of encodes, plaintext products, rescales,
// rotations, sums and differences (src/core/he_fft.cpp:13-223) a whole stage at a time, so on the same inputs and
// keys the results equal the reference schedule's bit for bit.  The encoder argument is kept for the signature: the
// engine encodes the twiddles itself, from the doubles of hec_fft_twiddles / hec_bfft_diagonal.
// The four functions are thin calls and are defined here, inline: a program that uses them links against
// libhecdna.so alone, with no further source file of the drop-in.
#include <cstddef>
#include <vector>

#include "hecdna/seal_compat.hpp"

namespace he::fft
{
    namespace detail
    {
        inline std::vector<hecdna::Ciphertext> run_fft(const hecdna::Evaluator &eval,
                                                       const std::vector<hecdna::Ciphertext> &vec_ct, int inverse)
        {
            const hecdna::Context &ctx = eval.context();
            std::vector<hecdna::Ciphertext> res(vec_ct.size());
            std::vector<const hec_ciphertext *> in(vec_ct.size());
            std::vector<hec_ciphertext *> out(vec_ct.size());
            for (std::size_t i = 0; i < vec_ct.size(); ++i) {
                res[i].bind(ctx);
                in[i] = vec_ct[i].get();
                out[i] = res[i].get();
            }
            hecdna::check(hec_fft(ctx.get(), in.data(), in.size(), inverse, out.data()));
            return res;
        }
        inline hecdna::Ciphertext run_bfft(const hecdna::Evaluator &eval, const hecdna::GaloisKeys &gk,
                                           const hecdna::Ciphertext &x_ct, std::size_t n, int inverse)
        {
            const hecdna::Context &ctx = eval.context();
            hecdna::Ciphertext res;
            res.bind(ctx);
            const hec_ciphertext *in = x_ct.get();
            hec_ciphertext *out = res.get();
            hecdna::check(hec_bfft(ctx.get(), &in, 1, n, inverse, gk.get(), &out));
            return res;
        }
    } // namespace detail

    // FFT over the ciphertexts of vec_ct (he_fft.h:9-12); vec_ct.size() a power of two
    inline std::vector<hecdna::Ciphertext> fft(const hecdna::CKKSEncoder &, const hecdna::Evaluator &eval,
                                               const std::vector<hecdna::Ciphertext> &vec_ct)
    {
        return detail::run_fft(eval, vec_ct, 0);
    }

    // inverse FFT over the ciphertexts of vec_ct (he_fft.h:14-17)
    inline std::vector<hecdna::Ciphertext> ifft(const hecdna::CKKSEncoder &, const hecdna::Evaluator &eval,
                                                const std::vector<hecdna::Ciphertext> &vec_ct)
    {
        return detail::run_fft(eval, vec_ct, 1);
    }

    // FFT of every n-block of the slots of x_ct, whose slot vector is n-periodic (he_fft.h:19-22); each block of the
    // result is in bit-reversed order
    inline hecdna::Ciphertext bfft(const hecdna::CKKSEncoder &, const hecdna::Evaluator &eval, const hecdna::GaloisKeys &gk,
                                   const hecdna::Ciphertext &x_ct, std::size_t n)
    {
        return detail::run_bfft(eval, gk, x_ct, n, 0);
    }

    // its inverse schedule with the 1/n step (he_fft.h:24-27)
    inline hecdna::Ciphertext ibfft(const hecdna::CKKSEncoder &, const hecdna::Evaluator &eval, const hecdna::GaloisKeys &gk,
                                    const hecdna::Ciphertext &x_ct, std::size_t n)
    {
        return detail::run_bfft(eval, gk, x_ct, n, 1);
    }
} // namespace he::fft
