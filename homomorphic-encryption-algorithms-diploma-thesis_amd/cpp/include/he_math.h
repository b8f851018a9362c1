#pragma once
// Drop-in for the reference's he::math (include/he_math.h:6-34) over hecdna types: Newton / Goldschmidt iterations
// for 1/x, 1/sqrt(2x), sqrt(x) and |x| on CKKS ciphertexts.  Each function issues the reference's sequence of
// scalar encodes, plaintext and ciphertext products, relinearizations and rescales (src/core/he_math.cpp:22-269),
// so on the same inputs and keys every intermediate ciphertext equals SEAL's bit for bit.
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <vector>

#include "he_operators.h"
#include "hecdna/seal_compat.hpp"

namespace he::math
{
    // f(x) = 1/x; a predicts the result with |a x - 1| < 1 (he_math.h:8-15)
    hecdna::Ciphertext signed_inv(const hecdna::CKKSEncoder &cencd, const hecdna::Evaluator &eval, const hecdna::RelinKeys &rk,
                                  const hecdna::Ciphertext &x_ct, double a, std::size_t iter_num);

    // f(x) = 1/sqrt(2x), x > 0; 0 < a < sqrt(3/(2x)) (he_math.h:17-23)
    hecdna::Ciphertext inv_sqrt_twice(const hecdna::CKKSEncoder &cencd, const hecdna::Evaluator &eval, const hecdna::RelinKeys &rk,
                                      const hecdna::Ciphertext &x_ct, double a, std::size_t iter_num);

    // f(x) = sqrt(x) (he_math.h:25-28)
    hecdna::Ciphertext sqrt(const hecdna::Context &ctx, const hecdna::CKKSEncoder &cencd, const hecdna::Evaluator &eval,
                            const hecdna::RelinKeys &rk, const hecdna::Ciphertext &x_ct, double a, std::size_t iter_num);

    // f(x) = |x| (he_math.h:30-33)
    hecdna::Ciphertext abs(const hecdna::Context &ctx, const hecdna::CKKSEncoder &cencd, const hecdna::Evaluator &eval,
                           const hecdna::RelinKeys &rk, const hecdna::Ciphertext &x_ct, double a, std::size_t iter_num);

    // An extension (the reference has no such function): f(x) = sum_j coeffs[j] x^j by Paterson-Stockmeyer with
    // block size bs (a power of two in [2, 16]; 0: chosen from the degree), one engine call (hec_math_poly,
    // include/hecdna.h; the schedule is DESIGN.md 2.9).  The result keeps x_ct's scale.  Real coefficients; the
    // polynomial must not be constant
    hecdna::Ciphertext poly(const hecdna::CKKSEncoder &cencd, const hecdna::Evaluator &eval, const hecdna::RelinKeys &rk,
                            const hecdna::Ciphertext &x_ct, const std::vector<double> &coeffs, std::size_t bs = 0);

    // An extension (the reference has no such overloads): the same four functions on a vector of ciphertexts of one
    // level and scale, each one engine call (hec_math_*, include/hecdna.h) that runs every stage of the schedule
    // above over the whole batch.  Result i equals the single-ciphertext function on x_cts[i], bit for bit.  The
    // encoder argument is kept for the signature: the engine forms the scalar constants itself.
    namespace detail
    {
        using batch_fn = int (*)(hec_context *, const hec_ciphertext *const *, std::uint64_t, double, std::uint64_t,
                                 const hec_kswitch_key *, hec_ciphertext *const *);
        inline std::vector<hecdna::Ciphertext> run(batch_fn fn, const hecdna::Evaluator &eval, const hecdna::RelinKeys &rk,
                                                   const std::vector<hecdna::Ciphertext> &x_cts, double a,
                                                   std::size_t iter_num)
        {
            const hecdna::Context &ctx = eval.context();
            std::vector<hecdna::Ciphertext> res(x_cts.size());
            std::vector<const hec_ciphertext *> in(x_cts.size());
            std::vector<hec_ciphertext *> out(x_cts.size());
            for (std::size_t i = 0; i < x_cts.size(); ++i) {
                res[i].bind(ctx);
                in[i] = x_cts[i].get();
                out[i] = res[i].get();
            }
            hecdna::check(fn(ctx.get(), in.data(), in.size(), a, iter_num, rk.get(), out.data()));
            return res;
        }
    } // namespace detail

    // poly on a vector of ciphertexts of one level and scale: one engine call over the whole batch
    inline std::vector<hecdna::Ciphertext> poly(const hecdna::CKKSEncoder &, const hecdna::Evaluator &eval,
                                                const hecdna::RelinKeys &rk, const std::vector<hecdna::Ciphertext> &x_cts,
                                                const std::vector<double> &coeffs, std::size_t bs = 0)
    {
        const hecdna::Context &ctx = eval.context();
        std::vector<hecdna::Ciphertext> res(x_cts.size());
        std::vector<const hec_ciphertext *> in(x_cts.size());
        std::vector<hec_ciphertext *> out(x_cts.size());
        for (std::size_t i = 0; i < x_cts.size(); ++i) {
            res[i].bind(ctx);
            in[i] = x_cts[i].get();
            out[i] = res[i].get();
        }
        if (coeffs.empty()) throw std::invalid_argument("polynomial must not be constant");
        hecdna::check(hec_math_poly(ctx.get(), in.data(), in.size(), coeffs.data(), coeffs.size() - 1, bs, rk.get(),
                                    out.data()));
        return res;
    }

    inline std::vector<hecdna::Ciphertext> signed_inv(const hecdna::CKKSEncoder &, const hecdna::Evaluator &eval,
                                                      const hecdna::RelinKeys &rk,
                                                      const std::vector<hecdna::Ciphertext> &x_cts, double a,
                                                      std::size_t iter_num)
    {
        return detail::run(hec_math_signed_inv, eval, rk, x_cts, a, iter_num);
    }
    inline std::vector<hecdna::Ciphertext> inv_sqrt_twice(const hecdna::CKKSEncoder &, const hecdna::Evaluator &eval,
                                                          const hecdna::RelinKeys &rk,
                                                          const std::vector<hecdna::Ciphertext> &x_cts, double a,
                                                          std::size_t iter_num)
    {
        return detail::run(hec_math_inv_sqrt_twice, eval, rk, x_cts, a, iter_num);
    }
    inline std::vector<hecdna::Ciphertext> sqrt(const hecdna::Context &, const hecdna::CKKSEncoder &,
                                                const hecdna::Evaluator &eval, const hecdna::RelinKeys &rk,
                                                const std::vector<hecdna::Ciphertext> &x_cts, double a,
                                                std::size_t iter_num)
    {
        return detail::run(hec_math_sqrt, eval, rk, x_cts, a, iter_num);
    }
    inline std::vector<hecdna::Ciphertext> abs(const hecdna::Context &, const hecdna::CKKSEncoder &,
                                               const hecdna::Evaluator &eval, const hecdna::RelinKeys &rk,
                                               const std::vector<hecdna::Ciphertext> &x_cts, double a,
                                               std::size_t iter_num)
    {
        return detail::run(hec_math_abs, eval, rk, x_cts, a, iter_num);
    }
} // namespace he::math
