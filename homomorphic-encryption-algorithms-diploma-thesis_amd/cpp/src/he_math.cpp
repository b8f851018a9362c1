// he::math over hecdna (reference src/core/he_math.cpp:22-269).  Each function is the engine's batched call
// (hec_math_*, include/hecdna.h) on a batch of one.  The engine walks the reference's schedule: every scalar constant
// encoded with CKKSEncoder::encode(double, parms_id, scale) at the level and scale of the ciphertext it meets, every
// plaintext and ciphertext product, relinearization and rescale in the reference's order, which is what fixes the output
// bits (CKKS rescaling rounds, so a reordered schedule would be a different ciphertext).  It runs each stage of that
// schedule as one fused launch sequence, measured 2.6 to 3.7 times faster at one ciphertext than the same schedule
// issued one Evaluator call at a time (tools/math_bench.py, profiles/math_bench.json); the results are equal word for
// word.  The encoder and context arguments are kept for the reference's signatures.
#include "he_math.h"

#include <cassert>
#include <stdexcept>

using hecdna::Ciphertext;
using hecdna::CKKSEncoder;
using hecdna::Evaluator;
using hecdna::RelinKeys;

namespace he::math
{
    namespace
    {
        Ciphertext run_one(detail::batch_fn fn, const Evaluator &eval, const RelinKeys &rk, const Ciphertext &x_ct, double a,
                           std::size_t iter_num)
        {
            const hecdna::Context &ctx = eval.context();
            Ciphertext res;
            res.bind(ctx);
            const hec_ciphertext *in = x_ct.get();
            hec_ciphertext *out = res.get();
            hecdna::check(fn(ctx.get(), &in, 1, a, iter_num, rk.get(), &out));
            return res;
        }
    } // namespace

    // 1/x = a prod_k (1 + (1 - a x)^(2^k)), started from 2a - a^2 x (he_math.cpp:22-90)
    Ciphertext signed_inv(const CKKSEncoder &, const Evaluator &eval, const RelinKeys &rk, const Ciphertext &x_ct, double a,
                          std::size_t iter_num)
    {
        assert(iter_num > 0);
        return run_one(hec_math_signed_inv, eval, rk, x_ct, a, iter_num);
    }

    // Newton for 1/sqrt(2x): y' = 3/2 y - x y^3, two levels per step (he_math.cpp:95-164, the `#if 1` form)
    Ciphertext inv_sqrt_twice(const CKKSEncoder &, const Evaluator &eval, const RelinKeys &rk, const Ciphertext &x_ct,
                              double a, std::size_t iter_num)
    {
        assert(iter_num > 0);
        return run_one(hec_math_inv_sqrt_twice, eval, rk, x_ct, a, iter_num);
    }

    // sqrt(x) = (1/sqrt(2x)) (sqrt(2) x) (he_math.cpp:211-232)
    Ciphertext sqrt(const hecdna::Context &, const CKKSEncoder &, const Evaluator &eval, const RelinKeys &rk,
                    const Ciphertext &x_ct, double a, std::size_t iter_num)
    {
        return run_one(hec_math_sqrt, eval, rk, x_ct, a, iter_num);
    }

    // |x| = (1/(sqrt(2)|x|)) (sqrt(2) x^2) (he_math.cpp:237-269)
    Ciphertext abs(const hecdna::Context &, const CKKSEncoder &, const Evaluator &eval, const RelinKeys &rk,
                   const Ciphertext &x_ct, double a, std::size_t iter_num)
    {
        return run_one(hec_math_abs, eval, rk, x_ct, a, iter_num);
    }

    // sum_j coeffs[j] x^j, Paterson-Stockmeyer (an extension; include/hecdna.h hec_math_poly)
    Ciphertext poly(const CKKSEncoder &, const Evaluator &eval, const RelinKeys &rk, const Ciphertext &x_ct,
                    const std::vector<double> &coeffs, std::size_t bs)
    {
        const hecdna::Context &ctx = eval.context();
        Ciphertext res;
        res.bind(ctx);
        const hec_ciphertext *in = x_ct.get();
        hec_ciphertext *out = res.get();
        if (coeffs.empty()) throw std::invalid_argument("polynomial must not be constant");
        hecdna::check(hec_math_poly(ctx.get(), &in, 1, coeffs.data(), coeffs.size() - 1, bs, rk.get(), &out));
        return res;
    }
} // namespace he::math
