// The one-object Evaluator calls of the CKKS engine (hec_negate_inplace through hec_apply_galois_inplace): each is
// the B = 1 case of the batched routines in hec_kernels.hip and hec_keyswitch.hip.
#include <algorithm>
#include <vector>

#include "hec_engine.h"

using namespace hec;

namespace {

void add_sub(hec_context *ctx, hec_ciphertext *a, const hec_ciphertext *b, bool sub)
{
    check_ct(ctx, a);
    check_ct(ctx, b);
    set_device(ctx);
    need(a->level == b->level, "encrypted1 and encrypted2 parameter mismatch");
    need(are_close(a->scale, b->scale), "scale mismatch");
    Ctx &c = ctx->c;
    const u64 ps = a->level * c.N;
    const std::size_t mn = std::min(a->size, b->size), mx = std::max(a->size, b->size);
    grow(a, mx * ps, a->size * ps);  // keeping a's polys
    ew_add(c, PolyArr{a->d, 0, ps}, PolyArr{b->d, 0, ps}, PolyArr{a->d, 0, ps}, 1, (int)mn, (int)a->level,
           sub ? 1 : 0);
    if (b->size > a->size) {  // SEAL: copy (add) or negate (sub) the extra polys of b
        const int extra = (int)(b->size - a->size);
        if (sub)
            ew_add(c, PolyArr{a->d + a->size * ps, 0, ps}, PolyArr{b->d + a->size * ps, 0, ps},
                   PolyArr{a->d + a->size * ps, 0, ps}, 1, extra, (int)a->level, 2);
        else
            d2d(c, a->d + a->size * ps, b->d + a->size * ps, extra * ps);
    }
    a->size = mx;
}

void plain_addsub(hec_context *ctx, hec_ciphertext *a, const hec_plaintext *p, bool sub)
{
    check_ct(ctx, a);
    check_plain_data(ctx, p);
    set_device(ctx);
    need(a->level == p->level, "encrypted and plain parameter mismatch");
    need(are_close(a->scale, p->scale), "scale mismatch");
    const u64 ps = a->level * ctx->c.N;
    ew_add(ctx->c, PolyArr{a->d, 0, ps}, PolyArr{p->d, 0, ps}, PolyArr{a->d, 0, ps}, 1, 1, (int)a->level,
           sub ? 1 : 0);
}

void multiply(hec_context *ctx, hec_ciphertext *a, const hec_ciphertext *b)
{
    check_ct(ctx, a);
    check_ct(ctx, b);
    set_device(ctx);
    need(a->level == b->level, "encrypted1 and encrypted2 parameter mismatch");
    const double ns = a->scale * b->scale;
    need(scale_ok(ctx->c, ns, a->level), "scale out of bounds");
    Ctx &c = ctx->c;
    const std::size_t ds = a->size + b->size - 1, ps = a->level * c.N;
    Scratch s(c, ds * ps + 64);
    u64 *tmp = s.take(ds * ps);
    ct_multiply(c, a->d, (int)a->size, b->d, (int)b->size, tmp, (int)a->level);
    grow(a, ds * ps);
    d2d(c, a->d, tmp, ds * ps);
    a->size = ds;
    a->scale = ns;
}

void galois_single(hec_context *ctx, hec_ciphertext *a, const std::vector<u32> &elts, const hec_galois_keys *gk)
{
    Ctx &c = ctx->c;
    const std::size_t l = a->level, N = c.N;
    Scratch s(c, ks_words(c, 1, l) + 2 * l * N + 128);
    const PolyArr x{a->d, 0, l * N};
    for (u32 e : elts) galois_ks(c, s, x, x, 1, (int)l, e, gk->keys.at(e));
}

}  // namespace

// =============================================================================== C-ABI =====
extern "C" {

int hec_negate_inplace(hec_context *ctx, hec_ciphertext *a)
{
    return guard([&] {
        check_ct(ctx, a);
        set_device(ctx);
        ew_negate(ctx->c, PolyArr{a->d, 0, a->level * ctx->c.N}, 1, (int)a->size, (int)a->level);
    });
}

int hec_add_inplace(hec_context *ctx, hec_ciphertext *a, const hec_ciphertext *b)
{
    return guard([&] { add_sub(ctx, a, b, false); });
}
int hec_sub_inplace(hec_context *ctx, hec_ciphertext *a, const hec_ciphertext *b)
{
    return guard([&] { add_sub(ctx, a, b, true); });
}

int hec_add_plain_inplace(hec_context *ctx, hec_ciphertext *a, const hec_plaintext *p)
{
    return guard([&] { plain_addsub(ctx, a, p, false); });
}
int hec_sub_plain_inplace(hec_context *ctx, hec_ciphertext *a, const hec_plaintext *p)
{
    return guard([&] { plain_addsub(ctx, a, p, true); });
}
int hec_multiply_plain_inplace(hec_context *ctx, hec_ciphertext *a, const hec_plaintext *p)
{
    return guard([&] {
        check_ct(ctx, a);
        check_plain_data(ctx, p);
        set_device(ctx);
        need(a->level == p->level, "encrypted_ntt and plain_ntt parameter mismatch");
        const double ns = a->scale * p->scale;
        need(scale_ok(ctx->c, ns, a->level), "scale out of bounds");
        ew_mul_plain(ctx->c, PolyArr{a->d, 0, 0}, p->d, (int)a->size, (int)a->level);
        a->scale = ns;
    });
}

int hec_multiply_inplace(hec_context *ctx, hec_ciphertext *a, const hec_ciphertext *b)
{
    return guard([&] { multiply(ctx, a, b); });
}
int hec_square_inplace(hec_context *ctx, hec_ciphertext *a)
{
    return guard([&] { multiply(ctx, a, a); });
}

int hec_relinearize_inplace(hec_context *ctx, hec_ciphertext *a, const hec_kswitch_key *rk)
{
    return guard([&] {
        check_ct(ctx, a);
        check_obj(ctx, rk, BAD_RK);
        set_device(ctx);
        if (a->size == 2) return;
        need(a->size == 3, "not enough relinearization keys");
        Ctx &c = ctx->c;
        const u64 ps = a->level * c.N;
        Scratch s(c, ks_words(c, 1, a->level));
        const PolyArr io{a->d, 0, ps};
        keyswitch(c, s, PolyArr{a->d + 2 * ps, 0, 0}, rk->d, io, 2, io, 1, (int)a->level);
        a->size = 2;
    });
}

int hec_rescale_to_next_inplace(hec_context *ctx, hec_ciphertext *a)
{
    return guard([&] {
        check_ct(ctx, a);
        set_device(ctx);
        if (a->level == 1) throw std::invalid_argument("end of modulus switching chain reached");
        Ctx &c = ctx->c;
        const std::size_t l = a->level, N = c.N, nk = a->size, So = nk * (l - 1) * N;
        Scratch s(c, rescale_words(c, 1, nk, l) + So + 64);
        u64 *O = s.take(So);
        rescale_batch(c, s, PolyArr{a->d, nk * l * N, l * N}, 1, (int)nk, (int)l, PolyArr{O, So, (l - 1) * N});
        d2d(c, a->d, O, So);
        a->level = l - 1;
        a->scale = a->scale / (double)c.q[l - 1];
    });
}

int hec_mod_switch_to_next_inplace(hec_context *ctx, hec_ciphertext *a)
{
    return guard([&] {
        check_ct(ctx, a);
        set_device(ctx);
        if (a->level == 1) throw std::invalid_argument("end of modulus switching chain reached");
        need(scale_ok(ctx->c, a->scale, a->level - 1), "scale out of bounds");
        Ctx &c = ctx->c;
        const std::size_t l = a->level, N = c.N, nk = a->size;
        Scratch s(c, nk * (l - 1) * N + 64);
        u64 *O = s.take(nk * (l - 1) * N);
        for (std::size_t k = 0; k < nk; ++k) d2d(c, O + k * (l - 1) * N, a->d + k * l * N, (l - 1) * N);
        d2d(c, a->d, O, nk * (l - 1) * N);
        a->level = l - 1;
    });
}

int hec_rotate_vector_inplace(hec_context *ctx, hec_ciphertext *a, int steps, const hec_galois_keys *gk)
{
    return guard([&] {
        check_ct(ctx, a);
        check_obj(ctx, gk, BAD_GK);
        set_device(ctx);
        if (steps == 0) return;  // Evaluator::rotate_internal
        need(a->size == 2, "encrypted size must be 2");
        std::vector<u32> elts;
        rotation_elts(ctx->c, steps, *gk, elts);
        galois_single(ctx, a, elts, gk);
    });
}

int hec_apply_galois_inplace(hec_context *ctx, hec_ciphertext *a, uint32_t elt, const hec_galois_keys *gk)
{
    return guard([&] {
        check_ct(ctx, a);
        check_obj(ctx, gk, BAD_GK);
        set_device(ctx);
        need(gk->keys.count(elt) > 0, "Galois key not present");
        gk_check_elt(ctx->c, elt);
        need(a->size == 2, "encrypted size must be 2");
        galois_single(ctx, a, {elt}, gk);
    });
}

}  // extern "C"
