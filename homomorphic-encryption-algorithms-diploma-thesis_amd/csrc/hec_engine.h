// What crosses between the engine's host files (hec_engine.hip, hec_keyswitch.hip, hec_matvec.hip, hec_shard.hip,
// hec_client.hip, hec_evaluator.hip), declared once, on top of hec_host.h, one section per defining file.
// hec_batched.hip includes hec_host.h alone and sees only the narrow surface declared there; a helper that one file
// alone uses stays in that file's anonymous namespace and is not declared here.
#pragma once
#include <memory>

#include "hec_host.h"

namespace hec {

// ------------------------------------------------------------------ hec_engine.hip
u64 invm(u64 a, u64 q);
std::vector<int> naf(int value);  // SEAL util::naf: least-significant term first
u64 *dalloc(std::size_t words);
void bind(DevObject &o, hec_context *ctx);
// A new object of ctx, owned until the constructor releases it into *out: a constructor that throws destroys it.
template <class T, int (*Destroy)(T *)>
auto make(hec_context *ctx)
{
    struct Del {
        void operator()(T *o) const { (void)Destroy(o); }
    };
    std::unique_ptr<T, Del> o(new T());
    bind(*o, ctx);
    return o;
}
void check_plain_data(const hec_context *ctx, const hec_plaintext *p);  // holds data; the caller compares the level
void check_plain(const hec_context *ctx, const hec_plaintext *p);
void check_pk(const hec_context *ctx, const hec_public_key *pk);
// Calls that take an object and no context: the object's context must still exist; selects its device
Ctx &live(const DevObject *o, const char *msg);

// A ciphertext's or plaintext's buffer of at least `words` words: at once when the capacity suffices (a warmed-up
// loop never waits here), else a new buffer holding the first keep_words words of the old one, the rest poisoned
// under c.poison.  The old buffer goes only after the context's stream has drained: enqueued work may still read it.
template <class T>
void grow(T *o, std::size_t words, std::size_t keep_words = 0)
{
    if (o->cap >= words) return;
    Ctx &c = o->ctx->c;
    u64 *nd = keep_words ? dalloc(words) : nullptr;
    if (keep_words) d2d(c, nd, o->d, keep_words);
    if (o->d) {
        HEC_HIP(hipStreamSynchronize(c.stream));
        HEC_HIP(hipFree(o->d));
        o->d = nullptr;
        o->cap = 0;
    }
    o->d = nd ? nd : dalloc(words);
    o->cap = words;
    if (c.poison) dev_fill(c, o->d + keep_words, 0xFFFFFFFFu, (words - keep_words) * sizeof(u64));
}
std::size_t key_words(const Ctx &c);  // the words of one key-switch key
void gk_check_elt(const Ctx &c, u32 elt);

// ------------------------------------------------------------------ hec_keyswitch.hip
// the mod-down of one key switch, and of ng sibling rotations of one hoisted node at once
void moddown(Ctx &c, u64 *ACC, u64 *Z, PolyArr IN, int in_nk, PolyArr OUT, int B, int l, u32 elt,
             PolyArr ADD = PolyArr{});
void moddown_group(Ctx &c, u64 *ACC, u64 *Z, PolyArr IN, int in_nk, const PolyArr *OUT, const u32 *elts, int ng,
                   int B, int l);
// OUT = key switch of the B targets T at level l, plus perm(IN) [+ ADD]
void keyswitch(Ctx &c, Scratch &s, PolyArr T, const u64 *key, PolyArr IN, int in_nk, PolyArr OUT, int B, int l,
               u32 elt = 1, PolyArr ADD = PolyArr{});
// hoisted mod-up data of one trie node (B targets at level l): D = INTT(c1) (canonical coefficient form),
// E[b][I][J] = NTT_I(D_J mod q_I) (canonical NTT form, J != I), zero lists of D (see hec_kernels.hip)
constexpr int HOIST_GROUP = 6;  // sibling rotations per grouped mod-down (and per k_hmacm accumulator set)
struct Hoist {
    u64 *D = nullptr, *E = nullptr;
    int *zl = nullptr;
    // key-switch accumulators of up to HOIST_GROUP siblings, contiguous (moddown_group), live across the recursion
    // into their subtrees
    u64 *acc0 = nullptr;
    u64 sacc = 0;
    u64 *acc(int q) const { return acc0 + (u64)q * sacc; }
};
std::size_t hoist_words(const Ctx &c, std::size_t B, std::size_t l);
Hoist hoist_alloc(const Ctx &c, Scratch &s, int B, int l);
void hoist_node(Ctx &c, PolyArr X, int B, int l, const Hoist &h);
void hoisted_child(Ctx &c, Scratch &s, PolyArr X, const Hoist &h, const u64 *W, const u64 *key, PolyArr OUT, int B,
                   int l, u32 elt);
std::size_t hoisted_child_words(const Ctx &c, std::size_t B, std::size_t l);
// the per-key tables of a Galois key, built on first use
const u64 *galois_negw(hec_context *ctx, hec_galois_keys &gk, u32 elt);
const u64 *galois_kw(hec_context *ctx, hec_galois_keys &gk, u32 elt, int l);
const u64 *galois_mkey(hec_context *ctx, hec_galois_keys &gk, u32 elt);
// divide-and-round by q_{l-1}: X = B entries of nk polys at level l -> OUT at level l-1
void rescale_batch(Ctx &c, Scratch &s, PolyArr X, int B, int nk, int l, PolyArr OUT);

// ------------------------------------------------------------------ hec_matvec.hip
// the argument checks of a diag x col matvec over the diagonals js, in SEAL's order; the product scale of every output
std::vector<double> matvec_check(hec_context *ctx, const hec_ciphertext *const *diags, const hec_plaintext *const *pdiags,
                                 std::size_t n, const std::vector<std::size_t> &js, const hec_ciphertext *const *cols,
                                 std::size_t p, const hec_kswitch_key *rk, const hec_galois_keys *gk, bool finish);
// the matvec over the context's batch lanes
void matvec_lanes(hec_context *ctx, const hec_ciphertext *const *diags, const hec_plaintext *const *pdiags,
                  std::size_t n, const std::vector<std::size_t> &js, const hec_ciphertext *const *cols, std::size_t p,
                  const hec_kswitch_key *rk, const hec_galois_keys *gk, bool finish, hec_ciphertext *const *out);
void free_lane(hec_context *l);
void debug_key_tables_forget(const hec_galois_keys *gk);

}  // namespace hec
