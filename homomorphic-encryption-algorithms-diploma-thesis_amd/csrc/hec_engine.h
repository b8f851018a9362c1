// What crosses between the engine's host files (hec_engine.hip, hec_keyswitch.hip), declared once, on top of
// hec_host.h.  hec_batched.hip includes hec_host.h alone and sees only the narrow surface declared there; a
// helper that one file alone uses stays in that file's anonymous namespace and is not declared here.
#pragma once
#include "hec_host.h"

namespace hec {

// ------------------------------------------------------------------ hec_engine.hip
u64 invm(u64 a, u64 q);
u64 *dalloc(std::size_t words);

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

}  // namespace hec
