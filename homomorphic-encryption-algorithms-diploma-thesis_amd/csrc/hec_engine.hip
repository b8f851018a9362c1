// Host orchestration + C-ABI of the CKKS engine (include/hecdna.h).
//
// Every public entry point restates one seal::Evaluator call that the reference's he_operators /
// he_linalg layer makes (file:line cited per function in hecdna.h), on device-resident SEAL-layout
// objects.  Internally all ciphertext work is BATCHED: the key switch, rotation and rescale
// routines take B ciphertexts in one strided array so that one launch sequence (and one read of
// the key) serves the whole batch; the single-object C-ABI calls are the B = 1 case.
//
// This file holds the objects' lifecycle, context setup and options, the rotation trie and the matvec, the evaluator
// calls, encode, decode, keygen and the wire-format glue, the sharded calls, the primitives and the profile calls.
// The key switch is in hec_keyswitch.hip; what crosses between the two files is declared in
// hec_engine.h.  The library-level layers over many ciphertexts (he::fft, he::math, he::linalg's element-wise
// products and slot sums) live in hec_batched.hip, written over the building blocks that hec_host.h declares; the
// object structs, the error guard, Scratch and ProfScope are in hec_host.h as well.
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <limits>
#include <memory>
#include <mutex>
#include <numeric>
#include <set>
#include <thread>
#include <tuple>

#include "hec_engine.h"
#include "hec_keygen_host.h"
#include "hec_live.h"

#include <array>
#include <dlfcn.h>
#include <unistd.h>
#include <rccl/rccl.h>

using namespace hec;
using u128 = unsigned __int128;

thread_local std::string hec::g_err;

namespace {

// ------------------------------------------------------------------ host number theory -----
u64 powm(u64 b, u64 e, u64 q)
{
    u64 r = 1 % q;
    b %= q;
    for (; e; e >>= 1) {
        if (e & 1) r = (u64)((u128)r * b % q);
        b = (u64)((u128)b * b % q);
    }
    return r;
}
bool isprime(u64 n)
{
    if (n < 2) return false;
    static const u64 sp[] = {2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37};
    for (u64 p : sp) {
        if (n % p == 0) return n == p;
    }
    u64 d = n - 1;
    int s = 0;
    while (!(d & 1)) { d >>= 1; ++s; }
    for (u64 a : sp) {
        u64 x = powm(a, d, n);
        if (x == 1 || x == n - 1) continue;
        bool composite = true;
        for (int i = 1; i < s && composite; ++i) {
            x = (u64)((u128)x * x % n);
            if (x == n - 1) composite = false;
        }
        if (composite) return false;
    }
    return true;
}
u64 shoupq(u64 w, u64 q) { return (u64)(((u128)w << 64) / q); }
}  // namespace
// Here and below, a `namespace hec` block holds a building block that another file calls (hec_host.h declares it for
// hec_batched.hip, hec_engine.h for hec_keyswitch.hip); the rest of this file's helpers stay in the anonymous
// namespace.
namespace hec {
u64 invm(u64 a, u64 q)
{
    __int128 t = 0, nt = 1, r = q, nr = a % q;
    while (nr) {
        const __int128 k = r / nr;
        __int128 x = t - k * nt; t = nt; nt = x;
        x = r - k * nr; r = nr; nr = x;
    }
    if (r != 1) throw std::invalid_argument("value is not invertible");
    return (u64)(t < 0 ? t + q : t);
}
u32 brev(u32 x, int bits)
{
    u32 r = 0;
    for (int i = 0; i < bits; ++i) r |= ((x >> i) & 1u) << (bits - 1 - i);
    return r;
}
}  // namespace hec
namespace {
// SEAL util::try_minimal_primitive_root: the smallest primitive 2N-th root of unity mod q
u64 minimal_root(u64 two_n, u64 q)
{
    u64 g = 0;
    for (u64 x = 2; x < q && !g; ++x) {
        const u64 c = powm(x, (q - 1) / two_n, q);
        if (powm(c, two_n / 2, q) == q - 1) g = c;
    }
    if (!g) throw std::logic_error("no primitive root found");
    const u64 g2 = (u64)((u128)g * g % q);
    u64 cur = g, best = g;
    for (u64 k = 0; k < two_n / 2; ++k) {
        best = std::min(best, cur);
        cur = (u64)((u128)cur * g2 % q);
    }
    return best;
}
}  // namespace
namespace hec {
bool are_close(double a, double b)  // SEAL util::are_close
{
    const double sf = std::max({std::fabs(a), std::fabs(b), 1.0});
    return std::fabs(a - b) < std::numeric_limits<double>::epsilon() * sf;
}
bool scale_ok(const Ctx &c, double scale, std::size_t level)  // SEAL is_scale_within_bounds
{
    return !(scale <= 0 || (int)std::log2(scale) >= c.total_bits(level));
}
}  // namespace hec
namespace {
std::vector<int> naf(int value)  // SEAL util::naf: least-significant term first
{
    std::vector<int> res;
    const bool sign = value < 0;
    value = std::abs(value);
    for (int i = 0; value; ++i) {
        const int zi = (value & 1) ? 2 - (value & 3) : 0;
        value = (value - zi) >> 1;
        if (zi) res.push_back((sign ? -zi : zi) * (1 << i));
    }
    return res;
}
}  // namespace
namespace hec {
u32 elt_from_step(const Ctx &c, int step)  // SEAL GaloisTool::get_elt_from_step
{
    const u32 n = (u32)c.N, m = 2 * n;
    if (step == 0) return m - 1;
    const bool sign = step < 0;
    u32 pos = (u32)std::abs(step);
    if (pos >= (n >> 1)) throw std::invalid_argument("step count too large");
    pos &= m - 1;
    int s = sign ? (int)(n >> 1) - (int)pos : (int)pos;
    u64 elt = 1;
    while (s--) { elt *= 3; elt &= m - 1; }
    return (u32)elt;
}
// SEAL Evaluator::rotate_internal flattened into the sequence of Galois elements it applies
void rotation_elts(const Ctx &c, int steps, const hec_galois_keys &gk, std::vector<u32> &out)
{
    if (steps == 0) return;
    const u32 elt = elt_from_step(c, steps);
    if (gk.keys.count(elt)) { out.push_back(elt); return; }
    const std::vector<int> terms = naf(steps);
    if (terms.size() == 1) throw std::invalid_argument("Galois key not present");
    for (int s : terms)
        if ((std::size_t)std::abs(s) != (c.N >> 1)) rotation_elts(c, s, gk, out);
}

// ------------------------------------------------------------------ device memory ----------
u64 *dalloc(std::size_t words)
{
    void *p = nullptr;
    if (words == 0) words = 1;
    HEC_HIP(hipMalloc(&p, words * sizeof(u64)));
    return (u64 *)p;
}
}  // namespace hec
namespace {

// ------------------------------------------------------------------ profiling -------------
// the pending event pairs of ProfScope (hec_host.h) under prof_mode 2, resolved when the profile is read
void prof_resolve(Ctx &c)
{
    if (c.prof_pend.empty()) return;
    HEC_HIP(hipStreamSynchronize(c.stream));
    for (const auto &p : c.prof_pend) {
        float ms = 0;
        HEC_HIP(hipEventElapsedTime(&ms, p.e0, p.e1));
        auto &r = c.prof_tab[p.name];
        r.ms += ms;
        r.n += 1;
        r.bytes += p.bytes;
        r.kl += p.kl;
    }
    c.prof_pend.clear();
    c.ev_used = 0;
}

}  // namespace
namespace hec {
void set_device(hec_context *ctx)
{
    need(ctx != nullptr, "context is null");
    HEC_HIP(hipSetDevice(ctx->c.device));
}

void d2d(Ctx &c, void *dst, const void *src, std::size_t words)
{
    if (!words) return;
    if (c.kernel_memops) dev_copy64(c, (u64 *)dst, (const u64 *)src, words);
    else HEC_HIP(hipMemcpyAsync(dst, src, words * sizeof(u64), hipMemcpyDeviceToDevice, c.stream));
}
}  // namespace hec
namespace {

// ------------------------------------------------------------------ device objects ---------
void bind(DevObject &o, hec_context *ctx)
{
    o.ctx = ctx;
    o.ctx_gen = ctx->gen;
    o.device = ctx->c.device;
}
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
}  // namespace
namespace hec {
// Calls that take a context: the object must belong to this very context (a later context at the same address has
// another generation).
void check_obj(const hec_context *ctx, const DevObject *o, const char *msg)
{
    need(o && o->ctx == ctx && o->ctx_gen == ctx->gen, msg);
}
void check_ct(const hec_context *ctx, const hec_ciphertext *a)
{
    check_obj(ctx, a, BAD_CT);
    need(a->level >= 1 && a->level <= ctx->c.L && a->size >= 2 && a->d, BAD_CT);
}
void check_out_alias(const std::vector<const hec_ciphertext *const *> &ins, hec_ciphertext *const *out, uint64_t B,
                     const hec_context *ctx, const hec_ciphertext *const *never, uint64_t n_never)
{
    constexpr const char *msg = "an output may alias only its own entry's inputs";
    std::map<const hec_ciphertext *, uint64_t> o;
    for (uint64_t i = 0; i < B; ++i) {
        if (ctx) check_obj(ctx, out[i], BAD_CT);
        need(o.emplace(out[i], i).second, msg);
    }
    for (const hec_ciphertext *const *in : ins)
        for (uint64_t i = 0; i < B; ++i) {
            const auto it = o.find(in[i]);
            need(it == o.end() || it->second == i, msg);
        }
    for (uint64_t j = 0; j < n_never; ++j) need(o.find(never[j]) == o.end(), msg);
}
}  // namespace hec
namespace {
void check_plain_data(const hec_context *ctx, const hec_plaintext *p)  // holds data; the caller compares the level
{
    check_obj(ctx, p, BAD_PLAIN);
    need(p->d != nullptr, BAD_PLAIN);
}
void check_plain(const hec_context *ctx, const hec_plaintext *p)
{
    check_plain_data(ctx, p);
    need(p->level >= 1 && p->level <= ctx->c.L, BAD_PLAIN);
}
void check_pk(const hec_context *ctx, const hec_public_key *pk)
{
    check_obj(ctx, pk, BAD_PK);
    need(pk->d != nullptr, BAD_PK);
}
// Calls that take an object and no context: the object's context must still exist, checked before anything is read
// through o->ctx; selects its device.  The registry lock is not held across the caller's work: one host thread
// drives a context (hecdna.h), only destroys arrive from other threads.
Ctx &live(const DevObject *o, const char *msg)
{
    need(hec_live::while_alive(o->ctx, o->ctx_gen, [] {}), msg);
    set_device(o->ctx);
    return o->ctx->c;
}

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

}  // namespace
namespace hec {
// The one output store: o becomes `size` polys of `level` limbs copied from src.  grow() comes before the copy (it may
// drain the stream and free the old buffer).  A call whose outputs may be its inputs reads what it needs of the inputs'
// host fields before its first store, and enqueues its gathers before it
void store_ct(Ctx &c, hec_ciphertext *o, const u64 *src, std::size_t size, std::size_t level, double scale)
{
    const std::size_t w = size * level * c.N;
    grow(o, w);
    d2d(c, o->d, src, w);
    o->size = size; o->level = level; o->scale = scale;
}
}  // namespace hec
namespace {

// The device memory an object owns
template <class T>
std::vector<u64 *> owned(const T &o)
{
    return {o.d};
}
std::vector<u64 *> owned(const hec_galois_keys &gk)
{
    std::vector<u64 *> v;
    for (const auto &kv : gk.keys) v.push_back(kv.second);
    for (const auto &kv : gk.negw) v.push_back(kv.second);
    for (const auto &kv : gk.kw) v.push_back(kv.second);
    for (const auto &kv : gk.mkey) v.push_back(kv.second);
    return v;
}
// The one destroy.  On the object's device: while its context lives, drain the context's stream (enqueued work may
// still read the object), then free what the object owns; after its context the object frees its own memory and
// touches nothing else.  wipe_words: SEAL wipes a secret key's memory when it goes, so that many words are
// zero-filled first with the engine's fill kernel, on the context's stream or else on the device's null stream.
template <class T>
int release(T *o, std::size_t wipe_words = 0)
{
    return guard([&] {
        if (!o) return;
        (void)hipSetDevice(o->device);
        const std::vector<u64 *> mem = owned(*o);
        auto drain = [&](hipStream_t st) {
            try {
                if (wipe_words) {
                    Ctx wipe;
                    wipe.stream = st;
                    dev_fill32(wipe, mem[0], 0, wipe_words * sizeof(u64));
                }
            } catch (...) {  // the memory is freed all the same
            }
            (void)hipStreamSynchronize(st);
        };
        const bool holds = std::any_of(mem.begin(), mem.end(), [](const u64 *p) { return p != nullptr; });
        const bool alive = holds && hec_live::while_alive(o->ctx, o->ctx_gen, [&] { drain(o->ctx->c.stream); });
        if (holds && !alive && wipe_words) drain(nullptr);
        for (u64 *p : mem) (void)hipFree(p);
        delete o;
    });
}

// ------------------------------------------------------------------ he::linalg driver -----
struct MatvecPlan {
    std::size_t l = 0;
    double prod_scale = 0;
    std::vector<std::vector<u32>> elts;  // per diagonal j
};

// Rotation prefix trie.  SEAL's rotate_internal turns rot(x, j) into a fixed sequence of key
// switches (one per NAF term, least significant first).  Rotations of the SAME input by different
// j share prefixes of that sequence (rot by 5 = KS_4(KS_1(x)) starts with rot by 1), so a
// depth-first walk over the trie of sequences computes every distinct prefix once: each rot(x, j)
// is still produced by exactly SEAL's sequence of key switches applied to exactly the same
// intermediate ciphertexts, so the bits are unchanged (cfg3: 18,204 -> 5,460 key switches).
struct RotTrie {
    struct Node {
        u32 elt = 0;
        std::vector<int> children;
        std::vector<std::size_t> terminals;  // rotation amounts ending at this node
    };
    std::vector<Node> nodes{Node{}};
    int depth = 0;
    void insert(const std::vector<u32> &seq, std::size_t tag)
    {
        int cur = 0;
        for (u32 e : seq) {
            int nxt = -1;
            for (int c : nodes[cur].children)
                if (nodes[c].elt == e) { nxt = c; break; }
            if (nxt < 0) {
                nodes.push_back(Node{e, {}, {}});
                nxt = (int)nodes.size() - 1;
                nodes[cur].children.push_back(nxt);
            }
            cur = nxt;
        }
        nodes[cur].terminals.push_back(tag);
        depth = std::max(depth, (int)seq.size());
    }
    std::size_t key_switches() const { return nodes.size() - 1; }
};

// Rotation buffers of the trie walk: nb per depth, taken round robin by consecutive children at a
// depth, so the buffer of a visited terminal stays intact for nb - 1 more siblings (deferred tensors).
struct TrieBufs {
    std::vector<std::vector<u64 *>> b;  // [depth][slot]
    std::vector<unsigned> next;
    TrieBufs(Scratch &s, int depth, int nb, u64 words) : b(depth + 1), next(depth + 1, 0)
    {
        for (int d = 0; d <= depth; ++d)
            for (int k = 0; k < (d == 0 ? 1 : nb); ++k) b[d].push_back(s.take(words));
    }
    // per[d] buffers at depth d: with per[d] = the trie's nodes at depth d, every node keeps its own buffer for the
    // whole walk (the baby rotations of bsgs_core stay alive until the inner kernel has read them)
    TrieBufs(Scratch &s, const std::vector<int> &per, u64 words) : b(per.size()), next(per.size(), 0)
    {
        for (std::size_t d = 0; d < per.size(); ++d)
            for (int k = 0; k < per[d]; ++k) b[d].push_back(s.take(words));
    }
    u64 *take(int d) { return b[d][next[d]++ % b[d].size()]; }
};

// Depth-first walk: visit(tag, src) for every terminal of `node`, then for each child compute the
// child's rotation into a depth + 1 buffer and recurse.  before_write(buf) runs before a buffer is
// overwritten (the caller flushes deferred work that still reads it).  A buffer is only rewritten
// after the subtree that read it has been enqueued (stream order makes that safe).
template <class F, class W>
void walk_trie(Ctx &c, Scratch &s, const RotTrie &t, int node, PolyArr src, int depth, int B, int l,
               const hec_galois_keys &gk, TrieBufs &bufs, u64 stride, F &visit, W &before_write)
{
    for (std::size_t tag : t.nodes[node].terminals) visit(tag, src);
    for (int ch : t.nodes[node].children) {
        const u32 e = t.nodes[ch].elt;
        const PolyArr dst{bufs.take(depth + 1), stride, (u64)l * c.N};
        before_write(dst.p);
        galois_ks(c, s, src, dst, B, l, e, gk.keys.at(e));
        walk_trie(c, s, t, ch, dst, depth + 1, B, l, gk, bufs, stride, visit, before_write);
    }
}

// The same walk with the hoisted mod-up (hec_kernels.hip): a node with at least min_children children
// computes INTT(c1) and the NTT-form digits of every (target prime, digit) once into hs[depth]; each
// child then only runs the hoisted key MAC and the mod-down.  Nodes with fewer children use the fused
// per-rotation key switch.
template <class F, class W>
void walk_trie_hoisted(Ctx &c, Scratch &s, const RotTrie &t, int node, PolyArr src, int depth, int B, int l,
                       hec_context *ctx, hec_galois_keys &gk, TrieBufs &bufs, const std::vector<Hoist> &hs,
                       u64 stride, int min_children, F &visit, W &before_write)
{
    for (std::size_t tag : t.nodes[node].terminals) visit(tag, src);
    const auto &ch = t.nodes[node].children;
    if ((int)ch.size() < min_children) {
        for (int cn : ch) {
            const u32 e = t.nodes[cn].elt;
            const PolyArr dst{bufs.take(depth + 1), stride, (u64)l * c.N};
            before_write(dst.p);
            galois_ks(c, s, src, dst, B, l, e, gk.keys.at(e));
            walk_trie_hoisted(c, s, t, cn, dst, depth + 1, B, l, ctx, gk, bufs, hs, stride, min_children, visit,
                              before_write);
        }
        return;
    }
    const Hoist &h = hs[depth];
    hoist_node(c, src, B, l, h);
    if (c.debug_lanes) debug_count_zl(c, h.zl, c.zflag + 1);
    const u64 N = c.N;
    // children in groups of up to `sup` siblings: one sibling-fused k_hmacm launch per hoisted_group() of them (the
    // default hmac_cfg 2: the whole group, slots of 2; 1: per pair), accumulators h.acc(q), contiguous; then the
    // mod-downs in groups of HOIST_GROUP share their small launches
    const std::size_t grp = (std::size_t)hoisted_group(c);
    const std::size_t sup = std::max<std::size_t>(grp, HOIST_GROUP / grp * grp);
    // the sibling-fused MAC folds the node's c0 into the children's accumulators (X0 P mod q_I), so their
    // mod-downs take no IN term; the one-child MAC (hmac_cfg 0) does not
    const bool fold = c.hmac_cfg != 0;
    const PolyArr X0 = fold ? PolyArr{src.p, src.sb, src.sk} : PolyArr{};
    const int in_nk = fold ? 0 : 1;
    for (std::size_t g0 = 0; g0 < ch.size(); g0 += sup) {
        const int ng = (int)std::min<std::size_t>(sup, ch.size() - g0);
        HChildSpec kids[HOIST_GROUP];
        for (int q = 0; q < ng; ++q) {
            const u32 e = t.nodes[ch[g0 + q]].elt;
            kids[q] = HChildSpec{e, (u32)invm(e, 2 * N), gk.keys.at(e), galois_negw(ctx, gk, e), h.acc(q),
                                 galois_kw(ctx, gk, e, l), fold ? galois_mkey(ctx, gk, e) : nullptr};
        }
        const double K = l + 1;  // per child: key (2 l K), W (K), KW (2 K), ACC (2 B K)
        // hmac_divround: the group launch (hmac_cfg 2, so ng <= HOIST_GROUP is one launch and the node's c0 is folded:
        // no IN term) in the order of the per-rotation mac_divround: the special-prime target of every child, its INTT
        // and the fan-out over the group, then the data targets' launch divides-and-rounds its accumulators into the
        // children's rotation buffers.  Short of rotation buffers for the group: the unfolded path below
        if (c.hmac_divround && c.hmac_cfg == 2 && c.hmac_int && c.fan_out && !(c.moddown1 && c.logN == 15) &&
            (int)bufs.b[depth + 1].size() >= ng) {
            const PolyArr X1{src.p + src.sk, src.sb, 0};
            PolyArr dst[HOIST_GROUP];
            HChildSpec outs[HOIST_GROUP];
            for (int q = 0; q < ng; ++q) {  // taken before the data launch writes them
                dst[q] = PolyArr{bufs.take(depth + 1), stride, (u64)l * N};
                before_write(dst[q].p);
                outs[q] = kids[q];
                outs[q].ACC = dst[q].p;
            }
            const std::size_t top = s.top;
            const u64 sz = (u64)B * 2 * l * N;
            u64 *Z = s.take((u64)ng * sz);
            {  // digits E[b][P] (B l) + per child key (2 l), W, KW (3) -> ACC's P limbs (2 B)
                ProfScope ps(c, "ks_hmac");
                ProfScope k(c, "k:k_hmacm/p", (double)B * l + ng * (2.0 * l + 3.0 + 2.0 * B));
                hoisted_mac_group(c, X1, X0, h.E, h.zl, kids, ng, B, l, 1);
            }
            {
                ProfScope ps(c, "ks_moddown");
                const int pP[1] = {(int)c.K - 1};
                {
                    ProfScope k(c, "k:k_ntt/moddown_intt", 4.0 * B * ng);
                    ntt_strided(c, true, h.acc(0) + l * N, (l + 1) * N, h.acc(0) + l * N, (l + 1) * N, 1, pP, 2 * B * ng, 1,
                                1);
                }
                ProfScope k(c, "k:k_fan2/moddown", 2.0 * B * ng * (l + 1));
                fan_divide_round(c, h.acc(0) + l * N, 2 * (l + 1) * N, (l + 1) * N, Z, B * ng, 2, l, (int)c.K - 1);
            }
            {  // digits E (B l (l - 1)) + c1, c0 (2 B l) + per child key (2 l l), W, KW (3 l), Z (2 B l) -> OUT (2 B l)
                ProfScope ps(c, "ks_hmac");
                ProfScope k(c, "k:k_hmacm/divround",
                            (double)B * (l * l + 2 * l) - (double)B * l + ng * (2.0 * l * l + 3.0 * l + 4.0 * B * l));
                HmacDR dr{};
                dr.Z = Z; dr.zs = sz; dr.osb = stride; dr.osk = (u64)l * N; dr.twb = c.twb; dr.twbf = c.twbf;
                for (int i = 0; i < l; ++i) { dr.inv[i] = c.p_inv[i]; dr.inv_q[i] = c.p_inv_q[i]; }
                hoisted_mac_group(c, X1, X0, h.E, h.zl, outs, ng, B, l, 2, &dr);
            }
            s.top = top;
            for (int q = 0; q < ng; ++q)
                walk_trie_hoisted(c, s, t, ch[g0 + q], dst[q], depth + 1, B, l, ctx, gk, bufs, hs, stride, min_children,
                                  visit, before_write);
            continue;
        }
        for (int q0 = 0, nk = 0; q0 < ng; q0 += nk) {  // one profile scope per launch (bench.py's roofline)
            nk = std::min((int)grp, ng - q0);
            // an odd group's last three children as one 3-child launch (the digits read once, not twice)
            if (c.hmac_odd3 && grp == 2 && ng - q0 == 3) nk = 3;
            ProfScope ps(c, "ks_hmac");  // digits E (B l^2) + c1 (B l) [+ c0 (B l), folded] + per child
            ProfScope k(c, "k:k_hmacm",
                        (double)B * (l * l + l + (fold ? l : 0)) + nk * (2.0 * l * K + 3.0 * K + 2.0 * B * K));
            if (c.hmac_cfg == 2)
                hoisted_mac_group(c, PolyArr{src.p + src.sk, src.sb, 0}, X0, h.E, h.zl, kids + q0, nk, B, l);
            else if (nk == 3 && grp == 2)
                hoisted_mac_3(c, PolyArr{src.p + src.sk, src.sb, 0}, X0, h.E, h.zl, kids + q0, B, l);
            else hoisted_mac_multi(c, PolyArr{src.p + src.sk, src.sb, 0}, X0, h.E, h.zl, kids + q0, nk, B, l);
        }
        for (int m0 = 0; m0 < ng; m0 += HOIST_GROUP) {  // mod-downs in groups, then each child's subtree
            const int nm = std::min(HOIST_GROUP, ng - m0);
            if ((int)bufs.b[depth + 1].size() < nm) {  // too few rotation buffers to hold the group at once
                for (int q = m0; q < m0 + nm; ++q) {
                    const PolyArr dst{bufs.take(depth + 1), stride, (u64)l * N};
                    before_write(dst.p);
                    const std::size_t top = s.top;
                    u64 *Z = s.take((u64)B * 2 * l * N);
                    moddown(c, h.acc(q), Z, PolyArr{src.p, src.sb, src.sk}, in_nk, dst, B, l, kids[q].elt);
                    s.top = top;
                    walk_trie_hoisted(c, s, t, ch[g0 + q], dst, depth + 1, B, l, ctx, gk, bufs, hs, stride,
                                      min_children, visit, before_write);
                }
                continue;
            }
            PolyArr dst[HOIST_GROUP];
            u32 elts[HOIST_GROUP];
            for (int q = 0; q < nm; ++q) {
                dst[q] = PolyArr{bufs.take(depth + 1), stride, (u64)l * N};
                before_write(dst[q].p);
                elts[q] = kids[m0 + q].elt;
            }
            {
                const std::size_t top = s.top;
                u64 *Z = s.take((u64)nm * B * 2 * l * N);
                moddown_group(c, h.acc(m0), Z, PolyArr{src.p, src.sb, src.sk}, in_nk, dst, elts, nm, B, l);
                s.top = top;
            }
            for (int q = 0; q < nm; ++q)
                walk_trie_hoisted(c, s, t, ch[g0 + m0 + q], dst[q], depth + 1, B, l, ctx, gk, bufs, hs, stride,
                                  min_children, visit, before_write);
        }
    }
}

// The argument checks SEAL runs along the reference loop (rotate_internal, multiply[_plain]_inplace's
// scale bound, add_inplace's are_close, relinearize / rescale at the end of the chain), in its order, on
// the host.  Returns the product scale of every output.  matvec_lanes runs it on the calling thread over
// the whole batch before any lane starts, so a failing call writes no output (as in SEAL).
std::vector<double> matvec_check(hec_context *ctx, const hec_ciphertext *const *diags, const hec_plaintext *const *pdiags,
                                 std::size_t n, const std::vector<std::size_t> &js, const hec_ciphertext *const *cols,
                                 std::size_t p, const hec_kswitch_key *rk, const hec_galois_keys *gk, bool finish)
{
    const Ctx &c = ctx->c;
    const bool pt = pdiags != nullptr;
    need(n >= 1 && p >= 1 && !js.empty(), "empty matrix operand");
    for (std::size_t j : js) need(j < n, "diagonal index out of range");
    check_obj(ctx, gk, BAD_GK);
    if (finish && !pt) check_obj(ctx, rk, BAD_RK);
    const std::size_t l = cols[0]->level;
    for (std::size_t i = 0; i < p; ++i) check_ct(ctx, cols[i]);
    for (std::size_t i = 0; i < p; ++i) need(cols[i]->size == 2, "encrypted size must be 2");
    for (std::size_t i = 0; i < p; ++i) need(cols[i]->level == l, "encrypted1 and encrypted2 parameter mismatch");
    if (pt) {
        for (std::size_t j : js) check_plain_data(ctx, pdiags[j]);
        for (std::size_t j : js) need(pdiags[j]->level == l, "encrypted_ntt and plain_ntt parameter mismatch");
    } else {
        for (std::size_t j : js) check_ct(ctx, diags[j]);
        for (std::size_t j : js) need(diags[j]->size == 2, "encrypted size must be 2");
        for (std::size_t j : js) need(diags[j]->level == l, "encrypted1 and encrypted2 parameter mismatch");
    }
    auto dscale = [&](std::size_t j) { return pt ? pdiags[j]->scale : diags[j]->scale; };
    // scale bookkeeping exactly as multiply[_plain]_inplace (bound) + add_inplace (are_close) would see it
    std::vector<double> ps(p);
    for (std::size_t i = 0; i < p; ++i) {
        for (std::size_t k = 0; k < js.size(); ++k) {
            const double sc = cols[i]->scale * dscale(js[k]);
            need(scale_ok(c, sc, l), "scale out of bounds");
            if (k == 0) ps[i] = sc;
            else need(are_close(ps[i], sc), "scale mismatch");
        }
    }
    if (finish && l < 2) throw std::invalid_argument("end of modulus switching chain reached");
    std::vector<u32> seq;  // rotate_internal's own errors ("step count too large", "Galois key not present")
    for (std::size_t j : js) {
        seq.clear();
        rotation_elts(c, (int)j, *gk, seq);
    }
    return ps;
}

// BatchedMatrix::matmul diag x col (he_linalg.cpp:943-1006) for the p columns at once, diagonals
// [jb, je).  The loop over i (output column) is interchanged with the loop over j so that one
// rotation launch sequence and one key read serve all p columns, and the rotations run over the
// prefix trie; every out[i] still sums the same terms (modular addition is exact and order free),
// so the bits equal the reference loop's.
// diags (ciphertexts) or pdiags (plaintexts, the ct x pt form: multiply_plain, products stay size 2,
// no relinearization) — exactly one is non-null.
void matvec_core(hec_context *ctx, const hec_ciphertext *const *diags, const hec_plaintext *const *pdiags,
                 std::size_t n, const std::vector<std::size_t> &js, const hec_ciphertext *const *cols, std::size_t p,
                 const hec_kswitch_key *rk, const hec_galois_keys *gk, bool finish, hec_ciphertext *const *out,
                 Ctx *exec = nullptr)  // exec: the lane context that runs it (objects still belong to ctx)
{
    Ctx &c = exec ? *exec : ctx->c;
    const bool pt = pdiags != nullptr;
    const std::vector<double> ps = matvec_check(ctx, diags, pdiags, n, js, cols, p, rk, gk, finish);
    const std::size_t l = cols[0]->level, N = c.N;
    auto ddata = [&](std::size_t j) -> const u64 * { return pt ? pdiags[j]->d : diags[j]->d; };
    RotTrie trie;
    {
        std::vector<u32> seq;
        for (std::size_t j : js) {
            seq.clear();
            rotation_elts(c, (int)j, *gk, seq);
            trie.insert(seq, j);
        }
    }
    const u64 S2 = 2 * l * N, S3 = 3 * l * N;
    const int D = trie.depth;
    const int nb = c.tensor_defer_bufs;  // rotation buffers per depth
    const bool hoist = c.hoist && D > 0;
    std::size_t words = p * (S2 * (1 + (std::size_t)D * nb) + S3) + 2 * p * l * N + ks_words(c, p, l) +
                        (D * nb + 80) * 64;
    if (hoist) {
        words += (std::size_t)D * hoist_words(c, p, l);
        words += hoisted_child_words(c, p, l);
    }
    if (finish) words += rescale_words(c, p, 2, l) + p * 2 * (l - 1) * N;
    Scratch s(c, words);
    TrieBufs bufs(s, D, nb, p * S2);
    u64 *ACC3 = s.take(p * S3);
    for (std::size_t i = 0; i < p; ++i) d2d(c, bufs.b[0][0] + i * S2, cols[i]->d, S2);
    const PolyArr Xa{bufs.b[0][0], S2, l * N}, Aa{ACC3, S3, l * N};
    bool first = true;
    // the products of up to TB_MAX visited terminals (ct x ct tensors, or ct x pt plain products) are
    // deferred and applied in one k_tensor_multi pass (the accumulator read/written once per batch); a
    // batch is flushed when full or before one of its rotation buffers is overwritten
    TensorBatch tb{};
    auto flush = [&] {
        if (tb.T == 0) return;
        ProfScope pr(c, "tensor");
        // T rotated inputs (2 B l each) + T diagonals (2 l, or l plaintext) + ACC read (unless first) + write
        const double accl = (pt ? 2.0 : 3.0) * p * l;
        ProfScope k(c, "k:k_tensor_multi2", tb.T * (2.0 * p * l + (pt ? 1.0 : 2.0) * l) + (first ? 1 : 2) * accl);
        tensor_multi(c, tb, S2, l * N, l * N, Aa, (int)p, (int)l, first, pt);
        first = false;
        tb.T = 0;
    };
    auto visit = [&](std::size_t j, PolyArr src) {
        tb.r[tb.T] = src.p;
        tb.a[tb.T] = ddata(j);
        if (++tb.T == std::min(TB_MAX, c.tensor_defer_max)) flush();
    };
    auto before_write = [&](const u64 *buf) {
        for (int t = 0; t < tb.T; ++t)
            if (tb.r[t] == buf) return flush();
    };
    if (hoist) {
        hec_galois_keys &gkm = const_cast<hec_galois_keys &>(*gk);  // negw is a per-key cache
        for (std::size_t nd = 1; nd < trie.nodes.size(); ++nd) {
            galois_negw(ctx, gkm, trie.nodes[nd].elt);
            galois_kw(ctx, gkm, trie.nodes[nd].elt, (int)l);
            if (c.hmac_cfg != 0) galois_mkey(ctx, gkm, trie.nodes[nd].elt);
        }
        std::vector<Hoist> hs(D);
        for (int d = 0; d < D; ++d) hs[d] = hoist_alloc(c, s, (int)p, (int)l);
        dev_zero(c, c.zflag, 2 * sizeof(int));
        walk_trie_hoisted(c, s, trie, 0, Xa, 0, (int)p, (int)l, ctx, gkm, bufs, hs, S2, c.hoist_min_children, visit,
                          before_write);
    } else {
        walk_trie(c, s, trie, 0, Xa, 0, (int)p, (int)l, *gk, bufs, S2, visit, before_write);
    }
    flush();
    if (hoist) {  // a digit limb with more zero coefficients than the hoisted MAC corrects: recompute
        int zfl[2] = {0, 0};
        HEC_HIP(hipMemcpyAsync(zfl, c.zflag, 2 * sizeof(int), hipMemcpyDeviceToHost, c.stream));
        HEC_HIP(hipStreamSynchronize(c.stream));
        const int zf = zfl[0];
        if (c.debug_lanes)
            std::fprintf(stderr, "hec-debug: %s p=%zu zero-list nodes %d overflow %d\n", exec ? "lane" : "ctx", p, zfl[1],
                         zfl[0]);
        if (zf) {
            if (std::getenv("HEC_DEBUG")) std::fprintf(stderr, "hec: zero-list overflow, matvec recomputed without hoisting (p=%zu)\n", p);
            c.hoist = false;
            try {
                matvec_core(ctx, diags, pdiags, n, js, cols, p, rk, gk, finish, out, exec);
            } catch (...) {
                c.hoist = true;
                throw;
            }
            c.hoist = true;
            return;
        }
    }
    if (!finish) {  // the accumulators as they are: size 3 for ct x ct, size 2 for ct x pt
        for (std::size_t i = 0; i < p; ++i) store_ct(c, out[i], ACC3 + i * S3, pt ? 2 : 3, l, ps[i]);
        return;
    }
    const u64 So = 2 * (l - 1) * N;
    u64 *O = s.take(p * So);
    const PolyArr Oa{O, So, (l - 1) * N};
    // relinearize (SMART_RELIN == 1: once per output, he_linalg.cpp:1000) and rescale (:1001); ct x pt products are
    // size 2 and only rescale
    if (pt) rescale_batch(c, s, Aa, (int)p, 2, (int)l, Oa);
    else relin_rescale(c, s, ACC3, rk->d, (int)p, (int)l, Oa, "relin");
    const double ql = (double)c.q[l - 1];
    for (std::size_t i = 0; i < p; ++i) store_ct(c, out[i], O + i * So, 2, l - 1, ps[i] / ql);
}

// ---------------------------------------------------------------- baby-step giant-step matvec, ct x pt and ct x ct
// The same product over another schedule (opt-in, not the bits of matvec_core unless bs_eff = n).  The
// ct x pt form (the ct x ct form's own steps are at bsgs_core):
//   inner_g = sum_{i < bs, g bs + i < n} multiply_plain(rotate_vector(x, i), P'[g bs + i])
//   out     = rescale_to_next(inner_0 + sum_{1 <= g < G} rotate_vector(inner_g, g bs))
// with the plaintext diagonals in BSGS form (P'[j] encodes diagonal j rotated right by (j / bs) bs slots), so
// (bs - 1) + (G - 1) rotations stand for the n - 1 of the reference loop.  Every operation is the per-operation
// call's (rotate_vector as rotation_elts() flattens it, multiply_plain's reduced products, exact modular sums), so
// the words equal that composition's.
struct BsgsPlan {
    std::size_t bs = 0, G = 0;  // bs_eff and the giant groups
    std::vector<int> steps;     // the rotation steps in the order the call issues them: babies, then giants
};
BsgsPlan bsgs_plan(uint64_t n, uint64_t bs)
{
    need(n >= 1, "empty matrix operand");
    need(n < (1ull << 30), "step count too large");  // the steps are ints
    if (bs == 0)
        for (bs = 1; bs * bs < n;) bs <<= 1;  // the smallest power of two >= sqrt(n)
    BsgsPlan p;
    p.bs = (std::size_t)std::min<uint64_t>(bs, n);
    need(p.bs <= 1024, "bs must be at most 1024");  // k_bsgs_inner's exact FP64 sums (hec_kernels.hip)
    p.G = (n + p.bs - 1) / p.bs;
    for (std::size_t i = 1; i < p.bs; ++i) p.steps.push_back((int)i);
    for (std::size_t g = 1; g < p.G; ++g) p.steps.push_back((int)(g * p.bs));
    return p;
}

// matvec_check's checks in its order over the BSGS schedule's operations, all before anything is written; returns the
// product scale of every output.  diags or pdiags, as matvec_check.  The aliasing rule (out[i] may be
// cols[i]; no diagonal may be an output) keeps each form's place: before the scale checks for ct x pt, last for ct x ct
std::vector<double> bsgs_check(hec_context *ctx, const hec_ciphertext *const *diags, const hec_plaintext *const *pdiags,
                               std::size_t n, const BsgsPlan &plan, const hec_ciphertext *const *cols, std::size_t p,
                               const hec_kswitch_key *rk, const hec_galois_keys *gk, hec_ciphertext *const *out)
{
    const Ctx &c = ctx->c;
    const bool pt = pdiags != nullptr;
    need(p >= 1, "empty matrix operand");
    check_obj(ctx, gk, BAD_GK);
    for (std::size_t i = 0; i < p; ++i) check_ct(ctx, cols[i]);
    const std::size_t l = cols[0]->level;
    for (std::size_t i = 0; i < p; ++i) need(cols[i]->size == 2, "encrypted size must be 2");
    for (std::size_t i = 0; i < p; ++i) need(cols[i]->level == l, "encrypted1 and encrypted2 parameter mismatch");
    if (pt) {
        for (std::size_t j = 0; j < n; ++j) check_plain_data(ctx, pdiags[j]);
        for (std::size_t j = 0; j < n; ++j)
            need(pdiags[j]->level == l, "encrypted_ntt and plain_ntt parameter mismatch");
        check_out_alias({cols}, out, p, ctx);
    } else {
        for (std::size_t j = 0; j < n; ++j) check_ct(ctx, diags[j]);
        for (std::size_t j = 0; j < n; ++j) need(diags[j]->size == 2, "encrypted size must be 2");
        for (std::size_t j = 0; j < n; ++j) need(diags[j]->level == l, "encrypted1 and encrypted2 parameter mismatch");
    }
    std::vector<double> ps(p);
    for (std::size_t i = 0; i < p; ++i)
        for (std::size_t j = 0; j < n; ++j) {
            const double sc = cols[i]->scale * (pt ? pdiags[j]->scale : diags[j]->scale);
            need(scale_ok(c, sc, l), "scale out of bounds");
            if (j == 0) ps[i] = sc;
            else need(are_close(ps[i], sc), "scale mismatch");
        }
    if (l < 2) throw std::invalid_argument("end of modulus switching chain reached");
    if (!pt) check_obj(ctx, rk, BAD_RK);
    std::vector<u32> seq;  // rotate_internal's own errors over every planned step
    for (int st : plan.steps) {
        seq.clear();
        rotation_elts(c, st, *gk, seq);
    }
    if (!pt) check_out_alias({cols}, out, p, ctx, diags, n);
    return ps;
}

// The rotations of a BSGS call, shared by the matvec's two forms and the col x col^T product: the trie of
// rotate(x, steps[t]) (terminal tag t; step 0 is x itself), every node with a buffer of its own (per[d] nodes at depth
// d), and the key switches of the rotations by g bs, 1 <= g < G, that run after the inner sums
struct BsgsRots {
    RotTrie trie;
    std::vector<std::vector<u32>> gelts;
    std::vector<int> per;
    int D = 0;
    bool hoist = false;
};
BsgsRots bsgs_rots(const Ctx &c, const std::vector<int> &steps, std::size_t bs, std::size_t G, const hec_galois_keys &gk)
{
    BsgsRots r;
    r.gelts.resize(G);
    std::vector<u32> seq;
    for (std::size_t t = 0; t < steps.size(); ++t) {
        seq.clear();
        rotation_elts(c, steps[t], gk, seq);
        r.trie.insert(seq, t);
    }
    for (std::size_t g = 1; g < G; ++g) rotation_elts(c, (int)(g * bs), gk, r.gelts[g]);
    r.D = r.trie.depth;
    std::vector<int> depth_of(r.trie.nodes.size(), 0);
    r.per.assign((std::size_t)r.D + 1, 0);
    r.per[0] = 1;
    for (std::size_t nd = 0; nd < r.trie.nodes.size(); ++nd)  // a child's index follows its parent's
        for (int ch : r.trie.nodes[nd].children) ++r.per[(std::size_t)(depth_of[(std::size_t)ch] = depth_of[nd] + 1)];
    r.hoist = c.hoist && r.D > 0;
    return r;
}

// input vectors per pass: the y-blocks of the key switch's mod-up launch ((l + 1) l per vector), option
// "bsgs_chunk", and a workspace (words_for(Bc) words) that fits the free device memory
template <class W>
std::size_t bsgs_pass_size(const Ctx &c, std::size_t p, std::size_t l, W words_for)
{
    std::size_t Bc = std::min<std::size_t>({p, 256, std::max<std::size_t>(1, 65535 / ((l + 1) * l))});
    if (c.bsgs_chunk > 0) Bc = std::min<std::size_t>(Bc, (std::size_t)c.bsgs_chunk);
    if (words_for(Bc) > c.ws.words) {
        std::size_t fr = 0, tot = 0;
        HEC_HIP(hipMemGetInfo(&fr, &tot));
        while (Bc > 1 && words_for(Bc) > c.ws.words && (double)words_for(Bc) * 8.0 > 0.9 * (double)fr) Bc = (Bc + 1) / 2;
    }
    return Bc;
}

// the per-key tables of the hoisted baby walk (lazily built caches of gk)
void bsgs_key_tables(hec_context *ctx, const BsgsRots &r, hec_galois_keys &gkm, std::size_t l)
{
    if (!r.hoist) return;
    for (std::size_t nd = 1; nd < r.trie.nodes.size(); ++nd) {
        galois_negw(ctx, gkm, r.trie.nodes[nd].elt);
        galois_kw(ctx, gkm, r.trie.nodes[nd].elt, (int)l);
        if (ctx->c.hmac_cfg != 0) galois_mkey(ctx, gkm, r.trie.nodes[nd].elt);
    }
}

// One pass's baby phase: cols[b0 .. b0 + cnt) into the root's buffer, the trie walked (hoisted; again without hoisting
// when a digit limb has more zero coefficients than the hoisted MAC corrects), rotation i's buffer in hr[i] and the
// table uploaded to tabR.  Returns with the stream synchronised: the pointer table has left the host vector.
void bsgs_babies(hec_context *ctx, Scratch &s, const BsgsRots &r, hec_galois_keys &gkm, TrieBufs &bufs,
                 const std::vector<Hoist> &hs, const hec_ciphertext *const *cols, std::size_t cnt, std::size_t l,
                 std::vector<const u64 *> &hr, const u64 **tabR)
{
    Ctx &c = ctx->c;
    const u64 S2 = 2 * l * c.N;
    for (std::size_t i = 0; i < cnt; ++i) d2d(c, bufs.b[0][0] + i * S2, cols[i]->d, S2);
    const PolyArr Xa{bufs.b[0][0], S2, l * c.N};
    auto visit = [&](std::size_t i, PolyArr src) { hr[i] = src.p; };
    auto keep = [](const u64 *) {};  // no buffer is written twice in a walk
    auto babies = [&](bool hoisted) {
        std::fill(bufs.next.begin(), bufs.next.end(), 0u);
        if (hoisted) {
            dev_zero(c, c.zflag, 2 * sizeof(int));
            walk_trie_hoisted(c, s, r.trie, 0, Xa, 0, (int)cnt, (int)l, ctx, gkm, bufs, hs, S2, c.hoist_min_children,
                              visit, keep);
        } else {
            walk_trie(c, s, r.trie, 0, Xa, 0, (int)cnt, (int)l, gkm, bufs, S2, visit, keep);
        }
        HEC_HIP(hipMemcpyAsync(tabR, hr.data(), hr.size() * sizeof(u64 *), hipMemcpyHostToDevice, c.stream));
    };
    babies(r.hoist);
    int zfl[2] = {0, 0};
    if (r.hoist) HEC_HIP(hipMemcpyAsync(zfl, c.zflag, 2 * sizeof(int), hipMemcpyDeviceToHost, c.stream));
    HEC_HIP(hipStreamSynchronize(c.stream));  // the flag is read; the pointer table has left the host vector
    if (zfl[0]) {
        if (std::getenv("HEC_DEBUG"))
            std::fprintf(stderr, "hec: zero-list overflow, baby rotations recomputed without hoisting (p=%zu)\n", cnt);
        babies(false);
        HEC_HIP(hipStreamSynchronize(c.stream));
    }
}

// The ct x ct form of the schedule multiplies by ciphertext diagonals, so its inner sums have size 3:
//   inner_g = sum_{i < bs, g bs + i < n} multiply(rotate_vector(x, i), A'[g bs + i])         (size 3)
//   r_g     = relinearize(inner_g)
//   out     = rescale_to_next(r_0 + sum_{1 <= g < G} rotate_vector(r_g, g bs))
// with the ciphertext diagonals in BSGS form (A'[j] encrypts diagonal j rotated right by (j / bs) bs slots): the
// rotations act on size-2 ciphertexts, so every giant group is relinearised before its rotation, (bs - 1) + G +
// (G - 1) key switches for the n - 1 NAF chains and one relinearisation of the reference loop.
//
// One core for both forms: diags (ct x ct, with rk) or pdiags (ct x pt, rk unused), exactly one non-null, as
// matvec_core.  The forms differ in the inner-sum kernel and its slot stride (size 3 or 2), in the relinearisation
// between the inner and the giant phase, and in where inner_0 lands (ct x pt: straight into the accumulator)
void bsgs_core(hec_context *ctx, const hec_ciphertext *const *diags, const hec_plaintext *const *pdiags, std::size_t n,
               const BsgsPlan &plan, const hec_ciphertext *const *cols, std::size_t p, const hec_kswitch_key *rk,
               const hec_galois_keys *gk, hec_ciphertext *const *out)
{
    Ctx &c = ctx->c;
    const bool pt = pdiags != nullptr;
    if (!pt) need(plan.bs <= 512, "bs must be at most 512");  // k_bsgs_inner_ct's exact FP64 sums (hec_kernels.hip)
    const std::vector<double> ps = bsgs_check(ctx, diags, pdiags, n, plan, cols, p, rk, gk, out);
    const std::size_t l = cols[0]->level, N = c.N, bs = plan.bs, G = plan.G;
    const std::size_t GG = (std::size_t)bsgs_tile(c, !pt);
    std::vector<int> babies(bs);
    std::iota(babies.begin(), babies.end(), 0);
    const BsgsRots rots = bsgs_rots(c, babies, bs, G, *gk);
    const int D = rots.D;
    const std::size_t nbuf = rots.trie.nodes.size();
    const u64 S2 = 2 * l * N, S3 = 3 * l * N, So = 2 * (l - 1) * N;
    const u64 Sin = pt ? S2 : S3;  // an inner sum's stride
    // ct x ct: a tile's relinearisations run as one key switch over its ng Bc slots while the NTT launches' y-blocks
    // allow
    const std::size_t ymax = std::max<std::size_t>(1, 65535 / ((l + 1) * l));
    auto merged = [&](std::size_t Bc) { return !pt && GG * Bc <= ymax; };  // by the pass size: the workspace covers it
    auto words_for = [&](std::size_t Bc) {
        const std::size_t Bks = merged(Bc) ? GG * Bc : Bc;
        std::size_t w = Bc * (S2 * (nbuf + 2) + Sin * GG + So) + 2 * Bc * l * N + ks_words(c, Bks, l) +
                        rescale_words(c, Bc, 2, l) + bs + n + (nbuf + GG + 100) * 64;
        if (rots.hoist) w += (std::size_t)D * hoist_words(c, Bc, l) + hoisted_child_words(c, Bc, l);
        return w;
    };
    const std::size_t Bc = bsgs_pass_size(c, p, l, words_for);
    Scratch s(c, words_for(Bc));
    std::vector<const u64 *> hp(n), hr(bs);
    for (std::size_t j = 0; j < n; ++j) hp[j] = pt ? pdiags[j]->d : diags[j]->d;
    const u64 **tabP = reinterpret_cast<const u64 **>(s.take(n));
    const u64 **tabR = reinterpret_cast<const u64 **>(s.take(bs));
    HEC_HIP(hipMemcpyAsync(tabP, hp.data(), n * sizeof(u64 *), hipMemcpyHostToDevice, c.stream));
    hec_galois_keys &gkm = const_cast<hec_galois_keys &>(*gk);  // the lazily built per-key tables are caches
    bsgs_key_tables(ctx, rots, gkm, l);
    const std::size_t mark = s.top;
    const double ql = (double)c.q[l - 1];
    for (std::size_t b0 = 0; b0 < p; b0 += Bc) {
        const std::size_t cnt = std::min(Bc, p - b0);
        s.top = mark;  // every carve of a pass is sized by its own count (the hoisted accumulators are contiguous)
        TrieBufs bufs(s, rots.per, cnt * S2);
        u64 *A[2] = {s.take(cnt * S2), s.take(cnt * S2)};
        u64 *T = s.take(GG * cnt * Sin);  // the tile's inner sums, contiguous: slot t at T + t cnt Sin
        auto slot = [&](std::size_t t) { return T + t * cnt * Sin; };
        u64 *O = s.take(cnt * So);
        std::vector<Hoist> hs((std::size_t)D);
        if (rots.hoist)
            for (int d = 0; d < D; ++d) hs[(std::size_t)d] = hoist_alloc(c, s, (int)cnt, (int)l);
        bsgs_babies(ctx, s, rots, gkm, bufs, hs, cols + b0, cnt, l, hr, tabR);
        // inner and giant phases over tiles of GG giants: only one tile of inner sums is live; inner_0 (ct x ct: r_0)
        // starts the accumulator, every other one is rotated by g bs with the accumulator added in the key switch's
        // last stage
        int cur = 0;
        for (std::size_t g0 = 0; g0 < G; g0 += GG) {
            const std::size_t ng = std::min(GG, G - g0);
            BsgsInner a{};
            a.R = tabR; a.P = tabP; a.n = n; a.bs = (int)bs; a.g0 = (int)g0; a.ng = (int)ng;
            for (std::size_t t = 0; t < ng; ++t) a.out[t] = pt && g0 + t == 0 ? A[cur] : slot(t);
            {
                ProfScope pr(c, pt ? "bsgs_inner" : "bsgs_inner_ct");
                // the babies once per launch (2 B l each), the tile's diagonals once (l each as plaintexts, 2 l as
                // ciphertexts), the outputs once
                const double nd = (double)(std::min(n, (g0 + ng) * bs) - g0 * bs);
                ProfScope k(c, pt ? "k:k_bsgs_inner" : "k:k_bsgs_inner_ct",
                            pt ? 2.0 * cnt * l * (double)(bs + ng) + nd * l
                               : cnt * l * (2.0 * bs + 3.0 * ng) + 2.0 * nd * l);
                bsgs_inner(c, a, !pt, S2, l * N, l * N, Sin, l * N, (int)cnt, (int)l);
            }
            if (!pt) {  // r_g = relinearize(inner_g), in place in the slot's first two polys; r_0 into the accumulator
                ProfScope pr(c, "bsgs_relin");
                auto relin = [&](std::size_t t, std::size_t cntk, PolyArr OUT) {
                    keyswitch(c, s, PolyArr{slot(t) + 2 * l * N, S3, 0}, rk->d, PolyArr{slot(t), S3, l * N}, 2, OUT,
                              (int)cntk, (int)l);
                };
                std::size_t t = 0;
                if (g0 == 0) relin(t++, cnt, PolyArr{A[cur], S2, l * N});
                if (t < ng && merged(Bc)) {
                    relin(t, (ng - t) * cnt, PolyArr{slot(t), S3, l * N});
                    t = ng;
                }
                for (; t < ng; ++t) relin(t, cnt, PolyArr{slot(t), S3, l * N});
            }
            for (std::size_t t = 0; t < ng; ++t) {
                const std::size_t g = g0 + t;
                if (g == 0) continue;
                const PolyArr X{slot(t), Sin, l * N};
                const std::vector<u32> &el = rots.gelts[g];
                for (std::size_t e = 0; e + 1 < el.size(); ++e)
                    galois_ks(c, s, X, X, (int)cnt, (int)l, el[e], gk->keys.at(el[e]));
                galois_ks(c, s, X, PolyArr{A[1 - cur], S2, l * N}, (int)cnt, (int)l, el.back(), gk->keys.at(el.back()),
                          PolyArr{A[cur], S2, l * N});
                cur = 1 - cur;
            }
        }
        rescale_batch(c, s, PolyArr{A[cur], S2, l * N}, (int)cnt, 2, (int)l, PolyArr{O, So, (l - 1) * N});
        for (std::size_t i = 0; i < cnt; ++i) store_ct(c, out[b0 + i], O + i * So, 2, l - 1, ps[b0 + i] / ql);
    }
    HEC_HIP(hipStreamSynchronize(c.stream));  // the host pointer tables go out of scope
}

// ---------------------------------------------------------------- baby-step giant-step col x col^T product
// BatchedMatrix::matmul's col x col^T branch (hec_matmul_col_colT) over the schedule above (opt-in, not
// that entry's bits unless bs_eff = p).  With output i = g bs + b:
//   Bb[j][b] = rotate_vector(B[j], b)         b < bs
//   Ag[j][g] = rotate_vector(A[j], -g bs)     g < G
//   acc_i    = sum_{j < n} multiply(Bb[j][b], Ag[j][g])                                     (size 3)
//   r_i      = rescale_to_next(relinearize(acc_i))
//   out[i]   = r_i (form HEC_DIAG_BSGS), rotate_vector(r_i, g bs) (form HEC_DIAG_NATURAL)
// r_i is diagonal i rotated right by g bs slots, hec_matmul_diag_col_bsgs's input form for the same bs.
struct CctPlan {
    std::size_t bs = 0, G = 0;
    std::vector<int> steps;  // babies, negative giants, (form 0) positive giants
};
CctPlan colcolt_plan(uint64_t p, uint64_t bs, int form)
{
    need(p >= 1, "empty matrix operand");
    need(p < (1ull << 30), "step count too large");  // the steps are ints
    need(form == HEC_DIAG_NATURAL || form == HEC_DIAG_BSGS, "form must be HEC_DIAG_NATURAL or HEC_DIAG_BSGS");
    if (bs == 0)
        for (bs = 1; bs * bs < p;) bs <<= 1;  // the smallest power of two >= sqrt(p), as bsgs_plan
    CctPlan pl;
    pl.bs = (std::size_t)std::min<uint64_t>(bs, p);
    pl.G = (p + pl.bs - 1) / pl.bs;
    for (std::size_t b = 1; b < pl.bs; ++b) pl.steps.push_back((int)b);
    for (std::size_t g = 1; g < pl.G; ++g) pl.steps.push_back(-(int)(g * pl.bs));
    if (form == HEC_DIAG_NATURAL)
        for (std::size_t g = 1; g < pl.G; ++g) pl.steps.push_back((int)(g * pl.bs));
    return pl;
}

void colcolt_bsgs(hec_context *ctx, const hec_ciphertext *const *A, std::size_t n, const hec_ciphertext *const *B,
                  std::size_t p, uint64_t bs_arg, int form, const hec_kswitch_key *rk, const hec_galois_keys *gk,
                  hec_ciphertext *const *out)
{
    Ctx &c = ctx->c;
    need(A && B && out && n >= 1 && p >= 1, "null argument");
    const CctPlan plan = colcolt_plan(p, bs_arg, form);
    check_obj(ctx, gk, BAD_GK);
    for (std::size_t j = 0; j < n; ++j) {
        check_ct(ctx, A[j]);
        check_ct(ctx, B[j]);
    }
    const std::size_t l = A[0]->level, N = c.N, bs = plan.bs, G = plan.G;
    for (std::size_t j = 0; j < n; ++j) need(A[j]->size == 2 && B[j]->size == 2, "encrypted size must be 2");
    for (std::size_t j = 0; j < n; ++j)
        need(A[j]->level == l && B[j]->level == l, "encrypted1 and encrypted2 parameter mismatch");
    double sc = 0;
    for (std::size_t j = 0; j < n; ++j) {
        const double s = B[j]->scale * A[j]->scale;
        need(scale_ok(c, s, l), "scale out of bounds");
        if (j == 0) sc = s;
        else need(are_close(sc, s), "scale mismatch");
    }
    if (l < 2) throw std::invalid_argument("end of modulus switching chain reached");
    check_obj(ctx, rk, BAD_RK);
    {
        std::vector<u32> seq;  // rotate_internal's own errors over every planned step
        for (int st : plan.steps) {
            seq.clear();
            rotation_elts(c, st, *gk, seq);
        }
    }
    check_out_alias({}, out, p, ctx, A, n);
    check_out_alias({}, out, p, ctx, B, n);

    std::vector<int> bsteps(bs), gsteps(G);
    for (std::size_t b = 0; b < bs; ++b) bsteps[b] = (int)b;
    for (std::size_t g = 0; g < G; ++g) gsteps[g] = -(int)(g * bs);
    const BsgsRots rotsB = bsgs_rots(c, bsteps, bs, form == HEC_DIAG_NATURAL ? G : 1, *gk);  // with the output giants
    const BsgsRots rotsA = bsgs_rots(c, gsteps, bs, 1, *gk);
    const std::size_t nbuf = rotsB.trie.nodes.size() + rotsA.trie.nodes.size();
    const int D = std::max(rotsB.D, rotsA.D);
    const bool hoist = rotsB.hoist || rotsA.hoist;
    const u64 S2 = 2 * l * N, S3 = 3 * l * N, So = 2 * (l - 1) * N;
    // the tail (relinearise, rescale, form 0's giant rotations) runs over the outputs in groups of at most Pc
    const std::size_t ymax = std::max<std::size_t>(1, 65535 / ((l + 1) * l));
    const std::size_t Pc = std::min<std::size_t>({p, 256, ymax});
    auto words_for = [&](std::size_t Jc) {
        const std::size_t Bks = std::max(Jc, Pc);
        std::size_t w = p * (S3 + So) + nbuf * Jc * S2 + 2 * Bks * l * N + ks_words(c, Bks, l) +
                        rescale_words(c, Pc, 2, l) + bs + G + (nbuf + 200) * 64;
        if (hoist) w += (std::size_t)D * hoist_words(c, Jc, l) + hoisted_child_words(c, Jc, l);
        return w;
    };
    // columns per pass: k_colcolt_inner's exact FP64 sums (512), the y-blocks of the key switch's mod-up launch,
    // option "cct_jchunk", and a workspace that fits the free device memory
    std::size_t Jc = std::min<std::size_t>({n, 512, ymax});
    if (c.cct_jchunk > 0) Jc = std::min<std::size_t>(Jc, (std::size_t)c.cct_jchunk);
    if (words_for(Jc) > c.ws.words) {
        std::size_t fr = 0, tot = 0;
        HEC_HIP(hipMemGetInfo(&fr, &tot));
        while (Jc > 1 && words_for(Jc) > c.ws.words && (double)words_for(Jc) * 8.0 > 0.9 * (double)fr) Jc = (Jc + 1) / 2;
    }
    Scratch s(c, words_for(Jc));
    u64 *AC = s.take(p * S3), *O = s.take(p * So);
    const u64 **tabB = reinterpret_cast<const u64 **>(s.take(bs));
    const u64 **tabA = reinterpret_cast<const u64 **>(s.take(G));
    std::vector<const u64 *> hrB(bs), hrA(G);
    hec_galois_keys &gkm = const_cast<hec_galois_keys &>(*gk);  // the lazily built per-key tables are caches
    bsgs_key_tables(ctx, rotsB, gkm, l);
    bsgs_key_tables(ctx, rotsA, gkm, l);
    const std::size_t mark = s.top;
    for (std::size_t j0 = 0; j0 < n; j0 += Jc) {
        const std::size_t cnt = std::min(Jc, n - j0);
        s.top = mark;  // every carve of a pass is sized by its own count (the hoisted accumulators are contiguous)
        TrieBufs bufsB(s, rotsB.per, cnt * S2), bufsA(s, rotsA.per, cnt * S2);
        std::vector<Hoist> hs((std::size_t)D);
        if (hoist)
            for (int d = 0; d < D; ++d) hs[(std::size_t)d] = hoist_alloc(c, s, (int)cnt, (int)l);
        bsgs_babies(ctx, s, rotsB, gkm, bufsB, hs, B + j0, cnt, l, hrB, tabB);  // every giant rotates the same source
        bsgs_babies(ctx, s, rotsA, gkm, bufsA, hs, A + j0, cnt, l, hrA, tabA);
        CctInner a{};
        a.Bb = tabB; a.Ag = tabA; a.acc = AC; a.p = p; a.bs = (int)bs; a.G = (int)G;
        u64 nbt, ngt;
        colcolt_tiles(c, a, nbt, ngt);
        ProfScope pr(c, "cct_inner");
        // every baby buffer (2 cnt l) once per giant tile, every giant buffer once per baby tile, the accumulators
        // written once and, when not assigning, read once
        ProfScope k(c, "k:k_colcolt_inner", 2.0 * cnt * l * ((double)bs * (double)ngt + (double)G * (double)nbt) +
                                                (j0 == 0 ? 1.0 : 2.0) * 3.0 * (double)p * l);
        colcolt_inner(c, a, S2, l * N, S3, l * N, (int)cnt, (int)l, j0 == 0);
    }
    s.top = mark;
    for (std::size_t i0 = 0; i0 < p; i0 += Pc) {
        const std::size_t cnt = std::min(Pc, p - i0);
        relin_rescale(c, s, AC + i0 * S3, rk->d, (int)cnt, (int)l, PolyArr{O + i0 * So, So, (l - 1) * N}, "cct_relin");
    }
    if (form == HEC_DIAG_NATURAL) {  // out[i] = rotate_vector(r_i, g bs): one batched chain per giant group
        ProfScope pr(c, "cct_giants");
        for (std::size_t g = 1; g < G; ++g) {
            const std::size_t ng = std::min(bs, p - g * bs);
            for (std::size_t i0 = 0; i0 < ng; i0 += Pc) {
                const std::size_t cnt = std::min(Pc, ng - i0);
                const PolyArr X{O + (g * bs + i0) * So, So, (l - 1) * N};
                for (u32 e : rotsB.gelts[g]) galois_ks(c, s, X, X, (int)cnt, (int)(l - 1), e, gk->keys.at(e));
            }
        }
    }
    const double so = sc / (double)c.q[l - 1];
    for (std::size_t i = 0; i < p; ++i) store_ct(c, out[i], O + i * So, 2, l - 1, so);
}


// ---------------------------------------------------------------- batch lanes
// The engine's kernels leave issue slots and bandwidth idle (they wait on memory for most of their
// cycles), so the batch of a matvec is split into up to c.lanes sub-batches of at least
// c.lane_min_batch vectors that run the same trie walk concurrently, each from its own host thread on its
// own HIP stream and workspace.  Outputs are independent per input vector, so the bits are unchanged.
hec_context *make_lane(hec_context *parent)
{
    auto *l = new hec_context();
    Ctx &c = l->c;
    c = parent->c;  // shared device tables (twiddles, primes, maps), host constants and knobs
    c.ws = Workspace{};
    c.ws.defer_free = true;  // grown from the lane's thread while the other lanes launch
    c.prof_mode = 0;
    c.prof_tab.clear();
    c.prof_pend.clear();
    c.ev_pool.clear();
    c.ev_used = 0;
    c.stream = nullptr;
    c.zflag = nullptr;
    HEC_HIP(hipStreamCreateWithFlags(&c.stream, hipStreamNonBlocking));
    c.own_stream = true;
    HEC_HIP(hipMalloc(&c.zflag, 2 * sizeof(int)));
    HEC_HIP(hipMemset(c.zflag, 0, 2 * sizeof(int)));
    HEC_HIP(hipEventCreateWithFlags(&l->lane_done, hipEventDisableTiming));
    return l;
}
void free_lane(hec_context *l)
{
    Ctx &c = l->c;
    (void)hipStreamSynchronize(c.stream);
    if (l->lane_done) (void)hipEventDestroy(l->lane_done);
    c.ws.release();
    (void)hipFree(c.zflag);
    (void)hipStreamDestroy(c.stream);
    delete l;
}

// HEC_DEBUG_LANES: a checksum of every key's sign-mask NTTs W and key sums KW at this level, compared with the first one
// seen (they are built once and must never change)
// first-seen checksums of the per-key tables, keyed by (key set, Galois element, level, table) -- not by device
// address, which a freed table hands on to another key set; a key set's entries leave with it
// (debug_key_tables_forget from hec_galois_keys_destroy)
static std::mutex g_dbg_mu;
static std::map<std::tuple<const hec_galois_keys *, u32, int, int>, u64> g_dbg_first;

static void debug_key_tables_forget(const hec_galois_keys *gk)
{
    std::lock_guard<std::mutex> lock(g_dbg_mu);
    for (auto it = g_dbg_first.begin(); it != g_dbg_first.end();)
        it = std::get<0>(it->first) == gk ? g_dbg_first.erase(it) : std::next(it);
}

void debug_key_tables(hec_context *ctx, const hec_galois_keys &gk, int l)
{
    std::lock_guard<std::mutex> lock(g_dbg_mu);
    Ctx &c = ctx->c;
    HEC_HIP(hipDeviceSynchronize());
    auto sum = [&](const u64 *d, std::size_t words) {
        std::vector<u64> h(words);
        HEC_HIP(hipMemcpy(h.data(), d, words * sizeof(u64), hipMemcpyDeviceToHost));
        u64 s = 1469598103934665603ull;
        for (u64 w : h) s = (s ^ w) * 1099511628211ull;
        return s;
    };
    int changed = 0, n = 0;
    for (const auto &kv : gk.negw) {
        const u64 sw = sum(kv.second, c.K * c.N);
        auto it = gk.kw.find({kv.first, l});
        const bool has_kw = it != gk.kw.end();
        const u64 sk = has_kw ? sum(it->second, (std::size_t)2 * (l + 1) * c.N) : 0;
        for (auto [key, v] : {std::pair{std::tuple{&gk, (u32)kv.first, 0, 0}, sw},
                              std::pair{std::tuple{&gk, (u32)kv.first, l, 1}, sk}}) {
            if (std::get<3>(key) == 1 && !has_kw) continue;
            auto f = g_dbg_first.find(key);
            if (f == g_dbg_first.end()) g_dbg_first[key] = v;
            else if (f->second != v) ++changed;
            ++n;
        }
    }
    std::fprintf(stderr, "hec-debug: key tables %d checked, %d changed\n", n, changed);
}

void matvec_lanes(hec_context *ctx, const hec_ciphertext *const *diags, const hec_plaintext *const *pdiags,
                  std::size_t n, const std::vector<std::size_t> &js, const hec_ciphertext *const *cols, std::size_t p,
                  const hec_kswitch_key *rk, const hec_galois_keys *gk, bool finish, hec_ciphertext *const *out)
{
    Ctx &c = ctx->c;
    const int nl = (int)std::min<std::size_t>((std::size_t)std::max(1, c.lanes), p / std::max(1, c.lane_min_batch));
    if (nl <= 1 || c.prof_mode != 0) {  // profiling: the single-stream schedule, one phase at a time
        // a whole batch on the context's own workspace: first return the idle lanes' workspaces (at the bench's
        // 192 vectors the lanes hold 3 x 64 vectors' worth, and the one-lane profile step needs as much again)
        if (p > (std::size_t)std::max(1, c.lane_min_batch))
            for (hec_context *l : ctx->lanes) {
                HEC_HIP(hipStreamSynchronize(l->c.stream));
                l->c.ws.release();
            }
        matvec_core(ctx, diags, pdiags, n, js, cols, p, rk, gk, finish, out);
        return;
    }
    matvec_check(ctx, diags, pdiags, n, js, cols, p, rk, gk, finish);  // whole batch, before any lane writes
    if (c.hoist) {  // the lazily built per-key tables, before the lanes only read them
        auto &gkm = const_cast<hec_galois_keys &>(*gk);
        for (auto &kv : gkm.keys) {
            galois_negw(ctx, gkm, kv.first);
            galois_kw(ctx, gkm, kv.first, (int)cols[0]->level);
            if (c.hmac_cfg != 0) galois_mkey(ctx, gkm, kv.first);
        }
    }
    // the outputs are sized here, on the calling thread, so no lane thread frees or allocates them (matvec_core's
    // grow() then finds them large enough)
    {
        const std::size_t l = cols[0]->level, N = c.N;
        const std::size_t w = finish ? 2 * (l - 1) * N : (pdiags ? 2 : 3) * l * N;
        for (std::size_t i = 0; i < p; ++i) {
            need(out[i] != nullptr, "null argument");
            grow(out[i], w);
        }
    }
    while ((int)ctx->lanes.size() < nl) ctx->lanes.push_back(make_lane(ctx));
    if (!ctx->lanes_start) HEC_HIP(hipEventCreateWithFlags(&ctx->lanes_start, hipEventDisableTiming));
    hipEvent_t start = ctx->lanes_start;
    HEC_HIP(hipEventRecord(start, c.stream));  // the inputs were produced on the context's stream
    std::vector<char> done(nl, 0);
    std::vector<std::exception_ptr> err(nl);
    std::vector<std::thread> th;
    for (int i = 0; i < nl; ++i) {
        const std::size_t b0 = p * i / nl, b1 = p * (i + 1) / nl;
        th.emplace_back([&, i, b0, b1] {
            try {
                Ctx &lc = ctx->lanes[i]->c;
                HEC_HIP(hipSetDevice(lc.device));
                HEC_HIP(hipStreamWaitEvent(lc.stream, start, 0));
                matvec_core(ctx, diags, pdiags, n, js, cols + b0, b1 - b0, rk, gk, finish, out + b0, &lc);
                HEC_HIP(hipEventRecord(ctx->lanes[i]->lane_done, lc.stream));
                if (c.lane_serial) HEC_HIP(hipStreamSynchronize(lc.stream));
                done[i] = 1;
            } catch (...) {
                err[i] = std::current_exception();
            }
        });
        if (c.lane_serial) th.back().join();
    }
    for (auto &t : th)
        if (t.joinable()) t.join();
    for (int i = 0; i < nl; ++i)  // later work on the context sees the outputs
        if (done[i]) HEC_HIP(hipStreamWaitEvent(c.stream, ctx->lanes[i]->lane_done, 0));
    for (int i = 0; i < nl; ++i)  // outgrown lane workspaces, now that no lane thread runs (waits only after a growth)
        ctx->lanes[i]->c.ws.reclaim(ctx->lanes[i]->c.stream);
    if (c.debug_lanes && c.hoist) debug_key_tables(ctx, *gk, (int)cols[0]->level);
    for (auto &e : err)
        if (e) std::rethrow_exception(e);
}

// ---------------------------------------------------------------- multi-GPU planner and RCCL
// The diagonal planner: SEAL's key-switch sequence of every rotation j < n (rotate_internal over the key
// set), the diagonals ordered depth-first over the rotation prefix trie (lexicographic order of the
// sequences keeps every subtree contiguous), then cut into `world` chunks with the smallest key-switch
// budget per chunk that fits (binary search).  A cut inside a subtree only repeats the path above it, so
// the ranks together spend about the 1-GPU trie's key switches.  Same rule as shard.plan_diagonal_shards.
void plan_elts(std::size_t N, int step, const std::set<u32> &keys, std::vector<u32> &out)
{
    if (step == 0) return;
    const u64 m = 2 * N;
    const u64 s = step < 0 ? (u64)((long)N / 2 + step) : (u64)step;
    u64 e = 1;
    for (u64 k = 0; k < s; ++k) e = e * 3 % m;
    if (keys.count((u32)e)) { out.push_back((u32)e); return; }
    for (int t : naf(step))
        if ((std::size_t)std::abs(t) != N / 2) plan_elts(N, t, keys, out);
}
std::vector<std::vector<std::size_t>> plan_shards(std::size_t N, std::size_t n, int world, const std::set<u32> &keys)
{
    need(world >= 1 && (std::size_t)world <= n, "need 1 <= world <= n");
    std::vector<std::vector<u32>> seq(n);
    for (std::size_t j = 0; j < n; ++j) plan_elts(N, (int)j, keys, seq[j]);
    std::vector<std::size_t> order(n);
    for (std::size_t j = 0; j < n; ++j) order[j] = j;
    std::stable_sort(order.begin(), order.end(), [&](std::size_t a, std::size_t b) { return seq[a] < seq[b]; });
    auto prefixes = [&](std::size_t j) {
        std::vector<std::vector<u32>> pre;
        for (std::size_t k = 1; k <= seq[j].size(); ++k) pre.emplace_back(seq[j].begin(), seq[j].begin() + k);
        return pre;
    };
    std::set<std::vector<u32>> all;
    for (std::size_t j = 0; j < n; ++j)
        for (auto &x : prefixes(j)) all.insert(x);
    const std::size_t total = all.size();
    auto chunk = [&](std::size_t budget, std::size_t limit, std::vector<std::vector<std::size_t>> &out) {
        out.clear();
        std::vector<std::size_t> cur;
        std::set<std::vector<u32>> seen;
        std::size_t cost = 0;
        for (std::size_t j : order) {
            const auto pre = prefixes(j);
            std::size_t add = 0;
            for (auto &x : pre) add += seen.count(x) ? 0 : 1;
            if (!cur.empty() && cost + add > budget) {
                out.push_back(cur);
                if (out.size() >= limit) return false;
                cur.clear();
                seen.clear();
                cost = 0;
                add = pre.size();
            }
            cur.push_back(j);
            for (auto &x : pre) seen.insert(x);
            cost += add;
        }
        out.push_back(cur);
        return true;
    };
    std::size_t lo = std::max<std::size_t>(1, total / (std::size_t)world), hi = total + 1;
    std::vector<std::vector<std::size_t>> best, tmp;
    while (lo <= hi) {
        const std::size_t mid = (lo + hi) / 2;
        if (chunk(mid, (std::size_t)world, tmp)) {
            best = tmp;
            hi = mid - 1;
        } else {
            lo = mid + 1;
        }
    }
    while ((int)best.size() < world) {  // split the largest chunks until every rank has one
        std::size_t k = 0;
        for (std::size_t i = 1; i < best.size(); ++i)
            if (best[i].size() > best[k].size()) k = i;
        std::vector<std::size_t> c = best[k];
        best.erase(best.begin() + (long)k);
        best.insert(best.begin() + (long)k, std::vector<std::size_t>(c.begin() + (long)(c.size() / 2), c.end()));
        best.insert(best.begin() + (long)k, std::vector<std::size_t>(c.begin(), c.begin() + (long)(c.size() / 2)));
    }
    for (auto &c : best) std::sort(c.begin(), c.end());
    return best;
}

// RCCL, loaded on first use (the engine itself does not link it): the functions of rccl.h we call
struct Rccl {
    decltype(&ncclGetUniqueId) get_unique_id = nullptr;
    decltype(&ncclCommInitRank) init_rank = nullptr;
    decltype(&ncclCommDestroy) destroy = nullptr;
    decltype(&ncclAllReduce) all_reduce = nullptr;
    decltype(&ncclGetErrorString) error_string = nullptr;
};
const Rccl &rccl()
{
    static Rccl r;
    static bool tried = false;
    static std::mutex mu;
    std::lock_guard<std::mutex> lock(mu);
    if (!tried) {
        tried = true;
        void *h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (h) {
            r.get_unique_id = (decltype(r.get_unique_id))dlsym(h, "ncclGetUniqueId");
            r.init_rank = (decltype(r.init_rank))dlsym(h, "ncclCommInitRank");
            r.destroy = (decltype(r.destroy))dlsym(h, "ncclCommDestroy");
            r.all_reduce = (decltype(r.all_reduce))dlsym(h, "ncclAllReduce");
            r.error_string = (decltype(r.error_string))dlsym(h, "ncclGetErrorString");
        }
    }
    if (!r.get_unique_id || !r.init_rank || !r.all_reduce || !r.destroy)
        throw std::logic_error("RCCL (librccl.so.1) is not available");
    return r;
}
void nccl_check(ncclResult_t e, const char *what)
{
    if (e != ncclSuccess)
        throw std::logic_error(std::string(what) + ": " + (rccl().error_string ? rccl().error_string(e) : "RCCL error"));
}

struct RcclComm final : HecComm {
    ncclComm_t comm;
    explicit RcclComm(ncclComm_t c) : comm(c) {}
    ~RcclComm() override { (void)rccl().destroy(comm); }
    void allreduce_f64(double *host, std::size_t n, int op, hipStream_t s) override
    {
        double *dv = nullptr;
        HEC_HIP(hipMallocAsync((void **)&dv, n * sizeof(double), s));
        HEC_HIP(hipMemcpyAsync(dv, host, n * sizeof(double), hipMemcpyHostToDevice, s));
        nccl_check(rccl().all_reduce(dv, dv, n, ncclFloat64, op == HEC_REDUCE_MIN ? ncclMin : ncclMax, comm, s),
                   "ncclAllReduce");
        HEC_HIP(hipMemcpyAsync(host, dv, n * sizeof(double), hipMemcpyDeviceToHost, s));
        HEC_HIP(hipFreeAsync(dv, s));
        HEC_HIP(hipStreamSynchronize(s));
    }
    void allreduce_u64_sum(u64 *dev, std::size_t n, hipStream_t s) override
    {
        nccl_check(rccl().all_reduce(dev, dev, n, ncclUint64, ncclSum, comm, s), "ncclAllReduce");
    }
};

// the caller's host collectives (hec_comm_ops): MPI, torch.distributed (gloo), ...
struct OpsComm final : HecComm {
    hec_comm_ops ops;
    explicit OpsComm(const hec_comm_ops &o) : ops(o) {}
    void allreduce_f64(double *host, std::size_t n, int op, hipStream_t) override
    {
        if (ops.allreduce_f64(ops.user, host, n, op) != 0) throw std::logic_error("hec_comm_ops allreduce_f64 failed");
    }
    void allreduce_u64_sum(u64 *dev, std::size_t n, hipStream_t s) override
    {
        std::vector<u64> h(n);
        HEC_HIP(hipMemcpyAsync(h.data(), dev, n * sizeof(u64), hipMemcpyDeviceToHost, s));
        HEC_HIP(hipStreamSynchronize(s));
        if (ops.allreduce_u64_sum(ops.user, h.data(), n) != 0)
            throw std::logic_error("hec_comm_ops allreduce_u64_sum failed");
        HEC_HIP(hipMemcpyAsync(dev, h.data(), n * sizeof(u64), hipMemcpyHostToDevice, s));
        HEC_HIP(hipStreamSynchronize(s));
    }
};

// The sharded matvec's agreement step, before any data-path collective: every rank contributes its own argument
// check (status, SEAL's message) and its p product scales; all ranks return the same verdict, so an argument error
// on one rank is an error on every rank instead of a rank left waiting in the exchange, and SEAL's add_inplace "scale
// mismatch" is checked over the whole sum (he_linalg.cpp:977-997 adds every rank's terms).  Two all-reduces of p + 1
// doubles: [0] = (status << 8) | (rank + 1) of a failing rank (max, so the highest failing rank names the error),
// [1 .. p] the scales (min and max; a failing rank contributes +inf / -inf so it never decides the comparison).
int shard_agree(HecComm &cm, int rank, int status, std::string &msg, const double *ps, std::size_t p, hipStream_t s)
{
    std::vector<double> mn(1 + p), mx(1 + p);
    mn[0] = mx[0] = status ? (double)((status << 8) | (rank + 1)) : 0.0;
    for (std::size_t i = 0; i < p; ++i) {
        mn[1 + i] = status ? std::numeric_limits<double>::infinity() : ps[i];
        mx[1 + i] = status ? -std::numeric_limits<double>::infinity() : ps[i];
    }
    cm.allreduce_f64(mn.data(), mn.size(), HEC_REDUCE_MIN, s);
    cm.allreduce_f64(mx.data(), mx.size(), HEC_REDUCE_MAX, s);
    const int agreed = (int)mx[0];
    if (!status && agreed) {
        status = agreed >> 8;
        msg = "matmul_diag_col_sharded: the arguments failed SEAL's checks on rank " + std::to_string((agreed & 0xff) - 1);
    }
    if (!status)
        for (std::size_t i = 0; i < p; ++i)
            if (!are_close(mn[1 + i], mx[1 + i])) {
                status = HEC_EINVAL;
                msg = "scale mismatch";
                break;
            }
    return status;
}
}  // namespace

// =============================================================================== workspace ==
void hec::Workspace::reserve(std::size_t w, hipStream_t stream)
{
    if (w <= words) return;
    if (std::getenv("HEC_DEBUG")) std::fprintf(stderr, "hec: workspace %zu -> %zu words\n", words, w);
    (void)stream;
    if (base) retired.push_back(base);  // reclaimed later (see Workspace)
    base = dalloc(w);
    words = w;
}
void hec::Workspace::reclaim(hipStream_t stream)
{
    if (retired.empty()) return;
    HEC_HIP(hipStreamSynchronize(stream));
    for (u64 *p : retired) HEC_HIP(hipFree(p));
    retired.clear();
}
void hec::Workspace::release()
{
    if (base) (void)hipFree(base);
    for (u64 *p : retired) (void)hipFree(p);
    retired.clear();
    base = nullptr;
    words = 0;
}

// =============================================================================== C-ABI =====
extern "C" {

const char *hec_last_error(void) { return g_err.c_str(); }
int hec_version(void) { return 100; }

int hec_create_coeff_modulus(uint64_t N, const int *bit_sizes, uint64_t count, uint64_t *out)
{
    return guard([&] {
        need(N >= 2 && !(N & (N - 1)), "poly_modulus_degree is invalid");
        std::map<int, std::size_t> cnt;
        for (uint64_t i = 0; i < count; ++i) {
            need(bit_sizes[i] >= 2 && bit_sizes[i] <= 60, "bit_sizes is invalid");
            ++cnt[bit_sizes[i]];
        }
        const u64 factor = 2 * N;
        std::map<int, std::vector<u64>> table;
        for (auto &[b, k] : cnt) {  // SEAL util::get_primes: walk down from ((2^b-1)/2N)*2N+1
            u64 v = (((u64)1 << b) - 1) / factor * factor + 1;
            const u64 lo = (u64)1 << (b - 1);
            std::size_t left = k;
            while (left && v > lo) {
                if (isprime(v)) { table[b].push_back(v); --left; }
                v -= factor;
            }
            if (left) throw std::logic_error("failed to find enough qualifying primes");
        }
        for (uint64_t i = 0; i < count; ++i) {  // CoeffModulus::Create: back(), pop_back()
            out[i] = table[bit_sizes[i]].back();
            table[bit_sizes[i]].pop_back();
        }
    });
}

int hec_context_create(uint64_t N, const uint64_t *mod, uint64_t K, int device, hec_context **out)
{
    return guard([&] {
        need(out != nullptr, "out is null");
        need(N >= 1024 && N <= 65536 && !(N & (N - 1)), "poly_modulus_degree must be a power of two in [2^10, 2^16]");
        need(K >= 2 && K - 1 <= HEC_MAXL, "coeff_modulus size is invalid");
        // SEAL's context validation: every modulus at most SEAL_USER_MOD_BIT_COUNT_MAX = 60 bits, prime,
        // = 1 mod 2N (NTT-friendly) and pairwise coprime.  The 60-bit bound is also what keeps the sharded
        // exchange's plain int64 sum of up to 8 partial residues exact (shard.py exchange_partials).
        for (uint64_t i = 0; i < K; ++i)
            need(isprime(mod[i]) && (mod[i] - 1) % (2 * N) == 0 && !(mod[i] >> 60), "coeff_modulus is invalid");
        for (uint64_t i = 0; i < K; ++i)
            for (uint64_t j = 0; j < i; ++j) need(mod[i] != mod[j], "coeff_modulus is invalid");
        int mac_divround = -1;
        if (const char *f = std::getenv("HEC_MAC_DIVROUND")) {  // an A/B value outside the range must not pass
            char *end = nullptr;
            const long v = std::strtol(f, &end, 10);
            need(end != f && *end == 0 && v >= 0 && v <= 1, "HEC_MAC_DIVROUND takes 0..1");
            mac_divround = (int)v;
        }
        int hmac_divround = -1;
        if (const char *f = std::getenv("HEC_HMAC_DIVROUND")) {
            char *end = nullptr;
            const long v = std::strtol(f, &end, 10);
            need(end != f && *end == 0 && v >= 0 && v <= 1, "HEC_HMAC_DIVROUND takes 0..1");
            hmac_divround = (int)v;
        }
        HEC_HIP(hipSetDevice(device));
        auto *ctx = new hec_context();
        Ctx &c = ctx->c;
        c.device = device;
        if (mac_divround >= 0) c.mac_divround = mac_divround;
        if (hmac_divround >= 0) c.hmac_divround = hmac_divround;
        if (const char *f = std::getenv("HEC_FUSED_MODUP_MAC")) c.fused_modup_mac = f[0] != '0';
        if (const char *f = std::getenv("HEC_FUSE_GALOIS")) c.fuse_galois = f[0] != '0';
        if (const char *f = std::getenv("HEC_FAN")) c.fan_out = f[0] != '0';
        if (const char *f = std::getenv("HEC_HOIST_SCAN")) c.hoist_scan = std::atoi(f);
        if (const char *f = std::getenv("HEC_LANES")) c.lanes = std::max(1, std::atoi(f));
        if (const char *f = std::getenv("HEC_HOIST")) c.hoist = f[0] != '0';
        if (const char *f = std::getenv("HEC_HMAC")) c.hmac_cfg = std::atoi(f);
        if (const char *f = std::getenv("HEC_HMAC_ODD3")) c.hmac_odd3 = std::atoi(f);
        if (const char *f = std::getenv("HEC_HOIST_MIN")) c.hoist_min_children = std::max(1, std::atoi(f));
        if (const char *f = std::getenv("HEC_TENSOR_DEFER")) c.tensor_defer_max = std::max(1, std::atoi(f));
        if (const char *f = std::getenv("HEC_TENSOR_BUFS")) c.tensor_defer_bufs = std::max(1, std::atoi(f));
        if (const char *f = std::getenv("HEC_TENSOR_XCD")) c.tensor_xcd = std::max(0, std::atoi(f));
        if (const char *f = std::getenv("HEC_POISON")) c.poison = f[0] != '0';
        if (const char *f = std::getenv("HEC_LANE_SERIAL")) c.lane_serial = f[0] != '0';
        if (const char *f = std::getenv("HEC_DEBUG_LANES")) c.debug_lanes = f[0] != '0';
        if (const char *f = std::getenv("HEC_KERNEL_MEMOPS")) c.kernel_memops = f[0] != '0';
        if (const char *f = std::getenv("HEC_SPLIT_BFLY")) c.split_bfly = std::atoi(f);
        if (const char *f = std::getenv("HEC_NTTB_SHFL")) c.nttb_shfl = std::min(2, std::max(0, std::atoi(f)));
        if (const char *f = std::getenv("HEC_NTTB_SHFL_DR")) c.nttb_shfl_dr = std::atoi(f) != 0;
        if (const char *f = std::getenv("HEC_HMAC_INT")) c.hmac_int = std::atoi(f) != 0;
        if (const char *f = std::getenv("HEC_MODDOWN1")) c.moddown1 = std::atoi(f) != 0;
        if (const char *f = std::getenv("HEC_NT_E")) c.nt_e = std::atoi(f) != 0;
        if (const char *f = std::getenv("HEC_BMAC_SPLIT")) c.bmac_split = f[0] != '0';
        c.N = N;
        c.logN = __builtin_ctzll(N);
        c.K = K;
        c.L = K - 1;
        c.q.assign(mod, mod + K);
        for (u64 q : c.q) c.bits.push_back(64 - __builtin_clzll(q));
        HEC_HIP(hipStreamCreateWithFlags(&c.stream, hipStreamNonBlocking));
        c.own_stream = true;
        std::vector<ulonglong2> tw(K * N), itw(K * N);
        std::vector<u64> psipow(K * 2 * N);  // hoisted mod-up: psi_i^e, e in [0, 2N)
        for (uint64_t i = 0; i < K; ++i) {
            const u64 q = c.q[i];
            DevPrime p{};
            p.q = q;
            u128 all = ~(u128)0, r = all / q;
            if (all % q == q - 1) r += 1;
            p.r0 = (u64)r;
            p.r1 = (u64)(r >> 64);
            p.ninv = invm(N % q, q);
            p.ninv_q = shoupq(p.ninv, q);
            p.fp = q < (1ull << 42) ? 1 : 0;  // exact FP64 NTT arithmetic (hec_device.h)
            p.qd = (double)q;
            p.qinv = 1.0 / (double)q;
            p.ninv_d = (double)p.ninv;
            c.hprimes.push_back(p);
            const u64 root = minimal_root(2 * N, q), iroot = invm(root, q);
            {
                u64 e = 1;
                for (uint64_t k = 0; k < 2 * N; ++k) {
                    psipow[i * 2 * N + k] = e;
                    e = (u64)((u128)e * root % q);
                }
            }
            u64 pw = 1, ipw = 1;
            for (uint64_t k = 0; k < N; ++k) {  // tw[bitrev(k)] = root^k
                const u32 t = brev((u32)k, c.logN);
                tw[i * N + t] = ulonglong2{pw, shoupq(pw, q)};
                itw[i * N + t] = ulonglong2{ipw, shoupq(ipw, q)};
                pw = (u64)((u128)pw * root % q);
                ipw = (u64)((u128)ipw * iroot % q);
            }
        }
        // pass-B re-laid tables: entry (s, i, r) = tw[(R + r) 2^s + i] at R (2^s - 1) + i R + r
        c.logR = (c.logN + 1) / 2;
        const uint64_t R = 1ull << c.logR, C = N / R;
        std::vector<ulonglong2> twb(K * N), itwb(K * N);
        for (uint64_t i = 0; i < K; ++i)
            for (uint64_t s = 0; (1ull << s) < C; ++s)
                for (uint64_t ii = 0; ii < (1ull << s); ++ii)
                    for (uint64_t r = 0; r < R; ++r) {
                        const uint64_t dst = i * N + R * ((1ull << s) - 1) + ii * R + r;
                        const uint64_t src = i * N + (R + r) * (1ull << s) + ii;
                        twb[dst] = tw[src];
                        itwb[dst] = itw[src];
                    }
        auto to_d = [](const std::vector<ulonglong2> &v) {
            std::vector<double> r(v.size());
            for (std::size_t k = 0; k < v.size(); ++k) r[k] = (double)v[k].x;  // exact when q < 2^42
            return r;
        };
        const std::vector<double> twf = to_d(tw), itwf = to_d(itw), twbf = to_d(twb), itwbf = to_d(itwb);
        for (auto [dst, src] : {std::pair{&c.twf, &twf}, std::pair{&c.itwf, &itwf}, std::pair{&c.twbf, &twbf},
                                std::pair{&c.itwbf, &itwbf}}) {
            HEC_HIP(hipMalloc(dst, K * N * sizeof(double)));
            HEC_HIP(hipMemcpy(*dst, src->data(), K * N * sizeof(double), hipMemcpyHostToDevice));
        }
        HEC_HIP(hipMalloc(&c.twb, K * N * sizeof(ulonglong2)));
        HEC_HIP(hipMalloc(&c.itwb, K * N * sizeof(ulonglong2)));
        HEC_HIP(hipMemcpy(c.twb, twb.data(), K * N * sizeof(ulonglong2), hipMemcpyHostToDevice));
        HEC_HIP(hipMemcpy(c.itwb, itwb.data(), K * N * sizeof(ulonglong2), hipMemcpyHostToDevice));
        {   // pass-B layout of the split-input Shoup words (k_bmac's integer targets): a = w 2^31 mod q of twb
            std::vector<u64> tba(K * N, 0);
            for (uint64_t i = 0; i < K; ++i)
                if (!c.hprimes[i].fp)
                    for (uint64_t k = 0; k < N; ++k) tba[i * N + k] = (u64)(((u128)twb[i * N + k].x << 31) % c.q[i]);
            HEC_HIP(hipMalloc(&c.twbs, K * N * sizeof(u64)));
            HEC_HIP(hipMemcpy(c.twbs, tba.data(), K * N * sizeof(u64), hipMemcpyHostToDevice));
        }
        {   // hoisted mod-up constants: psi powers per key prime, q_J mod q_I
            HEC_HIP(hipMalloc(&c.psipow, psipow.size() * sizeof(u64)));
            HEC_HIP(hipMemcpy(c.psipow, psipow.data(), psipow.size() * sizeof(u64), hipMemcpyHostToDevice));
            std::vector<u64> cji(c.L * K);
            for (std::size_t J = 0; J < c.L; ++J)
                for (std::size_t I = 0; I < K; ++I) cji[J * K + I] = c.q[J] % c.q[I];
            HEC_HIP(hipMalloc(&c.cji, cji.size() * sizeof(u64)));
            HEC_HIP(hipMemcpy(c.cji, cji.data(), cji.size() * sizeof(u64), hipMemcpyHostToDevice));
            HEC_HIP(hipMalloc(&c.zflag, 2 * sizeof(int)));
            HEC_HIP(hipMemset(c.zflag, 0, 2 * sizeof(int)));
        }
        {   // target-prime order tables per level (integer primes first)
            // second half (imap_split_at): row l = {l, then the data targets, integer primes first}
            std::vector<int> tab(2 * (c.L + 1) * (HEC_MAXL + 2), 0);
            c.imap_nint.assign(c.L + 1, 0);
            c.imap_pint = c.hprimes[K - 1].fp ? 0 : 1;
            for (std::size_t l = 1; l <= c.L; ++l) {
                int *t = tab.data() + l * (HEC_MAXL + 2), n = 0;
                int *t2 = tab.data() + (c.L + 1 + l) * (HEC_MAXL + 2), n2 = 0;
                t2[n2++] = (int)l;
                for (int pass = 0; pass < 2; ++pass)
                    for (int I = 0; I <= (int)l; ++I) {
                        const int kI = I == (int)l ? (int)K - 1 : I;
                        const bool fp = c.hprimes[kI].fp != 0;
                        if ((pass == 0) != fp) {
                            t[n++] = I;
                            if (I != (int)l) t2[n2++] = I;
                        }
                    }
                for (int I = 0; I <= (int)l; ++I)
                    if (!c.hprimes[I == (int)l ? K - 1 : I].fp) ++c.imap_nint[l];
            }
            HEC_HIP(hipMalloc(&c.imap, tab.size() * sizeof(int)));
            HEC_HIP(hipMemcpy(c.imap, tab.data(), tab.size() * sizeof(int), hipMemcpyHostToDevice));
        }
        HEC_HIP(hipMalloc(&c.primes, K * sizeof(DevPrime)));
        HEC_HIP(hipMemcpy(c.primes, c.hprimes.data(), K * sizeof(DevPrime), hipMemcpyHostToDevice));
        HEC_HIP(hipMalloc(&c.tw, K * N * sizeof(ulonglong2)));
        HEC_HIP(hipMalloc(&c.itw, K * N * sizeof(ulonglong2)));
        HEC_HIP(hipMemcpy(c.tw, tw.data(), K * N * sizeof(ulonglong2), hipMemcpyHostToDevice));
        HEC_HIP(hipMemcpy(c.itw, itw.data(), K * N * sizeof(ulonglong2), hipMemcpyHostToDevice));
        {   // split-input Shoup words a = w 2^31 mod q of tw / itw (integer primes; hec_device.h shoup_split_lazy)
            std::vector<u64> ta(K * N, 0), ita(K * N, 0);
            for (uint64_t i = 0; i < K; ++i) {
                if (c.hprimes[i].fp) continue;
                const u64 q = c.q[i];
                for (uint64_t k = 0; k < N; ++k) {
                    ta[i * N + k] = (u64)(((u128)tw[i * N + k].x << 31) % q);
                    ita[i * N + k] = (u64)(((u128)itw[i * N + k].x << 31) % q);
                }
            }
            HEC_HIP(hipMalloc(&c.tws, K * N * sizeof(u64)));
            HEC_HIP(hipMalloc(&c.itws, K * N * sizeof(u64)));
            HEC_HIP(hipMemcpy(c.tws, ta.data(), K * N * sizeof(u64), hipMemcpyHostToDevice));
            HEC_HIP(hipMemcpy(c.itws, ita.data(), K * N * sizeof(u64), hipMemcpyHostToDevice));
        }
        const u64 P = c.q[K - 1];
        for (uint64_t i = 0; i < c.L; ++i) {
            const u64 q = c.q[i], pi = invm(P % q, q);
            c.p_inv.push_back(pi);
            c.p_inv_q.push_back(shoupq(pi, q));
            c.p_half_mod.push_back((P >> 1) % q);
        }
        c.ql_inv.assign(c.L + 1, {});
        c.ql_inv_q.assign(c.L + 1, {});
        c.ql_half_mod.assign(c.L + 1, {});
        for (uint64_t l = 2; l <= c.L; ++l)
            for (uint64_t i = 0; i + 1 < l; ++i) {
                const u64 q = c.q[i], ql = c.q[l - 1], v = invm(ql % q, q);
                c.ql_inv[l].push_back(v);
                c.ql_inv_q[l].push_back(shoupq(v, q));
                c.ql_half_mod[l].push_back((ql >> 1) % q);
            }
        // the tables went up with blocking copies on the null stream, which the non-blocking context stream does
        // not wait for: finish them before any kernel can read them
        HEC_HIP(hipDeviceSynchronize());
        ctx->gen = hec_live::ctx_register(ctx);
        *out = ctx;
    });
}

int hec_context_destroy(hec_context *ctx)
{
    return guard([&] {
        if (!ctx) return;
        hec_live::ctx_unregister(ctx);  // waits for a destroy that is draining this context's stream
        Ctx &c = ctx->c;
        (void)hipSetDevice(c.device);
        (void)hipStreamSynchronize(c.stream);
        for (hec_context *l : ctx->lanes) free_lane(l);
        if (ctx->lanes_start) (void)hipEventDestroy(ctx->lanes_start);
        delete ctx->comm;
        c.ws.release();
        (void)hipFree(c.primes);
        (void)hipFree(c.imap);
        (void)hipFree(c.psipow);
        (void)hipFree(c.cji);
        (void)hipFree(c.zflag);
        (void)hipFree(c.tw);
        (void)hipFree(c.itw);
        (void)hipFree(c.twb);
        (void)hipFree(c.itwb);
        (void)hipFree(c.tws);
        (void)hipFree(c.itws);
        (void)hipFree(c.twbs);
        for (double *p : {c.twf, c.itwf, c.twbf, c.itwbf}) (void)hipFree(p);
        (void)hipFree(c.enc_map);
        (void)hipFree(c.enc_tw);
        (void)hipFree(c.dec_tw);
        for (u64 *t : c.dec_crt) (void)hipFree(t);
        if (c.own_stream) (void)hipStreamDestroy(c.stream);
        for (hipEvent_t e : c.ev_pool) (void)hipEventDestroy(e);
        delete ctx;
    });
}

int hec_context_set_stream(hec_context *ctx, void *stream)
{
    return guard([&] {
        set_device(ctx);
        Ctx &c = ctx->c;
        HEC_HIP(hipStreamSynchronize(c.stream));
        if (c.own_stream) HEC_HIP(hipStreamDestroy(c.stream));
        if (stream) {
            c.stream = (hipStream_t)stream;
            c.own_stream = false;
        } else {
            HEC_HIP(hipStreamCreateWithFlags(&c.stream, hipStreamNonBlocking));
            c.own_stream = true;
        }
    });
}

int hec_context_set_option(hec_context *ctx, const char *name, int64_t value)
{
    return guard([&] {
        need(ctx && name, "null argument");
        set_device(ctx);
        const std::string n(name);
        // the enumerated knobs take only their listed values (a typo in an A/B value must not pass as
        // another schedule)
        auto in = [&](int64_t lo, int64_t hi) {
            if (value < lo || value > hi)
                throw std::invalid_argument("option " + n + " takes " + std::to_string(lo) + ".." + std::to_string(hi));
            return (int)value;
        };
        auto one_of = [&](auto list, const char *takes) {  // a kernel tile: the members of its list (hec_internal.h)
            if (!list.has(value)) throw std::invalid_argument("option " + n + takes);
            return (int)value;
        };
        auto apply = [&](Ctx &c) {
            if (n == "lanes") c.lanes = (int)std::max<int64_t>(1, value);
            else if (n == "lane_min_batch") c.lane_min_batch = (int)std::max<int64_t>(1, value);
            else if (n == "poison") c.poison = value != 0;
            else if (n == "lane_serial") c.lane_serial = value != 0;
            else if (n == "debug_lanes") c.debug_lanes = value != 0;
            else if (n == "kernel_memops") c.kernel_memops = value != 0;
            else if (n == "split_bfly") c.split_bfly = in(0, 4);
            else if (n == "nttb_shfl") c.nttb_shfl = in(0, 2);
            else if (n == "nttb_shfl_dr") c.nttb_shfl_dr = in(0, 1);
            else if (n == "hmac_int") c.hmac_int = in(0, 1);
            else if (n == "moddown1") c.moddown1 = in(0, 1);
            else if (n == "nt_e") c.nt_e = in(0, 1);
            else if (n == "bmac_split") c.bmac_split = value != 0;
            else if (n == "mac_divround") c.mac_divround = in(0, 1);
            else if (n == "hmac_divround") c.hmac_divround = in(0, 1);
            else if (n == "hoist") c.hoist = value != 0;
            else if (n == "hoist_min") c.hoist_min_children = (int)std::max<int64_t>(1, value);
            else if (n == "hmac") c.hmac_cfg = in(0, 2);
            else if (n == "hmac_odd3") c.hmac_odd3 = in(0, 1);
            else if (n == "hoist_scan") c.hoist_scan = in(0, 1);
            else if (n == "fan") c.fan_out = value != 0;
            else if (n == "fuse_galois") c.fuse_galois = value != 0;
            else if (n == "fused_modup_mac") c.fused_modup_mac = value != 0;
            else if (n == "tensor_defer") c.tensor_defer_max = (int)std::max<int64_t>(1, value);
            else if (n == "tensor_bufs") c.tensor_defer_bufs = (int)std::max<int64_t>(1, value);
            else if (n == "tensor_xcd") c.tensor_xcd = (int)std::max<int64_t>(0, value);
            else if (n == "prng_group") c.prng_group = in(0, 16);
            else if (n == "math_chunk") c.math_chunk = in(0, 65535);
            else if (n == "rot_add") c.rot_add = in(0, 1);
            else if (n == "bsgs_chunk") c.bsgs_chunk = in(0, 65535);
            else if (n == "bsgs_bg") c.bsgs_bg = one_of(BsgsBG{}, " takes 1, 2 or 4");
            else if (n == "bsgs_gg") c.bsgs_gg = one_of(BsgsGG{}, " takes 2, 4, 8 or 16");
            else if (n == "bsgs_ct_bg") c.bsgs_ct_bg = one_of(BsgsCtBG{}, " takes 1 or 2");
            else if (n == "bsgs_ct_gg") c.bsgs_ct_gg = one_of(BsgsCtGG{}, " takes 2, 4 or 8");
            else if (n == "bsgs_order") c.bsgs_order = in(0, 1);
            else if (n == "cct_jchunk") c.cct_jchunk = in(0, 512);
            else if (n == "cct_tb") c.cct_tb = one_of(CctTB{}, " takes 1, 2 or 4");
            else if (n == "cct_tg") c.cct_tg = one_of(CctTG{}, " takes 1, 2 or 4");
            else throw std::invalid_argument("unknown option");
        };
        HEC_HIP(hipStreamSynchronize(ctx->c.stream));
        apply(ctx->c);
        for (hec_context *l : ctx->lanes) {  // the lanes hold copies of the knobs (make_lane)
            HEC_HIP(hipStreamSynchronize(l->c.stream));
            apply(l->c);
        }
    });
}

int hec_context_synchronize(hec_context *ctx)
{
    return guard([&] {
        set_device(ctx);
        HEC_HIP(hipStreamSynchronize(ctx->c.stream));
    });
}
uint64_t hec_context_poly_degree(const hec_context *ctx) { return ctx ? ctx->c.N : 0; }
uint64_t hec_context_key_moduli(const hec_context *ctx) { return ctx ? ctx->c.K : 0; }

uint32_t hec_galois_elt_from_step(const hec_context *ctx, int step)
{
    u32 e = 0;
    if (guard([&] { e = elt_from_step(ctx->c, step); })) return 0;
    return e;
}

uint64_t hec_default_galois_elts(const hec_context *ctx, uint32_t *out)
{
    const u32 m = (u32)(2 * ctx->c.N);
    std::vector<u32> v{m - 1};
    u64 pos = 3, neg = invm(3, m);
    for (int i = 0; i < ctx->c.logN - 1; ++i) {  // SEAL GaloisTool::get_elts_all
        v.push_back((u32)pos);
        pos = (pos * pos) & (m - 1);
        v.push_back((u32)neg);
        neg = (neg * neg) & (m - 1);
    }
    if (out) std::memcpy(out, v.data(), v.size() * sizeof(u32));
    return v.size();
}

// ------------------------------------------------------------------ ciphertext / plaintext
int hec_ciphertext_create(hec_context *ctx, hec_ciphertext **out)
{
    return guard([&] {
        need(ctx && out, "null argument");
        *out = make<hec_ciphertext, hec_ciphertext_destroy>(ctx).release();
    });
}
int hec_ciphertext_destroy(hec_ciphertext *ct) { return release(ct); }
int hec_ciphertext_upload(hec_ciphertext *ct, const uint64_t *host, uint64_t size, uint64_t level, double scale)
{
    return guard([&] {
        need(ct && host, "null argument");
        Ctx &c = live(ct, BAD_CT);
        need(size >= 1 && level >= 1 && level <= c.K, BAD_CT);
        const std::size_t w = size * level * c.N;
        grow(ct, w);
        HEC_HIP(hipMemcpyAsync(ct->d, host, w * sizeof(u64), hipMemcpyHostToDevice, c.stream));
        HEC_HIP(hipStreamSynchronize(c.stream));
        ct->size = size; ct->level = level; ct->scale = scale;
    });
}
int hec_ciphertext_download(const hec_ciphertext *ct, uint64_t *host)
{
    return guard([&] {
        need(ct && host && ct->d, "null argument");
        Ctx &c = live(ct, BAD_CT);
        const std::size_t w = ct->size * ct->level * c.N;
        HEC_HIP(hipMemcpyAsync(host, ct->d, w * sizeof(u64), hipMemcpyDeviceToHost, c.stream));
        HEC_HIP(hipStreamSynchronize(c.stream));
    });
}
int hec_ciphertext_info(const hec_ciphertext *ct, uint64_t *size, uint64_t *level, double *scale)
{
    return guard([&] {
        need(ct != nullptr, "null argument");
        if (size) *size = ct->size;
        if (level) *level = ct->level;
        if (scale) *scale = ct->scale;
    });
}
int hec_ciphertext_copy(hec_ciphertext *dst, const hec_ciphertext *src)
{
    return guard([&] {
        need(dst && src && dst->ctx == src->ctx && dst->ctx_gen == src->ctx_gen, "null argument");
        Ctx &c = live(dst, BAD_CT);
        if (dst == src) return;
        store_ct(c, dst, src->d, src->size, src->level, src->scale);
    });
}
int hec_ciphertext_export_device(const hec_ciphertext *ct, void *dev_dst)
{
    return guard([&] {
        need(ct && dev_dst && ct->d, "null argument");
        Ctx &c = live(ct, BAD_CT);
        d2d(c, dev_dst, ct->d, ct->size * ct->level * c.N);
    });
}
int hec_ciphertext_import_device(hec_ciphertext *ct, const void *dev_src, uint64_t size, uint64_t level, double scale)
{
    return guard([&] {
        need(ct && dev_src, "null argument");
        Ctx &c = live(ct, BAD_CT);
        const std::size_t w = size * level * c.N;
        grow(ct, w);
        d2d(c, ct->d, dev_src, w);
        ct->size = size; ct->level = level; ct->scale = scale;
    });
}
int hec_ciphertext_reduce(hec_context *ctx, hec_ciphertext *ct)
{
    return guard([&] {
        check_ct(ctx, ct);
        set_device(ctx);
        ew_reduce(ctx->c, ct->d, (int)ct->size, (int)ct->level);
    });
}
int hec_ciphertext_fill_uniform(hec_ciphertext *ct, uint64_t size, uint64_t level, double scale, uint64_t seed)
{
    return guard([&] {
        need(ct != nullptr, "null argument");
        Ctx &c = live(ct, BAD_CT);
        need(size >= 1 && level >= 1 && level <= c.L, BAD_CT);
        grow(ct, size * level * c.N);
        fill_uniform(c, ct->d, (int)size, (int)level, 0, 0, seed);
        ct->size = size; ct->level = level; ct->scale = scale;
    });
}

int hec_plaintext_create(hec_context *ctx, hec_plaintext **out)
{
    return guard([&] {
        need(ctx && out, "null argument");
        *out = make<hec_plaintext, hec_plaintext_destroy>(ctx).release();
    });
}
int hec_plaintext_destroy(hec_plaintext *pt) { return release(pt); }
int hec_plaintext_fill_uniform(hec_plaintext *pt, uint64_t level, double scale, uint64_t seed)
{
    return guard([&] {
        need(pt != nullptr, "null argument");
        Ctx &c = live(pt, BAD_PLAIN);
        need(level >= 1 && level <= c.L, BAD_PLAIN);
        grow(pt, level * c.N);
        fill_uniform(c, pt->d, 1, (int)level, 0, 0, seed);
        pt->level = level; pt->scale = scale;
    });
}

int hec_plaintext_upload(hec_plaintext *pt, const uint64_t *host, uint64_t level, double scale)
{
    return guard([&] {
        need(pt && host, "null argument");
        Ctx &c = live(pt, BAD_PLAIN);
        need(level >= 1 && level <= c.L, BAD_PLAIN);
        const std::size_t w = level * c.N;
        grow(pt, w);
        HEC_HIP(hipMemcpyAsync(pt->d, host, w * sizeof(u64), hipMemcpyHostToDevice, c.stream));
        HEC_HIP(hipStreamSynchronize(c.stream));
        pt->level = level; pt->scale = scale;
    });
}

int hec_plaintext_download(const hec_plaintext *pt, uint64_t *host)
{
    return guard([&] {
        need(pt && host, "null argument");
        need(pt->d != nullptr, BAD_PLAIN);
        Ctx &c = live(pt, BAD_PLAIN);
        HEC_HIP(hipMemcpyAsync(host, pt->d, pt->level * c.N * sizeof(u64), hipMemcpyDeviceToHost, c.stream));
        HEC_HIP(hipStreamSynchronize(c.stream));
    });
}

int hec_plaintext_info(const hec_plaintext *pt, uint64_t *level, double *scale)
{
    return guard([&] {
        need(pt != nullptr, "null argument");
        if (level) *level = pt->level;
        if (scale) *scale = pt->scale;
    });
}

// ------------------------------------------------------------------ CKKS encoder ----------
namespace {
// host tables of the GPU encoder (hec_encode.hip), built once per context, as SEAL 4.1's CKKSEncoder constructor
// builds them: matrix_reps_index_map_ (generator 3, bit-reversed positions) and inv_root_powers_[i] =
// conj(ComplexRoots(2N).get_root(bitrev(i - 1, logN) + 1)), where ComplexRoots holds (cos t, sin t),
// t = (i 6.283185307179586) / 2N for i <= 2N / 8 (glibc cos and sin as separate calls) and get_root extends them by
// the 8-fold symmetry
struct SealRoots {  // a class member: no C language linkage inside the C-ABI block
static std::complex<double> get(u64 m, const std::vector<std::complex<double>> &roots, u64 index)
{
    index &= m - 1;
    if (index <= m / 8) return roots[index];
    if (index <= m / 4) {
        const auto a = roots[m / 4 - index];
        return {a.imag(), a.real()};
    }
    if (index <= m / 2) {
        const auto a = get(m, roots, m / 2 - index);
        return {-a.real(), a.imag()};
    }
    if (index <= 3 * m / 4) {
        const auto a = get(m, roots, index - m / 2);
        return {-a.real(), -a.imag()};
    }
    const auto a = get(m, roots, m - index);
    return {a.real(), -a.imag()};
}
};
}  // namespace
extern "C++" {  // C++ linkage inside the C-ABI block, as hec_host.h declares it
namespace hec {
void encoder_tables(Ctx &c)
{
    if (c.enc_map) return;
    const u64 N = c.N, slots = N / 2, m = 2 * N;
    std::vector<u32> map(N);
    u64 pos = 1;
    for (u64 i = 0; i < slots; ++i) {
        map[i] = brev((u32)((pos - 1) >> 1), c.logN);
        map[slots + i] = brev((u32)((m - pos - 1) >> 1), c.logN);
        pos = (pos * 3) & (m - 1);
    }
    double (*volatile vcos)(double) = std::cos;  // never fused into sincos
    double (*volatile vsin)(double) = std::sin;
    std::vector<std::complex<double>> roots(m / 8 + 1);
    for (u64 i = 0; i <= m / 8; ++i) {
        const double t = ((double)i * 6.283185307179586) / (double)m;
        roots[i] = {vcos(t), vsin(t)};
    }
    std::vector<double> inv(2 * N, 0.0);
    for (u64 i = 1; i < N; ++i) {
        const auto r = SealRoots::get(m, roots, (u64)brev((u32)(i - 1), c.logN) + 1);
        inv[2 * i] = r.real();
        inv[2 * i + 1] = -r.imag();
    }
    u32 *dm = nullptr;
    double *dt = nullptr;
    HEC_HIP(hipMalloc(&dm, N * sizeof(u32)));
    HEC_HIP(hipMalloc(&dt, inv.size() * sizeof(double)));
    HEC_HIP(hipMemcpyAsync(dm, map.data(), N * sizeof(u32), hipMemcpyHostToDevice, c.stream));
    HEC_HIP(hipMemcpyAsync(dt, inv.data(), inv.size() * sizeof(double), hipMemcpyHostToDevice, c.stream));
    HEC_HIP(hipStreamSynchronize(c.stream));  // the host tables go out of scope
    c.enc_map = dm;
    c.enc_tw = dt;
}
}  // namespace hec
}  // extern "C++"

int hec_encode(hec_context *ctx, const double *re, const double *im, uint64_t n_values, uint64_t count, double scale,
               uint64_t level, hec_plaintext *const *out)
{
    return guard([&] {
        need(ctx && out && (re || n_values == 0), "null argument");
        Ctx &c = ctx->c;
        set_device(ctx);
        // argument checks in SEAL CKKSEncoder::encode_internal's order
        if (n_values > c.N / 2) throw std::invalid_argument("values has invalid size");
        if (level < 1 || level > c.L) throw std::invalid_argument("parms_id is not valid for encryption parameters");
        if (scale <= 0 || (int)std::log2(scale) >= c.total_bits(level)) throw std::invalid_argument("scale out of bounds");
        for (u64 v = 0; v < count; ++v) check_obj(ctx, out[v], BAD_PLAIN);
        if (count == 0) return;
        encoder_tables(c);
        const u64 N = c.N, nv = n_values;
        // chunks of vectors: the work area (2N doubles + level N residues per vector) stays under ~2 GiB
        const u64 per = 2 * N + level * N + 2 * nv + 1;
        const u64 chunk = std::max<u64>(1, std::min<u64>(count, (u64(1) << 28) / per));
        std::vector<u64> mx(chunk);
        for (u64 v0 = 0; v0 < count; v0 += chunk) {
            const u64 cnt = std::min(chunk, count - v0);
            Scratch s(c, cnt * per + 5 * 64);
            double *dre = reinterpret_cast<double *>(s.take(std::max<u64>(cnt * nv, 1)));
            double *dim = im ? reinterpret_cast<double *>(s.take(std::max<u64>(cnt * nv, 1))) : nullptr;
            double *work = reinterpret_cast<double *>(s.take(cnt * 2 * N));
            u64 *res = s.take(cnt * level * N), *dmx = s.take(cnt);
            if (nv) {
                HEC_HIP(hipMemcpyAsync(dre, re + v0 * nv, cnt * nv * sizeof(double), hipMemcpyHostToDevice, c.stream));
                if (im)
                    HEC_HIP(hipMemcpyAsync(dim, im + v0 * nv, cnt * nv * sizeof(double), hipMemcpyHostToDevice,
                                           c.stream));
            }
            encode_batch(c, dre, dim, nv, (int)cnt, scale, (int)level, work, res, dmx);
            HEC_HIP(hipMemcpyAsync(mx.data(), dmx, cnt * sizeof(u64), hipMemcpyDeviceToHost, c.stream));
            HEC_HIP(hipStreamSynchronize(c.stream));
            for (u64 v = 0; v < cnt; ++v) {
                double maxabs;
                std::memcpy(&maxabs, &mx[v], sizeof(double));
                // ceil(log2(max(max |Re|, 1))) + 1 >= total coeff-modulus bits -> throw (SEAL encode_internal; the
                // maximum is over the unrounded real parts); a non-finite value is rejected the same way
                if (!std::isfinite(maxabs)) throw std::invalid_argument("encoded values are too large");
                const int max_bits = (int)std::ceil(std::log2(std::max(maxabs, 1.0))) + 1;
                if (max_bits >= c.total_bits(level)) throw std::invalid_argument("encoded values are too large");
            }
            for (u64 v = 0; v < cnt; ++v) {
                hec_plaintext *pt = out[v0 + v];
                const std::size_t w = level * N;
                grow(pt, w);
                d2d(c, pt->d, res + v * w, w);
                pt->level = level;
                pt->scale = scale;
            }
            HEC_HIP(hipStreamSynchronize(c.stream));  // the next chunk reuses the workspace
        }
    });
}

// the residue mod q of a non-negative integer-valued double a (exactly the integer a, as SEAL's 64-bit, 128-bit
// (fmod / division by 2^64) and multi-word decompositions give it)
static u64 exact_residue(double a, u64 q)
{
    if (a < 18446744073709551616.0) return (u64)a % q;
    int e = 0;
    const double f = std::frexp(a, &e);  // a = f 2^e, 0.5 <= f < 1, e > 64
    u64 r = (u64)std::ldexp(f, 53) % q, pw = 2 % q;
    for (int k = e - 53; k > 0; k >>= 1) {  // r *= 2^(e - 53) mod q
        if (k & 1) r = (u64)((unsigned __int128)r * pw % q);
        pw = (u64)((unsigned __int128)pw * pw % q);
    }
    return r;
}

extern "C++" {  // as encoder_tables above
namespace hec {
// SEAL 4.1 CKKSEncoder::encode_internal(double value, parms_id, scale, destination) up to its fill: the checks, in its
// order, and the word of every limb (Chain: hec_host.h)
void scalar_words(const Ctx &c, double value, double scale, std::size_t level, u64 *words)
{
    scalar_words_chain(Chain{c.q.data(), c.L}, value, scale, level, words);
}
void scalar_words_chain(const Chain &c, double value, double scale, std::size_t level, u64 *words)
{
    if (level < 1 || level > c.L) throw std::invalid_argument("parms_id is not valid for encryption parameters");
    const int total = c.total_bits(level);
    if (scale <= 0 || (int)std::log2(scale) >= total) throw std::invalid_argument("scale out of bounds");
    value *= scale;
    // coeff_bit_count = int(log2 |value|) + 2; a zero value passes (SEAL's cast of -inf), a non-finite one is
    // rejected (SEAL would cast NaN / inf to int: undefined behaviour)
    if (!std::isfinite(value)) throw std::invalid_argument("encoded value is too large");
    if (value != 0.0 && (int)std::log2(std::fabs(value)) + 2 >= total)
        throw std::invalid_argument("encoded value is too large");
    const double cd = std::round(value);
    const bool neg = std::signbit(cd);
    const double a = std::fabs(cd);
    for (std::size_t j = 0; j < level; ++j) {
        const u64 q = c.q[j], r = exact_residue(a, q);
        words[j] = neg && r ? q - r : r;  // negate_uint_mod
    }
}
}  // namespace hec
}  // extern "C++"

int hec_encode_scalar(hec_context *ctx, double value, double scale, uint64_t level, hec_plaintext *out)
{
    return guard([&] {
        need(ctx && out, "null argument");
        Ctx &c = ctx->c;
        set_device(ctx);
        if (level < 1 || level > c.L) throw std::invalid_argument("parms_id is not valid for encryption parameters");
        check_obj(ctx, out, BAD_PLAIN);
        u64 words[HEC_MAXL + 1];
        scalar_words(c, value, scale, level, words);
        // the constant polynomial in NTT form: every coefficient of limb j is the residue (SEAL's fill_n)
        grow(out, level * c.N);
        fill_limbs(c, out->d, (int)level, words);
        out->level = level;
        out->scale = scale;
    });
}

// ------------------------------------------------------------------ decrypt / decode -------
namespace {
struct Big {  // a class member: no C language linkage inside the C-ABI block
// little-endian multi-word x times a word
static std::vector<u64> mul(const std::vector<u64> &x, u64 s)
{
    std::vector<u64> r(x.size() + 1, 0);
    u64 carry = 0;
    for (std::size_t i = 0; i < x.size(); ++i) {
        const u128 t = (u128)x[i] * s + carry;
        r[i] = (u64)t;
        carry = (u64)(t >> 64);
    }
    r[x.size()] = carry;
    while (r.size() > 1 && r.back() == 0) r.pop_back();
    return r;
}
};
// host tables of the GPU decoder (hec_decode.hip), built on first use: root_powers_[i] = ComplexRoots(2N).get_root(
// bitrev(i, logN)) by the encoder's cos / sin route, and per level Q, (Q + 1) / 2, Q / q_i, (Q / q_i)^-1 mod q_i
void decoder_tables(Ctx &c, std::size_t level)
{
    encoder_tables(c);  // the slot map
    if (!c.dec_tw) {
        const u64 N = c.N, m = 2 * N;
        double (*volatile vcos)(double) = std::cos;
        double (*volatile vsin)(double) = std::sin;
        std::vector<std::complex<double>> roots(m / 8 + 1);
        for (u64 i = 0; i <= m / 8; ++i) {
            const double t = ((double)i * 6.283185307179586) / (double)m;
            roots[i] = {vcos(t), vsin(t)};
        }
        std::vector<double> rp(2 * N, 0.0);
        for (u64 i = 1; i < N; ++i) {
            const auto r = SealRoots::get(m, roots, (u64)brev((u32)i, c.logN));
            rp[2 * i] = r.real();
            rp[2 * i + 1] = r.imag();
        }
        double *dt = nullptr;
        HEC_HIP(hipMalloc(&dt, rp.size() * sizeof(double)));
        HEC_HIP(hipMemcpyAsync(dt, rp.data(), rp.size() * sizeof(double), hipMemcpyHostToDevice, c.stream));
        HEC_HIP(hipStreamSynchronize(c.stream));
        c.dec_tw = dt;
    }
    if (c.dec_crt[level]) return;
    std::vector<u64> Q{1};
    for (std::size_t i = 0; i < level; ++i) Q = Big::mul(Q, c.q[i]);
    const int wm = dec_wmax((int)Big::mul(Q, level).size());  // the composition's sum is below level Q
    std::vector<u64> tab((2 + level) * wm + level, 0);
    std::copy(Q.begin(), Q.end(), tab.begin());
    {  // (Q + 1) / 2 = (Q >> 1) + 1 for odd Q
        u64 *h = tab.data() + wm;
        for (std::size_t j = 0; j < Q.size(); ++j) h[j] = (Q[j] >> 1) | (j + 1 < Q.size() ? Q[j + 1] << 63 : 0);
        for (int j = 0; j < wm && ++h[j] == 0; ++j) {}
    }
    for (std::size_t i = 0; i < level; ++i) {
        std::vector<u64> P{1};
        u64 pm = 1;
        for (std::size_t j = 0; j < level; ++j) {
            if (j == i) continue;
            P = Big::mul(P, c.q[j]);
            pm = (u64)((u128)pm * (c.q[j] % c.q[i]) % c.q[i]);
        }
        std::copy(P.begin(), P.end(), tab.begin() + (2 + i) * wm);
        tab[(2 + level) * wm + i] = level == 1 ? 1 : invm(pm, c.q[i]);
    }
    u64 *d = dalloc(tab.size());
    HEC_HIP(hipMemcpyAsync(d, tab.data(), tab.size() * sizeof(u64), hipMemcpyHostToDevice, c.stream));
    HEC_HIP(hipStreamSynchronize(c.stream));
    c.dec_crt[level] = d;
    c.dec_wm[level] = wm;
}

struct DecEntry {
    const u64 *d;
    std::size_t size, level;  // size 1: a plaintext
    double scale;
};

// The shared driver of hec_decrypt (pts != null), hec_decode (sk == null, size-1 entries) and hec_decrypt_decode:
// rows in chunks that bound the work area, each chunk grouped by (size, level); every group runs k_decrypt, and,
// when decoding, INTT -> CRT + upper layers -> LDS layers -> gather into the chunk's rows, copied out once per chunk.
void dec_run(hec_context *ctx, const u64 *sk, const std::vector<DecEntry> &in, hec_plaintext *const *pts, u64 nv,
             double *re, double *im)
{
    Ctx &c = ctx->c;
    const u64 N = c.N, count = in.size();
    const bool decode = pts == nullptr;
    std::size_t lmax = 1;
    for (const DecEntry &e : in) {
        lmax = std::max(lmax, e.level);
        if (decode) decoder_tables(c, e.level);
    }
    const u64 per = lmax * N + (decode ? 2 * N + 2 * nv : 0) + 4;
    const u64 chunk = std::max<u64>(1, std::min<u64>({count, (u64(1) << 28) / per, 65535}));
    std::vector<const u64 *> hsrc(chunk);
    std::vector<double> his(chunk);
    std::vector<u32> hrow(chunk);
    for (u64 v0 = 0; v0 < count; v0 += chunk) {
        const u64 cnt = std::min(chunk, count - v0);
        Scratch s(c, cnt * per + 8 * 64);
        u64 *X = s.take(cnt * lmax * N);
        const u64 **dsrc = reinterpret_cast<const u64 **>(s.take(cnt));
        double *dis = nullptr, *work = nullptr, *dre = nullptr, *dim = nullptr;
        u32 *drow = nullptr;
        if (decode) {
            dis = reinterpret_cast<double *>(s.take(cnt));
            drow = reinterpret_cast<u32 *>(s.take(cnt));
            work = reinterpret_cast<double *>(s.take(cnt * 2 * N));
            dre = reinterpret_cast<double *>(s.take(std::max<u64>(cnt * nv, 1)));
            if (im) dim = reinterpret_cast<double *>(s.take(std::max<u64>(cnt * nv, 1)));
        }
        // the chunk's entries ordered by group; one upload of the pointer / scale / row lists for all groups
        std::map<std::pair<std::size_t, std::size_t>, std::vector<u32>> groups;
        for (u64 v = 0; v < cnt; ++v) groups[{in[v0 + v].size, in[v0 + v].level}].push_back((u32)v);
        u64 k = 0;
        for (const auto &g : groups)
            for (u32 v : g.second) {
                hsrc[k] = in[v0 + v].d;
                his[k] = 1.0 / in[v0 + v].scale;
                hrow[k] = v;
                ++k;
            }
        HEC_HIP(hipMemcpyAsync(dsrc, hsrc.data(), cnt * sizeof(u64 *), hipMemcpyHostToDevice, c.stream));
        if (decode) {
            HEC_HIP(hipMemcpyAsync(dis, his.data(), cnt * sizeof(double), hipMemcpyHostToDevice, c.stream));
            HEC_HIP(hipMemcpyAsync(drow, hrow.data(), cnt * sizeof(u32), hipMemcpyHostToDevice, c.stream));
        }
        u64 b0 = 0, xoff = 0;
        for (const auto &g : groups) {
            const std::size_t size = g.first.first, level = g.first.second, n = g.second.size();
            u64 *x = X + xoff;
            {  // compulsory bytes: the ciphertexts and the key limbs read, the plaintexts written
                ProfScope ps(c, "dec_decrypt", (double)(n * (size + 1) * level + (size > 1 ? level : 0)));
                decrypt_batch(c, dsrc + b0, sk, (int)size, (int)level, (int)n, x);
            }
            if (decode) {
                // the plaintext limbs read, N/2 complex slots written; 4 launches + the inverse NTT's two passes
                ProfScope ps(c, "dec_decode", (double)(n * (level + 1)), 6);
                decode_batch(c, x, (int)n, (int)level, c.dec_crt[level], c.dec_wm[level], dis + b0,
                             work + b0 * 2 * N, nv, drow + b0, dre, dim);
            } else {
                for (std::size_t j = 0; j < n; ++j) {
                    hec_plaintext *pt = pts[v0 + g.second[j]];
                    const std::size_t w = level * N;
                    grow(pt, w);
                    d2d(c, pt->d, x + j * w, w);
                    pt->level = level;
                    pt->scale = in[v0 + g.second[j]].scale;
                }
            }
            b0 += n;
            xoff += n * level * N;
        }
        if (decode && nv) {
            HEC_HIP(hipMemcpyAsync(re + v0 * nv, dre, cnt * nv * sizeof(double), hipMemcpyDeviceToHost, c.stream));
            if (im)
                HEC_HIP(hipMemcpyAsync(im + v0 * nv, dim, cnt * nv * sizeof(double), hipMemcpyDeviceToHost, c.stream));
        }
        HEC_HIP(hipStreamSynchronize(c.stream));  // host lists and outputs; the next chunk reuses the workspace
    }
}

void check_sk(const hec_context *ctx, const hec_secret_key *sk)
{
    check_obj(ctx, sk, BAD_SK);
    need(sk->d != nullptr, BAD_SK);
}
void check_dec_scale(const Ctx &c, double scale, std::size_t level)
{
    if (!scale_ok(c, scale, level)) throw std::invalid_argument("scale out of bounds");
}
}  // namespace

int hec_secret_key_upload(hec_context *ctx, const uint64_t *host, hec_secret_key **out)
{
    return guard([&] {
        need(ctx && host && out, "null argument");
        set_device(ctx);
        Ctx &c = ctx->c;
        auto k = make<hec_secret_key, hec_secret_key_destroy>(ctx);
        k->words = c.K * c.N;
        k->d = dalloc(k->words);
        HEC_HIP(hipMemcpyAsync(k->d, host, k->words * sizeof(u64), hipMemcpyHostToDevice, c.stream));
        HEC_HIP(hipStreamSynchronize(c.stream));
        *out = k.release();
    });
}
int hec_secret_key_download(const hec_secret_key *sk, uint64_t *host)
{
    return guard([&] {
        need(sk && host, "null argument");
        Ctx &c = live(sk, BAD_SK);
        HEC_HIP(hipMemcpyAsync(host, sk->d, sk->words * sizeof(u64), hipMemcpyDeviceToHost, c.stream));
        HEC_HIP(hipStreamSynchronize(c.stream));
    });
}
int hec_secret_key_destroy(hec_secret_key *sk) { return release(sk, sk ? sk->words : 0); }

int hec_decrypt(hec_context *ctx, const hec_secret_key *sk, const hec_ciphertext *const *cts, uint64_t count,
                hec_plaintext *const *out)
{
    return guard([&] {
        need(ctx && (count == 0 || (cts && out)), "null argument");
        set_device(ctx);
        check_sk(ctx, sk);
        std::vector<DecEntry> in(count);
        for (u64 i = 0; i < count; ++i) {
            check_ct(ctx, cts[i]);
            in[i] = {cts[i]->d, cts[i]->size, cts[i]->level, cts[i]->scale};
        }
        for (u64 i = 0; i < count; ++i) check_obj(ctx, out[i], BAD_PLAIN);
        if (count) dec_run(ctx, sk->d, in, out, 0, nullptr, nullptr);
    });
}

int hec_decode(hec_context *ctx, const hec_plaintext *const *pts, uint64_t count, uint64_t n_values, double *re,
               double *im)
{
    return guard([&] {
        need(ctx && (count == 0 || pts) && (re || count * n_values == 0), "null argument");
        set_device(ctx);
        Ctx &c = ctx->c;
        std::vector<DecEntry> in(count);
        for (u64 i = 0; i < count; ++i) {
            const hec_plaintext *p = pts[i];
            check_plain(ctx, p);
            in[i] = {p->d, 1, p->level, p->scale};
        }
        for (const DecEntry &e : in) check_dec_scale(c, e.scale, e.level);
        if (n_values > c.N / 2) throw std::invalid_argument("values has invalid size");
        if (count) dec_run(ctx, nullptr, in, nullptr, n_values, re, im);
    });
}

int hec_decrypt_decode(hec_context *ctx, const hec_secret_key *sk, const hec_ciphertext *const *cts, uint64_t count,
                       uint64_t n_values, double *re, double *im)
{
    return guard([&] {
        need(ctx && (count == 0 || cts) && (re || count * n_values == 0), "null argument");
        set_device(ctx);
        Ctx &c = ctx->c;
        check_sk(ctx, sk);
        std::vector<DecEntry> in(count);
        for (u64 i = 0; i < count; ++i) {
            check_ct(ctx, cts[i]);
            in[i] = {cts[i]->d, cts[i]->size, cts[i]->level, cts[i]->scale};
        }
        for (const DecEntry &e : in) check_dec_scale(c, e.scale, e.level);
        if (n_values > c.N / 2) throw std::invalid_argument("values has invalid size");
        if (count) dec_run(ctx, sk->d, in, nullptr, n_values, re, im);
    });
}

// ------------------------------------------------------------------ keys ------------------
static std::size_t key_words(const Ctx &c) { return c.L * 2 * c.K * c.N; }

int hec_kswitch_key_upload(hec_context *ctx, const uint64_t *host, hec_kswitch_key **out)
{
    return guard([&] {
        need(ctx && host && out, "null argument");
        set_device(ctx);
        auto k = make<hec_kswitch_key, hec_kswitch_key_destroy>(ctx);
        k->d = dalloc(key_words(ctx->c));
        // on the context stream, drained before the host buffer may go (a pageable hipMemcpy on the null stream is
        // not ordered with the non-blocking context stream)
        HEC_HIP(hipMemcpyAsync(k->d, host, key_words(ctx->c) * sizeof(u64), hipMemcpyHostToDevice, ctx->c.stream));
        HEC_HIP(hipStreamSynchronize(ctx->c.stream));
        *out = k.release();
    });
}
int hec_kswitch_key_download(const hec_kswitch_key *key, uint64_t *host)
{
    return guard([&] {
        need(key && host, "null argument");
        Ctx &c = live(key, BAD_RK);
        HEC_HIP(hipMemcpyAsync(host, key->d, key_words(c) * sizeof(u64), hipMemcpyDeviceToHost, c.stream));
        HEC_HIP(hipStreamSynchronize(c.stream));
    });
}
int hec_kswitch_key_fill_uniform(hec_context *ctx, uint64_t seed, hec_kswitch_key **out)
{
    return guard([&] {
        need(ctx && out, "null argument");
        set_device(ctx);
        Ctx &c = ctx->c;
        auto k = make<hec_kswitch_key, hec_kswitch_key_destroy>(ctx);
        k->d = dalloc(key_words(c));
        fill_uniform(c, k->d, (int)(c.L * 2), (int)c.K, 0, 0, seed);
        HEC_HIP(hipStreamSynchronize(c.stream));
        *out = k.release();
    });
}
int hec_kswitch_key_destroy(hec_kswitch_key *key) { return release(key); }
int hec_galois_keys_create(hec_context *ctx, hec_galois_keys **out)
{
    return guard([&] {
        need(ctx && out, "null argument");
        *out = make<hec_galois_keys, hec_galois_keys_destroy>(ctx).release();
    });
}
static void gk_check_elt(const Ctx &c, u32 elt)
{
    need((elt & 1) && elt < 2 * c.N, "Galois element is not valid");
}
int hec_galois_keys_add(hec_galois_keys *gk, uint32_t elt, const uint64_t *host)
{
    return guard([&] {
        need(gk && host, "null argument");
        Ctx &c = live(gk, BAD_GK);
        gk_check_elt(c, elt);
        HEC_HIP(hipStreamSynchronize(c.stream));  // a replaced key may still be read by enqueued work
        u64 *&d = gk->keys[elt];
        if (!d) d = dalloc(key_words(c));
        gk->drop_kw(elt);
        HEC_HIP(hipMemcpyAsync(d, host, key_words(c) * sizeof(u64), hipMemcpyHostToDevice, c.stream));
        HEC_HIP(hipStreamSynchronize(c.stream));
    });
}
int hec_galois_keys_download(const hec_galois_keys *gk, uint32_t elt, uint64_t *host)
{
    return guard([&] {
        need(gk && host, "null argument");
        Ctx &c = live(gk, BAD_GK);
        const auto it = gk->keys.find(elt);
        need(it != gk->keys.end(), "Galois key not present");
        HEC_HIP(hipMemcpyAsync(host, it->second, key_words(c) * sizeof(u64), hipMemcpyDeviceToHost, c.stream));
        HEC_HIP(hipStreamSynchronize(c.stream));
    });
}
int hec_galois_keys_add_uniform(hec_galois_keys *gk, uint32_t elt, uint64_t seed)
{
    return guard([&] {
        need(gk != nullptr, "null argument");
        Ctx &c = live(gk, BAD_GK);
        gk_check_elt(c, elt);
        HEC_HIP(hipStreamSynchronize(c.stream));
        u64 *&d = gk->keys[elt];
        if (!d) d = dalloc(key_words(c));
        gk->drop_kw(elt);
        fill_uniform(c, d, (int)(c.L * 2), (int)c.K, 0, 0, seed);
        HEC_HIP(hipStreamSynchronize(c.stream));
    });
}
int hec_galois_keys_has(const hec_galois_keys *gk, uint32_t elt) { return gk && gk->keys.count(elt) ? 1 : 0; }
int hec_galois_keys_destroy(hec_galois_keys *gk)
{
    debug_key_tables_forget(gk);
    return release(gk);
}

// ------------------------------------------------------------------ KeyGenerator / Encryptor
// DESIGN.md 4.10.  Every call derives its sub-streams on the host (64-byte seeds), uploads them, and runs the
// generator, the samplers, the noise NTTs and the fused RLWE kernel over all of its samples at once (in chunks that
// bound the workspace).  The uniform sampler's redraws are resolved once per chunk: one read-back of the count, and
// only when it is not zero the host walk over the streams' continuations and one scatter kernel.
extern "C++" {  // helpers with templates and class return types inside the C-ABI block
namespace {
using Seed = std::array<u64, 8>;

Seed master_seed(const uint64_t *seed)
{
    Seed m;
    if (seed) std::memcpy(m.data(), seed, 64);
    else if (!hec_host::entropy_seed(m.data())) throw std::logic_error("getrandom failed: no entropy for a seed");
    return m;
}
Seed sub_seed(const Seed &m, u64 call, u64 role, u64 i, u64 j)
{
    Seed o;
    hec_host::sub_seed(m.data(), call, role, i, j, o.data());
    return o;
}

// host staging of a call's asynchronous uploads: kept until the call has drained the stream
struct HostKeep {
    std::vector<std::vector<u64>> bufs;
};
u64 *upload_words(Ctx &c, Scratch &s, HostKeep &keep, std::vector<u64> words)
{
    u64 *d = s.take(std::max<std::size_t>(words.size(), 1));
    keep.bufs.push_back(std::move(words));
    const std::vector<u64> &w = keep.bufs.back();
    if (!w.empty()) HEC_HIP(hipMemcpyAsync(d, w.data(), w.size() * sizeof(u64), hipMemcpyHostToDevice, c.stream));
    return d;
}
u64 *upload_seeds(Ctx &c, Scratch &s, HostKeep &keep, const std::vector<Seed> &seeds)
{
    std::vector<u64> w(seeds.size() * 8);
    for (std::size_t i = 0; i < seeds.size(); ++i) std::memcpy(&w[i * 8], seeds[i].data(), 64);
    return upload_words(c, s, keep, std::move(w));
}
template <class T>
T **upload_ptrs(Ctx &c, Scratch &s, HostKeep &keep, const std::vector<T *> &ptrs)
{
    static_assert(sizeof(T *) == sizeof(u64), "device pointers travel as words");
    std::vector<u64> w(ptrs.size());
    for (std::size_t i = 0; i < ptrs.size(); ++i) w[i] = (u64)(uintptr_t)ptrs[i];
    return reinterpret_cast<T **>(upload_words(c, s, keep, std::move(w)));
}
u64 *fresh_words(Ctx &c, std::size_t words)  // an output buffer of a generating call
{
    u64 *d = dalloc(words);
    if (c.poison) dev_fill(c, d, 0xFFFFFFFFu, words * sizeof(u64));
    return d;
}

// SEAL's sample_poly_uniform for S streams at once: stream s draws nwords words, word g reduced mod q[g / N], into
// dst[s].  The redrawn words come from the host walk (hec_host::redraw_walk) and one scatter launch.
void sample_uniform(Ctx &c, Scratch &s, HostKeep &keep, const std::vector<Seed> &seeds, const std::vector<u64 *> &dst,
                    u64 nwords, const u64 *q, int nl, const char *cls)
{
    const std::size_t S = seeds.size(), top = s.top;
    if (!S) return;
    UniSpec spec{};
    for (int j = 0; j < nl; ++j) {
        spec.q[j] = q[j];
        spec.ratio[j] = (u64)((((u128)1) << 64) / q[j]);
        spec.maxm[j] = ~0ull - ~0ull % q[j] - 1;
    }
    // a word is redrawn with probability < q / 2^64 <= 1/8 (q < 2^61): a quarter of the words and a floor for small
    // calls is never reached
    const u64 cap64 = std::min<u64>(S * nwords / 4 + 1024, 0x7fffffffu);
    const u32 cap = (u32)cap64;
    u64 *dseed = upload_seeds(c, s, keep, seeds);
    u64 **ddst = upload_ptrs(c, s, keep, dst);
    u64 *rej = s.take(cap), *val = nullptr;
    u32 *cnt = reinterpret_cast<u32 *>(s.take(8));
    dev_zero(c, cnt, 8);
    {
        ProfScope ps(c, cls, (double)S * (double)nwords / (double)c.N);  // the words written
        prng_streams(c, dseed, ddst, (int)S, nwords, &spec, rej, cnt, cap);
    }
    u32 n = 0;
    HEC_HIP(hipMemcpyAsync(&n, cnt, sizeof(u32), hipMemcpyDeviceToHost, c.stream));
    HEC_HIP(hipStreamSynchronize(c.stream));
    if (n) {
        if (n > cap) throw std::logic_error("uniform sampler: redraw list overflow");
        std::vector<u64> pos(n), v(n);
        HEC_HIP(hipMemcpyAsync(pos.data(), rej, n * sizeof(u64), hipMemcpyDeviceToHost, c.stream));
        HEC_HIP(hipStreamSynchronize(c.stream));
        std::sort(pos.begin(), pos.end());  // (stream, position): the order the host routine meets them
        std::vector<u64> g;
        for (std::size_t a = 0; a < n;) {
            std::size_t b = a;
            const u64 st = pos[a] >> 32;
            g.clear();
            for (; b < n && pos[b] >> 32 == st; ++b) g.push_back(pos[b] & 0xffffffffull);
            hec_host::redraw_walk(seeds[st].data(), nwords, c.N, q, g.data(), g.size(), v.data() + a);
            a = b;
        }
        u64 *dpos = upload_words(c, s, keep, std::move(pos));
        val = upload_words(c, s, keep, std::move(v));
        ProfScope ps(c, "k:k_sample/redraw", 0);
        scatter_words(c, ddst, dpos, val, (int)n);
    }
    s.top = top;
}
std::size_t uniform_words(std::size_t S, u64 nwords) { return S * (nwords / 4 + 16) + 2 * (S * nwords / 4 + 1024) + 16 * 64; }

// `e` of S streams: the raw stream bytes, the centred binomial, its residues on nl primes, the forward NTTs:
// E[s][j][i], NTT form
void sample_noise(Ctx &c, Scratch &s, HostKeep &keep, const std::vector<Seed> &seeds, u64 *E, int nl)
{
    const std::size_t S = seeds.size(), top = s.top;
    if (!S) return;
    const u64 N = c.N, nwords = 6 * N / 8, stride = (nwords + 63) & ~(u64)63;
    u64 *raw = s.take(S * stride);
    std::vector<u64 *> dst(S);
    for (std::size_t i = 0; i < S; ++i) dst[i] = raw + i * stride;
    u64 *dseed = upload_seeds(c, s, keep, seeds);
    u64 **ddst = upload_ptrs(c, s, keep, dst);
    {
        ProfScope ps(c, "k:k_prng/raw", (double)S * 0.75);
        prng_streams(c, dseed, ddst, (int)S, nwords, nullptr, nullptr, nullptr, 0);
    }
    {
        ProfScope ps(c, "k:k_sample/cbd", (double)S * (0.75 + nl));
        sample_cbd(c, raw, stride, E, (int)S, nl);
    }
    int pm[HEC_MAXL + 1];
    for (int j = 0; j < nl; ++j) pm[j] = j;
    ProfScope ps(c, "k:k_ntt/keygen", 4.0 * S * nl, 2);
    ntt_strided(c, false, E, nl * N, E, nl * N, nl, pm, (int)(S * nl));
    s.top = top;
}
std::size_t noise_words(const Ctx &c, std::size_t S) { return S * (c.N + 64 + 16) + 8 * 64; }

// a ternary polynomial per stream: the uniform sampler with the modulus 3 over N words, coefficient (v mod 3) - 1,
// its residues on nl primes, NTT form: out[s][j][i].  wipe: the coefficient words are zeroed (a secret key's)
void sample_ternary(Ctx &c, Scratch &s, HostKeep &keep, const std::vector<Seed> &seeds, u64 *out, int nl, bool wipe)
{
    const std::size_t S = seeds.size(), top = s.top;
    if (!S) return;
    const u64 N = c.N, three = 3;
    u64 *T = s.take(S * N);
    std::vector<u64 *> dst(S);
    for (std::size_t i = 0; i < S; ++i) dst[i] = T + i * N;
    sample_uniform(c, s, keep, seeds, dst, N, &three, 1, "k:k_prng/ternary");
    {
        ProfScope ps(c, "k:k_sample/ternary", (double)S * (1 + nl));
        ternary_expand(c, T, out, (int)S, nl);
    }
    if (wipe) dev_zero(c, T, S * N * sizeof(u64));
    int pm[HEC_MAXL + 1];
    for (int j = 0; j < nl; ++j) pm[j] = j;
    ProfScope ps(c, "k:k_ntt/keygen", 4.0 * S * nl, 2);
    ntt_strided(c, false, out, nl * N, out, nl * N, nl, pm, (int)(S * nl));
    s.top = top;
}
std::size_t ternary_words(const Ctx &c, std::size_t S) { return S * (c.N + 64) + uniform_words(S, c.N); }

// encrypt_zero_symmetric for a batch over the primes 0 .. nl - 1: c1 = a, c0 = -(a s + NTT(e)) (+ the job's term)
struct RlweReq {
    u64 *c0, *c1;
    const u64 *add;
    u64 add_mul;
    int add_limb;
    Seed a, e;
};
std::size_t rlwe_words(const Ctx &c, std::size_t B, std::size_t nl)
{
    return B * (nl * c.N + 64 + sizeof(RlweJob) / 8 + 8) + uniform_words(B, nl * c.N) + noise_words(c, B) + 8 * 64;
}
std::size_t rlwe_chunk(const Ctx &c, std::size_t count, std::size_t nl)  // samples per pass: about 1 GiB of workspace
{
    return std::max<std::size_t>(1, std::min<std::size_t>({count, (std::size_t(1) << 27) / rlwe_words(c, 1, nl), 32767}));
}
void rlwe_batch(Ctx &c, Scratch &s, HostKeep &keep, const u64 *sk, int nl, const RlweReq *req, std::size_t B)
{
    const std::size_t top = s.top;
    const u64 N = c.N;
    std::vector<Seed> sa(B), se(B);
    std::vector<u64 *> dst(B);
    std::vector<u64> jobs(B * (sizeof(RlweJob) / 8));
    double add_limbs = 0;
    for (std::size_t b = 0; b < B; ++b) {
        sa[b] = req[b].a;
        se[b] = req[b].e;
        dst[b] = req[b].c1;
        const RlweJob j{req[b].c0, req[b].c1, req[b].add, req[b].add_mul, req[b].add_limb, 0};
        std::memcpy(&jobs[b * (sizeof(RlweJob) / 8)], &j, sizeof(RlweJob));
        add_limbs += !req[b].add ? 0 : req[b].add_limb < 0 ? nl : 1;
    }
    u64 *E = s.take(B * nl * N);
    sample_uniform(c, s, keep, sa, dst, (u64)nl * N, c.q.data(), nl, "k:k_prng/uniform");
    sample_noise(c, s, keep, se, E, nl);
    const RlweJob *djobs = reinterpret_cast<const RlweJob *>(upload_words(c, s, keep, std::move(jobs)));
    {
        ProfScope ps(c, "k:k_rlwe/sym", 4.0 * B * nl + add_limbs);  // a, s, e read, c0 written, the added term read
        rlwe_c0(c, djobs, sk, E, (int)B, nl);
    }
    s.top = top;
}

static_assert(sizeof(RlweJob) % 8 == 0, "RlweJob is uploaded as words");

// generate_one_kswitch_key for nkeys keys at once: key t's digit J is an RLWE sample over all K primes with
// (P mod q_J) newkey_t[J] added to limb J of c0; seeds sub(call, role, J, tag_t)
void kswitch_keygen(Ctx &c, const u64 *sk, const Seed &m, u64 call, u64 *const *keys, const u64 *const *newkey,
                    const u64 *tags, std::size_t nkeys, Scratch &s, HostKeep &keep)
{
    const u64 N = c.N, K = c.K, L = c.L, P = c.q[K - 1];
    std::vector<RlweReq> req;
    for (std::size_t t = 0; t < nkeys; ++t)
        for (u64 J = 0; J < L; ++J) {
            u64 *d = keys[t] + J * 2 * K * N;
            req.push_back({d, d + K * N, newkey[t], P % c.q[J], (int)J, sub_seed(m, call, 1, J, tags[t]),
                           sub_seed(m, call, 2, J, tags[t])});
        }
    const std::size_t chunk = rlwe_chunk(c, req.size(), K);
    for (std::size_t b0 = 0; b0 < req.size(); b0 += chunk)
        rlwe_batch(c, s, keep, sk, (int)K, req.data() + b0, std::min(chunk, req.size() - b0));
}
}  // namespace
}  // extern "C++"

int hec_keygen_secret(hec_context *ctx, const uint64_t seed[8], hec_secret_key **out)
{
    return guard([&] {
        need(ctx && out, "null argument");
        set_device(ctx);
        Ctx &c = ctx->c;
        const Seed m = master_seed(seed);
        auto k = make<hec_secret_key, hec_secret_key_destroy>(ctx);
        k->words = c.K * c.N;
        k->d = fresh_words(c, k->words);
        HostKeep keep;
        Scratch s(c, ternary_words(c, 1));
        sample_ternary(c, s, keep, {sub_seed(m, 1, 3, 0, 0)}, k->d, (int)c.K, true);
        HEC_HIP(hipStreamSynchronize(c.stream));
        *out = k.release();
    });
}

int hec_keygen_public(hec_context *ctx, const hec_secret_key *sk, const uint64_t seed[8], hec_public_key **out)
{
    return guard([&] {
        need(ctx && out, "null argument");
        set_device(ctx);
        check_sk(ctx, sk);
        Ctx &c = ctx->c;
        const Seed m = master_seed(seed);
        auto k = make<hec_public_key, hec_public_key_destroy>(ctx);
        k->d = fresh_words(c, 2 * c.K * c.N);
        HostKeep keep;
        Scratch s(c, rlwe_words(c, 1, c.K));
        const RlweReq r{k->d, k->d + c.K * c.N, nullptr, 0, -1, sub_seed(m, 2, 1, 0, 0), sub_seed(m, 2, 2, 0, 0)};
        rlwe_batch(c, s, keep, sk->d, (int)c.K, &r, 1);
        HEC_HIP(hipStreamSynchronize(c.stream));
        *out = k.release();
    });
}

int hec_public_key_upload(hec_context *ctx, const uint64_t *host, hec_public_key **out)
{
    return guard([&] {
        need(ctx && host && out, "null argument");
        set_device(ctx);
        Ctx &c = ctx->c;
        auto k = make<hec_public_key, hec_public_key_destroy>(ctx);
        k->d = dalloc(2 * c.K * c.N);
        HEC_HIP(hipMemcpyAsync(k->d, host, 2 * c.K * c.N * sizeof(u64), hipMemcpyHostToDevice, c.stream));
        HEC_HIP(hipStreamSynchronize(c.stream));
        *out = k.release();
    });
}
int hec_public_key_download(const hec_public_key *pk, uint64_t *host)
{
    return guard([&] {
        need(pk && host, "null argument");
        Ctx &c = live(pk, BAD_PK);
        HEC_HIP(hipMemcpyAsync(host, pk->d, 2 * c.K * c.N * sizeof(u64), hipMemcpyDeviceToHost, c.stream));
        HEC_HIP(hipStreamSynchronize(c.stream));
    });
}
int hec_public_key_destroy(hec_public_key *pk) { return release(pk); }

int hec_keygen_relin(hec_context *ctx, const hec_secret_key *sk, const uint64_t seed[8], hec_kswitch_key **out)
{
    return guard([&] {
        need(ctx && out, "null argument");
        set_device(ctx);
        check_sk(ctx, sk);
        Ctx &c = ctx->c;
        const Seed m = master_seed(seed);
        auto k = make<hec_kswitch_key, hec_kswitch_key_destroy>(ctx);
        k->d = fresh_words(c, key_words(c));
        HostKeep keep;
        const std::size_t B = rlwe_chunk(c, c.L, c.K);
        Scratch s(c, c.K * c.N + 64 + rlwe_words(c, B, c.K));
        u64 *S2 = s.take(c.K * c.N);  // newkey = s (*) s
        {
            ProfScope ps(c, "k:k_dyadic", 3.0 * c.K);
            ew_dyadic(c, sk->d, sk->d, S2, 0, (int)c.K, 1);
        }
        const u64 *nk = S2;
        const u64 tag = 0;
        kswitch_keygen(c, sk->d, m, 3, &k->d, &nk, &tag, 1, s, keep);
        dev_zero(c, S2, c.K * c.N * sizeof(u64));  // a function of the secret key
        HEC_HIP(hipStreamSynchronize(c.stream));
        *out = k.release();
    });
}

int hec_keygen_galois(hec_galois_keys *gk, const hec_secret_key *sk, const uint32_t *elts, uint64_t n,
                      const uint64_t seed[8])
{
    return guard([&] {
        need(gk && (elts || n == 0), "null argument");
        Ctx &c = live(gk, BAD_GK);
        hec_context *ctx = gk->ctx;
        check_sk(ctx, sk);
        std::vector<u32> es(elts, elts + n);
        if (n == 0) {
            es.resize(hec_default_galois_elts(ctx, nullptr));
            (void)hec_default_galois_elts(ctx, es.data());
        }
        for (u32 e : es) gk_check_elt(c, e);
        std::sort(es.begin(), es.end());
        es.erase(std::unique(es.begin(), es.end()), es.end());
        const Seed m = master_seed(seed);
        HEC_HIP(hipStreamSynchronize(c.stream));  // a replaced key may still be read by enqueued work
        const u64 N = c.N, K = c.K;
        // keys per pass: their permuted secret keys and their L digits each within the workspace bound
        const std::size_t per_key = K * N + 64 + rlwe_words(c, c.L, K);
        const std::size_t kc = std::max<std::size_t>(1, std::min<std::size_t>(es.size(), (std::size_t(1) << 27) / per_key));
        for (std::size_t e0 = 0; e0 < es.size(); e0 += kc) {
            const std::size_t cnt = std::min(kc, es.size() - e0);
            HostKeep keep;
            Scratch s(c, cnt * per_key + 64);
            u64 *G = s.take(cnt * K * N);
            std::vector<u64 *> keys(cnt);
            std::vector<const u64 *> nk(cnt);
            std::vector<u64> tags(cnt);
            for (std::size_t t = 0; t < cnt; ++t) {
                const u32 e = es[e0 + t];
                u64 *&d = gk->keys[e];
                if (!d) d = fresh_words(c, key_words(c));
                gk->drop_kw(e);
                keys[t] = d;
                nk[t] = G + t * K * N;
                tags[t] = e;
                ProfScope ps(c, "galois");
                galois_permute(c, PolyArr{sk->d, 0, 0}, PolyArr{G + t * K * N, 0, 0}, 1, 1, (int)K, e);
            }
            kswitch_keygen(c, sk->d, m, 4, keys.data(), nk.data(), tags.data(), cnt, s, keep);
            dev_zero(c, G, cnt * K * N * sizeof(u64));  // permutations of the secret key
            HEC_HIP(hipStreamSynchronize(c.stream));
        }
    });
}

int hec_encrypt_symmetric(hec_context *ctx, const hec_secret_key *sk, const hec_plaintext *const *pts, uint64_t count,
                          const uint64_t seed[8], hec_ciphertext *const *out, uint64_t *public_seeds)
{
    return guard([&] {
        need(ctx && (count == 0 || (pts && out)), "null argument");
        set_device(ctx);
        check_sk(ctx, sk);
        Ctx &c = ctx->c;
        for (u64 v = 0; v < count; ++v) check_plain(ctx, pts[v]);
        for (u64 v = 0; v < count; ++v) check_obj(ctx, out[v], BAD_CT);
        const Seed m = master_seed(seed);
        const u64 N = c.N;
        std::map<std::size_t, std::vector<u64>> groups;  // by level, as hec_decrypt groups
        for (u64 v = 0; v < count; ++v) groups[pts[v]->level].push_back(v);
        for (const auto &g : groups) {
            const std::size_t l = g.first, chunk = rlwe_chunk(c, g.second.size(), l);
            for (std::size_t b0 = 0; b0 < g.second.size(); b0 += chunk) {
                const std::size_t B = std::min(chunk, g.second.size() - b0);
                HostKeep keep;
                Scratch s(c, rlwe_words(c, B, l));
                std::vector<RlweReq> req(B);
                for (std::size_t b = 0; b < B; ++b) {
                    const u64 v = g.second[b0 + b];
                    hec_ciphertext *ct = out[v];
                    grow(ct, 2 * l * N);
                    req[b] = {ct->d, ct->d + l * N, pts[v]->d, 0, -1, sub_seed(m, 5, 1, v, 0), sub_seed(m, 5, 2, v, 0)};
                    if (public_seeds) std::memcpy(public_seeds + v * 8, req[b].a.data(), 64);
                }
                rlwe_batch(c, s, keep, sk->d, (int)l, req.data(), B);
                for (std::size_t b = 0; b < B; ++b) {
                    hec_ciphertext *ct = out[g.second[b0 + b]];
                    ct->size = 2;
                    ct->level = l;
                    ct->scale = pts[g.second[b0 + b]]->scale;
                }
                HEC_HIP(hipStreamSynchronize(c.stream));
            }
        }
    });
}

int hec_encrypt(hec_context *ctx, const hec_public_key *pk, const hec_plaintext *const *pts, uint64_t count,
                const uint64_t seed[8], hec_ciphertext *const *out)
{
    return guard([&] {
        need(ctx && (count == 0 || (pts && out)), "null argument");
        set_device(ctx);
        check_pk(ctx, pk);
        Ctx &c = ctx->c;
        for (u64 v = 0; v < count; ++v) check_plain(ctx, pts[v]);
        for (u64 v = 0; v < count; ++v) check_obj(ctx, out[v], BAD_CT);
        const Seed m = master_seed(seed);
        const u64 N = c.N, K = c.K;
        std::map<std::size_t, std::vector<u64>> groups;
        for (u64 v = 0; v < count; ++v) groups[pts[v]->level].push_back(v);
        for (const auto &g : groups) {
            const std::size_t l = g.first, nl = l + 1;  // the level above: primes 0 .. l (l = L: prime l is P)
            const std::size_t per = N * (nl + 2 * nl + 2 + 4 * l) + 8 * 64 + ternary_words(c, 1) + noise_words(c, 2);
            const std::size_t chunk = std::max<std::size_t>(
                1, std::min<std::size_t>({g.second.size(), (std::size_t(1) << 27) / per, 16383}));
            const std::vector<u64> &inv = l < c.L ? c.ql_inv[l + 1] : c.p_inv;
            const std::vector<u64> &inv_q = l < c.L ? c.ql_inv_q[l + 1] : c.p_inv_q;
            for (std::size_t b0 = 0; b0 < g.second.size(); b0 += chunk) {
                const std::size_t B = std::min(chunk, g.second.size() - b0);
                HostKeep keep;
                Scratch s(c, B * per + 16 * 64);
                u64 *U = s.take(B * nl * N), *E = s.take(B * 2 * nl * N), *Y = s.take(B * 2 * N);
                u64 *Z = s.take(B * 2 * l * N), *O = s.take(B * 2 * l * N);
                std::vector<Seed> su(B), se(2 * B);
                std::vector<u64 *> cts(B);
                std::vector<const u64 *> pp(B);
                for (std::size_t b = 0; b < B; ++b) {
                    const u64 v = g.second[b0 + b];
                    su[b] = sub_seed(m, 6, 3, v, 0);
                    se[2 * b] = sub_seed(m, 6, 2, v, 0);
                    se[2 * b + 1] = sub_seed(m, 6, 2, v, 1);
                    grow(out[v], 2 * l * N);
                    cts[b] = out[v]->d;
                    pp[b] = pts[v]->d;
                }
                sample_ternary(c, s, keep, su, U, (int)nl, true);
                sample_noise(c, s, keep, se, E, (int)nl);
                {  // u, both key polys and both noise polys read, both t_j written
                    ProfScope ps(c, "k:k_rlwe/pk", 7.0 * B * nl);
                    rlwe_pk(c, U, pk->d, K * N, E, (int)B, (int)nl);
                }
                {  // the last limbs' INTT (in, out), then X read, the rounding limbs written and read, OUT written
                    ProfScope ps(c, "k:k_ntt/enc_divround", 2.0 * B * (2 + 4 * l), 4);
                    const int pm[1] = {(int)l};
                    for (int k = 0; k < 2; ++k)
                        ntt_strided(c, true, E + k * nl * N + l * N, 2 * nl * N, Y + k * N, 2 * N, 1, pm, (int)B);
                    divide_round(c, Y, 2 * N, N, PolyArr{E, 2 * nl * N, nl * N}, PolyArr{}, 0,
                                 PolyArr{O, 2 * l * N, l * N}, (int)B, 2, (int)l, (int)l, inv.data(), inv_q.data(), Z);
                }
                u64 **dct = upload_ptrs(c, s, keep, cts);
                const u64 **dpt = upload_ptrs(c, s, keep, pp);
                {
                    ProfScope ps(c, "k:k_rlwe/store", 5.0 * B * l);
                    ct_store(c, O, dct, dpt, (int)B, (int)l);
                }
                dev_zero(c, U, B * nl * N * sizeof(u64));  // the encryption randomness
                for (std::size_t b = 0; b < B; ++b) {
                    hec_ciphertext *ct = out[g.second[b0 + b]];
                    ct->size = 2;
                    ct->level = l;
                    ct->scale = pts[g.second[b0 + b]]->scale;
                }
                HEC_HIP(hipStreamSynchronize(c.stream));
            }
        }
    });
}

// ------------------------------------------------------------------ evaluator -------------
// ---------------------------------------------------------------- SEAL wire format on device objects
namespace {
void seal_rc(int rc)
{
    if (rc == HEC_EINVAL) throw std::invalid_argument(hec_seal_last_error());
    if (rc != HEC_OK) throw std::logic_error(hec_seal_last_error());
}
}  // namespace

int hec_ciphertext_load_seal(hec_ciphertext *ct, const void *bytes, uint64_t nbytes, uint64_t *consumed)
{
    return guard([&] {
        need(ct && bytes, "null argument");
        const Ctx &c = live(ct, BAD_CT);
        uint64_t size = 0, level = 0, N = 0, pid[4], used = 0;
        double scale = 0;
        // the context's data-level primes expand a seeded object (client.cpp:113-114 sends those)
        seal_rc(hec_seal_ciphertext_load_ex(bytes, nbytes, c.q.data(), c.L, &size, &level, &N, &scale, pid, nullptr, 0,
                                            &used));
        // Ciphertext::load(context, ...): the data must be valid for the context (is_valid_for)
        need(N == c.N && level >= 1 && level <= c.L && size >= 2, "ciphertext data is invalid");
        uint64_t want[4];
        seal_rc(hec_seal_parms_id(c.N, c.q.data(), level, want));
        need(std::memcmp(want, pid, 32) == 0, "ciphertext data is invalid");
        std::vector<u64> host(size * level * N);
        seal_rc(hec_seal_ciphertext_load_ex(bytes, nbytes, c.q.data(), c.L, nullptr, nullptr, nullptr, nullptr, nullptr,
                                            host.data(), host.size(), nullptr));
        const int rc = hec_ciphertext_upload(ct, host.data(), size, level, scale);
        if (rc != HEC_OK) throw std::logic_error(hec_last_error());
        if (consumed) *consumed = used;
    });
}

int hec_ciphertext_save_seal(const hec_ciphertext *ct, int compr_mode, void *out, uint64_t cap, uint64_t *written)
{
    return guard([&] {
        need(ct && ct->d, "null argument");
        const Ctx &c = live(ct, BAD_CT);
        std::vector<u64> host(ct->size * ct->level * c.N);
        const int rc = hec_ciphertext_download(ct, host.data());
        if (rc != HEC_OK) throw std::logic_error(hec_last_error());
        seal_rc(hec_seal_ciphertext_save(host.data(), ct->size, ct->level, c.N, ct->scale, c.q.data(), compr_mode, out,
                                         cap, written));
    });
}

// Decompressed-size limit of a KSwitchKeys object loaded into this context (the bytes come from a client socket,
// server.cpp:110-122): `lists` key lists of L PublicKeys of u64[2][K][N], the object's N list-length words, and at
// most 256 B of SEALHeader / parms_id / ciphertext metadata per PublicKey.  The loader inflates the whole object into
// host memory before parsing it, so the default number of non-empty GaloisKeys lists is a fixed cap that does not
// depend on the device: four times SEAL's default set (create_galois_keys(), the reference's only form:
// matrix_operations.cpp:771,872,1064, holds 2 log2(N) - 1 lists), at least 64, at most N, and no more than half of the
// host's available physical memory can hold.  The same bound applies whether the object is compressed (the inflate
// budget) or not (counted as the lists are parsed).  hec_galois_keys_load_seal_ex takes an explicit limit instead.
static uint64_t galois_lists_default(const Ctx &c)
{
    const uint64_t logn = (uint64_t)__builtin_ctzll(c.N);
    uint64_t lists = std::min<uint64_t>(c.N, std::max<uint64_t>(64, 4 * (2 * logn - 1)));
    const long pages = sysconf(_SC_AVPHYS_PAGES), psz = sysconf(_SC_PAGESIZE);
    if (pages > 0 && psz > 0) {
        const uint64_t per = c.L * (2 * c.K * c.N * 8 + 256);
        lists = std::min<uint64_t>(lists, std::max<uint64_t>(1, (uint64_t)pages * (uint64_t)psz / 2 / per));
    }
    return lists;
}
static uint64_t seal_keys_max_bytes(const Ctx &c, uint64_t lists)
{
    return lists * c.L * (2 * c.K * c.N * 8 + 256) + c.N * 8 + 4096;
}

int hec_kswitch_key_load_seal(hec_context *ctx, const void *bytes, uint64_t nbytes, hec_kswitch_key **out,
                              uint64_t *consumed)
{
    return guard([&] {
        need(ctx && bytes && out, "null argument");
        const Ctx &c = ctx->c;
        uint64_t words = 0, used = 0, lists = 0;
        const uint64_t cap = seal_keys_max_bytes(c, 1);
        seal_rc(hec_seal_kswitch_keys_load_ex(bytes, nbytes, 0, cap, &lists, nullptr, 0, &words, &used));
        need(lists >= 1 && words == c.L * 2 * c.K * c.N, "relin_keys is not valid for encryption parameters");
        std::vector<u64> host(words);
        seal_rc(hec_seal_kswitch_keys_load_ex(bytes, nbytes, 0, cap, nullptr, host.data(), words, nullptr, nullptr));
        const int rc = hec_kswitch_key_upload(ctx, host.data(), out);
        if (rc != HEC_OK) throw std::logic_error(hec_last_error());
        if (consumed) *consumed = used;
    });
}

int hec_galois_keys_load_seal_ex(hec_galois_keys *gk, const void *bytes, uint64_t nbytes, uint64_t max_lists,
                                 uint64_t *consumed)
{
    return guard([&] {
        need(gk && bytes, "null argument");
        const Ctx &c = live(gk, BAD_GK);
        struct Visit {
            hec_galois_keys *gk;
            const Ctx &c;
            uint64_t max_lists, seen = 0;
            std::string err;
            int rc = HEC_OK;
        } v{gk, c, max_lists ? std::min<uint64_t>(max_lists, c.N) : galois_lists_default(c)};
        // one pass over the object: GaloisKeys::get_index(elt) = (elt - 1) / 2, every non-empty list uploaded as it
        // is parsed
        auto cb = [](void *user, uint64_t index, const uint64_t *words, uint64_t nwords) -> int {
            auto *st = static_cast<Visit *>(user);
            const Ctx &c = st->c;
            if (nwords != c.L * 2 * c.K * c.N) {
                st->err = "galois_keys is not valid for encryption parameters";
                return st->rc = HEC_EINVAL;
            }
            if (++st->seen > st->max_lists) {  // the uncompressed object's form of the inflate budget below
                st->err = "decompressed SEAL object exceeds the size limit";
                return st->rc = HEC_EINVAL;
            }
            const int rc = hec_galois_keys_add(st->gk, (uint32_t)(2 * index + 1), words);
            if (rc != HEC_OK) st->err = hec_last_error();
            return st->rc = rc;
        };
        uint64_t used = 0;
        const int rc = hec_seal_kswitch_keys_foreach_ex(bytes, nbytes, seal_keys_max_bytes(c, v.max_lists),
                                                        cb, &v, nullptr, &used);
        if (v.rc != HEC_OK) {
            if (v.rc == HEC_EINVAL) throw std::invalid_argument(v.err);
            throw std::logic_error(v.err);
        }
        seal_rc(rc);
        if (consumed) *consumed = used;
    });
}

int hec_galois_keys_load_seal(hec_galois_keys *gk, const void *bytes, uint64_t nbytes, uint64_t *consumed)
{
    return hec_galois_keys_load_seal_ex(gk, bytes, nbytes, 0, consumed);
}

uint64_t hec_galois_keys_load_seal_default_lists(const hec_context *ctx)
{
    return ctx ? galois_lists_default(ctx->c) : 0;
}

int hec_negate_inplace(hec_context *ctx, hec_ciphertext *a)
{
    return guard([&] {
        check_ct(ctx, a);
        set_device(ctx);
        ew_negate(ctx->c, PolyArr{a->d, 0, a->level * ctx->c.N}, 1, (int)a->size, (int)a->level);
    });
}

static void add_sub(hec_context *ctx, hec_ciphertext *a, const hec_ciphertext *b, bool sub)
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
int hec_add_inplace(hec_context *ctx, hec_ciphertext *a, const hec_ciphertext *b)
{
    return guard([&] { add_sub(ctx, a, b, false); });
}
int hec_sub_inplace(hec_context *ctx, hec_ciphertext *a, const hec_ciphertext *b)
{
    return guard([&] { add_sub(ctx, a, b, true); });
}

static void plain_addsub(hec_context *ctx, hec_ciphertext *a, const hec_plaintext *p, bool sub)
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

static void multiply(hec_context *ctx, hec_ciphertext *a, const hec_ciphertext *b)
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

static void galois_single(hec_context *ctx, hec_ciphertext *a, const std::vector<u32> &elts, const hec_galois_keys *gk)
{
    Ctx &c = ctx->c;
    const std::size_t l = a->level, N = c.N;
    Scratch s(c, ks_words(c, 1, l) + 2 * l * N + 128);
    const PolyArr x{a->d, 0, l * N};
    for (u32 e : elts) galois_ks(c, s, x, x, 1, (int)l, e, gk->keys.at(e));
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

// ------------------------------------------------------------------ he::linalg ------------
int hec_matmul_diag_col(hec_context *ctx, const hec_ciphertext *const *diags, uint64_t n,
                        const hec_ciphertext *const *cols, uint64_t p, const hec_kswitch_key *rk,
                        const hec_galois_keys *gk, hec_ciphertext *const *out)
{
    return guard([&] {
        set_device(ctx);
        need(diags && cols && out, "null argument");
        std::vector<std::size_t> js(n);
        for (std::size_t j = 0; j < n; ++j) js[j] = j;
        matvec_lanes(ctx, diags, nullptr, n, js, cols, p, rk, gk, true, out);
    });
}

int hec_matmul_diag_col_partial(hec_context *ctx, const hec_ciphertext *const *diags, uint64_t n, uint64_t j_begin,
                                uint64_t j_end, const hec_ciphertext *const *cols, uint64_t p,
                                const hec_galois_keys *gk, hec_ciphertext *const *acc_out)
{
    return guard([&] {
        set_device(ctx);
        need(diags && cols && acc_out, "null argument");
        need(j_begin < j_end && j_end <= n, "empty matrix operand");
        std::vector<std::size_t> js;
        for (uint64_t j = j_begin; j < j_end; ++j) js.push_back(j);
        matvec_lanes(ctx, diags, nullptr, n, js, cols, p, nullptr, gk, false, acc_out);
    });
}

int hec_matmul_diag_col_partial_set(hec_context *ctx, const hec_ciphertext *const *diags, uint64_t n,
                                    const uint64_t *j_idx, uint64_t nj, const hec_ciphertext *const *cols, uint64_t p,
                                    const hec_galois_keys *gk, hec_ciphertext *const *acc_out)
{
    return guard([&] {
        set_device(ctx);
        need(diags && cols && acc_out && j_idx, "null argument");
        std::vector<std::size_t> js(j_idx, j_idx + nj);
        std::sort(js.begin(), js.end());
        need(std::adjacent_find(js.begin(), js.end()) == js.end(), "duplicate diagonal index");
        matvec_lanes(ctx, diags, nullptr, n, js, cols, p, nullptr, gk, false, acc_out);
    });
}

int hec_matmul_diagpt_col(hec_context *ctx, const hec_plaintext *const *diags, uint64_t n,
                          const hec_ciphertext *const *cols, uint64_t p, const hec_galois_keys *gk,
                          hec_ciphertext *const *out)
{
    return guard([&] {
        set_device(ctx);
        need(diags && cols && out, "null argument");
        std::vector<std::size_t> js(n);
        for (std::size_t j = 0; j < n; ++j) js[j] = j;
        matvec_lanes(ctx, nullptr, diags, n, js, cols, p, nullptr, gk, true, out);
    });
}

int hec_bsgs_plan(uint64_t n, uint64_t bs, int *steps, uint64_t cap, uint64_t *count, uint64_t *bs_eff)
{
    return guard([&] {
        need(count != nullptr && (steps != nullptr || cap == 0), "null argument");
        const BsgsPlan plan = bsgs_plan(n, bs);
        *count = plan.steps.size();
        if (bs_eff) *bs_eff = plan.bs;
        for (std::size_t i = 0; i < plan.steps.size() && i < cap; ++i) steps[i] = plan.steps[i];
    });
}

int hec_matmul_diagpt_col_bsgs(hec_context *ctx, const hec_plaintext *const *pdiags, uint64_t n, uint64_t bs,
                               const hec_ciphertext *const *cols, uint64_t p, const hec_galois_keys *gk,
                               hec_ciphertext *const *out)
{
    return guard([&] {
        set_device(ctx);
        need(pdiags && cols && out, "null argument");
        bsgs_core(ctx, nullptr, pdiags, n, bsgs_plan(n, bs), cols, p, /*rk*/ nullptr, gk, out);
    });
}

int hec_matmul_diag_col_bsgs(hec_context *ctx, const hec_ciphertext *const *diags, uint64_t n, uint64_t bs,
                             const hec_ciphertext *const *cols, uint64_t p, const hec_kswitch_key *rk,
                             const hec_galois_keys *gk, hec_ciphertext *const *out)
{
    return guard([&] {
        set_device(ctx);
        need(diags && cols && out, "null argument");
        bsgs_core(ctx, diags, nullptr, n, bsgs_plan(n, bs), cols, p, rk, gk, out);
    });
}

int hec_colcolT_bsgs_plan(uint64_t p, uint64_t bs, int form, int *steps, uint64_t cap, uint64_t *count,
                          uint64_t *bs_eff)
{
    return guard([&] {
        need(count != nullptr && (steps != nullptr || cap == 0), "null argument");
        const CctPlan plan = colcolt_plan(p, bs, form);
        *count = plan.steps.size();
        if (bs_eff) *bs_eff = plan.bs;
        for (std::size_t i = 0; i < plan.steps.size() && i < cap; ++i) steps[i] = plan.steps[i];
    });
}

int hec_matmul_col_colT_bsgs(hec_context *ctx, const hec_ciphertext *const *A, uint64_t n,
                             const hec_ciphertext *const *B, uint64_t p, uint64_t bs, int form,
                             const hec_kswitch_key *rk, const hec_galois_keys *gk, hec_ciphertext *const *out)
{
    return guard([&] {
        set_device(ctx);
        colcolt_bsgs(ctx, A, n, B, p, bs, form, rk, gk, out);
    });
}

int hec_matmul_finish(hec_context *ctx, hec_ciphertext *const *acc, uint64_t p, const hec_kswitch_key *rk,
                      hec_ciphertext *const *out)
{
    return guard([&] {
        set_device(ctx);
        need(acc && out && p >= 1, "null argument");
        check_obj(ctx, rk, BAD_RK);
        Ctx &c = ctx->c;
        const std::size_t l = acc[0]->level, N = c.N, S3 = 3 * l * N, So = 2 * (l - 1) * N;
        for (uint64_t i = 0; i < p; ++i) {
            check_ct(ctx, acc[i]);
            need(acc[i]->size == 3 && acc[i]->level == l, "encrypted1 and encrypted2 parameter mismatch");
        }
        if (l < 2) throw std::invalid_argument("end of modulus switching chain reached");
        Scratch s(c, p * (S3 + So) + ks_words(c, p, l) + rescale_words(c, p, 2, l) + 256);
        u64 *A3 = s.take(p * S3), *O = s.take(p * So);
        for (uint64_t i = 0; i < p; ++i) d2d(c, A3 + i * S3, acc[i]->d, S3);
        relin_rescale(c, s, A3, rk->d, (int)p, (int)l, PolyArr{O, So, (l - 1) * N});
        std::vector<double> sc(p);  // out[i] may be an acc[j]: every scale is read before the first store
        for (uint64_t i = 0; i < p; ++i) sc[i] = acc[i]->scale / (double)c.q[l - 1];
        for (uint64_t i = 0; i < p; ++i) store_ct(c, out[i], O + i * So, 2, l - 1, sc[i]);
    });
}

// ------------------------------------------------------------------ multi-GPU

int hec_plan_diagonal_shards(uint64_t N, uint64_t n, int world, const uint32_t *key_elts, uint64_t nkeys,
                             int32_t *rank_of_diag)
{
    return guard([&] {
        need(rank_of_diag && (key_elts || nkeys == 0), "null argument");
        need(N >= 1024 && N <= 65536 && !(N & (N - 1)), "poly_modulus_degree must be a power of two in [2^10, 2^16]");
        std::set<u32> keys(key_elts, key_elts + nkeys);
        const auto plan = plan_shards(N, n, world, keys);
        for (std::size_t r = 0; r < plan.size(); ++r)
            for (std::size_t j : plan[r]) rank_of_diag[j] = (int32_t)r;
    });
}

int hec_comm_unique_id(void *unique_id)
{
    return guard([&] {
        need(unique_id != nullptr, "null argument");
        ncclUniqueId id;
        nccl_check(rccl().get_unique_id(&id), "ncclGetUniqueId");
        std::memcpy(unique_id, &id, sizeof(id));
    });
}

int hec_comm_init(hec_context *ctx, int rank, int world, const void *unique_id)
{
    return guard([&] {
        set_device(ctx);
        need(world >= 1 && rank >= 0 && rank < world, "invalid rank / world");
        // the exchange adds `world` canonical residues < 2^60 in u64 (hec_matmul_diag_col_sharded); shard.py's
        // int64 exchange has the same bound
        need(world <= 8, "world must be at most 8 (exact u64 partial-sum exchange)");
        need(ctx->comm == nullptr, "communicator already initialised");
        if (world > 1 || unique_id) {  // world 1 with an id: a one-rank communicator (exercises the RCCL path)
            need(unique_id != nullptr, "null argument");
            ncclUniqueId id;
            std::memcpy(&id, unique_id, sizeof(id));
            ncclComm_t comm = nullptr;
            nccl_check(rccl().init_rank(&comm, world, id, rank), "ncclCommInitRank");
            ctx->comm = new RcclComm(comm);
        }
        ctx->rank = rank;
        ctx->world = world;
    });
}

int hec_comm_init_ops(hec_context *ctx, int rank, int world, const hec_comm_ops *ops)
{
    return guard([&] {
        set_device(ctx);
        need(world >= 1 && rank >= 0 && rank < world, "invalid rank / world");
        need(world <= 8, "world must be at most 8 (exact u64 partial-sum exchange)");
        need(ctx->comm == nullptr, "communicator already initialised");
        need(ops && ops->allreduce_f64 && ops->allreduce_u64_sum, "null argument");
        ctx->comm = new OpsComm(*ops);
        ctx->rank = rank;
        ctx->world = world;
    });
}

int hec_shard_agree(const hec_comm_ops *ops, int rank, int status, const char *reason, const double *scales,
                    uint64_t p, char *msg, uint64_t msg_cap)
{
    int agreed = HEC_OK;
    const int rc = guard([&] {
        need(ops && ops->allreduce_f64 && ops->allreduce_u64_sum && (p == 0 || scales || status), "null argument");
        need(status == HEC_OK || status == HEC_EINVAL || status == HEC_ELOGIC, "status must be HEC_OK / EINVAL / ELOGIC");
        need(rank >= 0 && rank < 255, "invalid rank / world");
        OpsComm cm(*ops);
        std::string m = reason ? reason : "";
        agreed = shard_agree(cm, rank, status, m, scales, p, nullptr);
        if (msg && msg_cap) {
            const std::size_t k = std::min<std::size_t>(m.size(), msg_cap - 1);
            std::memcpy(msg, m.data(), k);
            msg[k] = 0;
        }
    });
    return rc != HEC_OK ? rc : agreed;
}

int hec_context_comm(const hec_context *ctx, int *rank, int *world)
{
    if (!ctx) return HEC_EINVAL;
    if (rank) *rank = ctx->rank;
    if (world) *world = ctx->world;
    return ctx->comm ? 1 : 0;
}

int hec_matmul_diag_col_sharded(hec_context *ctx, const hec_ciphertext *const *diags, uint64_t n,
                                const hec_ciphertext *const *cols, uint64_t p, const hec_kswitch_key *rk,
                                const hec_galois_keys *gk, hec_ciphertext *const *out)
{
    return guard([&] {
        set_device(ctx);
        need(ctx->world == 1 || ctx->comm, "hec_comm_init has not been called");
        Ctx &c = ctx->c;
        // The argument checks run on this rank's planned diagonals only (the others are never dereferenced), then
        // the ranks agree on them before any data-path collective, so a bad argument on one rank is an error on
        // every rank instead of a rank left waiting in the exchange.  The product scales of the ranks' diagonals
        // are compared across ranks too (SEAL's add_inplace "scale mismatch" over the whole sum).
        std::vector<std::size_t> mine;
        std::vector<double> ps;
        int status = HEC_OK;
        std::string msg;
        try {
            need(diags && cols && out && n >= 1 && p >= 1, "empty matrix operand");
            check_obj(ctx, gk, BAD_GK);
            std::set<u32> keys;
            for (const auto &kv : gk->keys) keys.insert(kv.first);
            mine = plan_shards(c.N, n, ctx->world, keys)[ctx->rank];
            ps = matvec_check(ctx, diags, nullptr, n, mine, cols, p, rk, gk, true);
        } catch (const std::invalid_argument &e) {
            status = HEC_EINVAL; msg = e.what();
        } catch (const std::logic_error &e) {
            status = HEC_ELOGIC; msg = e.what();
        }
        if (ctx->comm) status = shard_agree(*ctx->comm, ctx->rank, status, msg, ps.data(), p, c.stream);
        if (status == HEC_EINVAL) throw std::invalid_argument(msg);
        if (status) throw std::logic_error(msg);
        const std::size_t l = cols[0]->level, S3 = 3 * l * c.N;
        // this rank's size-3 partials over its trie subtrees of diagonals
        std::vector<hec_ciphertext> acc(p);
        std::vector<hec_ciphertext *> accp(p);
        for (uint64_t i = 0; i < p; ++i) { bind(acc[i], ctx); accp[i] = &acc[i]; }
        struct Free {
            std::vector<hec_ciphertext> &a;
            ~Free() { for (auto &x : a) if (x.d) (void)hipFree(x.d); }
        } free_acc{acc};
        matvec_lanes(ctx, diags, nullptr, n, mine, cols, p, nullptr, gk, false, accp.data());
        if (ctx->comm) {
            // the one exchange: a plain u64 sum of the world's canonical residues (< world 2^60 < 2^64), then
            // reduce mod q; every rank then holds the full accumulators (he_linalg.cpp:977-997 summed)
            u64 *buf = nullptr;
            HEC_HIP(hipMallocAsync((void **)&buf, p * S3 * sizeof(u64), c.stream));
            for (uint64_t i = 0; i < p; ++i) d2d(c, buf + i * S3, acc[i].d, S3);
            ctx->comm->allreduce_u64_sum(buf, p * S3, c.stream);
            ew_reduce(c, buf, (int)(3 * p), (int)l);
            for (uint64_t i = 0; i < p; ++i) d2d(c, acc[i].d, buf + i * S3, S3);
            HEC_HIP(hipFreeAsync(buf, c.stream));
        }
        // lazy relinearize + rescale (he_linalg.cpp:999-1002) of every output on every rank: p key switches
        // against the ~n/world rotations each rank ran, and no second collective
        const int rc = hec_matmul_finish(ctx, accp.data(), p, rk, out);
        if (rc != HEC_OK) throw std::logic_error(hec_last_error());
    });
}

int hec_matmul_col_colT(hec_context *ctx, const hec_ciphertext *const *A, uint64_t n, const hec_ciphertext *const *B,
                        uint64_t p, const hec_kswitch_key *rk, const hec_galois_keys *gk,
                        hec_ciphertext *const *out)
{
    return guard([&] {
        set_device(ctx);
        need(A && B && out && n >= 1 && p >= 1, "null argument");
        check_obj(ctx, rk, "keys are not valid for encryption parameters");
        check_obj(ctx, gk, "keys are not valid for encryption parameters");
        Ctx &c = ctx->c;
        const std::size_t l = A[0]->level, N = c.N, S2 = 2 * l * N, S3 = 3 * l * N, So = 2 * (l - 1) * N;
        for (uint64_t j = 0; j < n; ++j) {
            check_ct(ctx, A[j]);
            check_ct(ctx, B[j]);
            need(A[j]->size == 2 && B[j]->size == 2, "encrypted size must be 2");
            need(A[j]->level == l && B[j]->level == l, "encrypted1 and encrypted2 parameter mismatch");
        }
        double sc = 0;
        for (uint64_t j = 0; j < n; ++j) {
            const double s = B[j]->scale * A[j]->scale;
            need(scale_ok(c, s, l), "scale out of bounds");
            if (j == 0) sc = s;
            else need(are_close(sc, s), "scale mismatch");
        }
        if (l < 2) throw std::invalid_argument("end of modulus switching chain reached");
        RotTrie trie;  // rotations rot(B[j], i) for all j share the trie over i
        {
            std::vector<u32> seq;
            for (uint64_t i = 0; i < p; ++i) {
                seq.clear();
                rotation_elts(c, (int)i, *gk, seq);
                trie.insert(seq, i);
            }
        }
        const int D = trie.depth;
        Scratch s(c, n * S2 * (D + 2) + p * (S3 + So) + ks_words(c, std::max<uint64_t>(n, p), l) + 2 * n * l * N +
                         rescale_words(c, p, 2, l) + (D + 80) * 64);
        TrieBufs bufs(s, D, 1, n * S2);
        u64 *Aw = s.take(n * S2), *AC = s.take(p * S3), *O = s.take(p * So);
        for (uint64_t j = 0; j < n; ++j) {
            d2d(c, Aw + j * S2, A[j]->d, S2);
            d2d(c, bufs.b[0][0] + j * S2, B[j]->d, S2);
        }
        const PolyArr Ba{bufs.b[0][0], S2, l * N}, Aa{Aw, S2, l * N};
        auto visit = [&](std::size_t i, PolyArr src) {  // out[i] = sum_j rot(B[j], i) (x) A[j]
            tensor_sum(c, src, Aa, AC + i * S3, l * N, (int)n, (int)l);
        };
        auto no_flush = [](const u64 *) {};
        walk_trie(c, s, trie, 0, Ba, 0, (int)n, (int)l, *gk, bufs, S2, visit, no_flush);
        relin_rescale(c, s, AC, rk->d, (int)p, (int)l, PolyArr{O, So, (l - 1) * N});
        for (uint64_t i = 0; i < p; ++i) store_ct(c, out[i], O + i * So, 2, l - 1, sc / (double)c.q[l - 1]);
    });
}

int hec_matrix_matmul(hec_context *ctx, const hec_ciphertext *const *A, uint64_t ar, uint64_t ac, int atr,
                      const hec_ciphertext *const *B, uint64_t br, uint64_t bc, int btr, const hec_kswitch_key *rk,
                      hec_ciphertext *const *out)
{
    return guard([&] {
        set_device(ctx);
        need(A && B && out, "null argument");
        check_obj(ctx, rk, BAD_RK);
        Ctx &c = ctx->c;
        // Matrix::get_dims / ij_to_idx (he_linalg.cpp:25-28, 376-379)
        const uint64_t r1 = atr ? ac : ar, c1 = atr ? ar : ac, r2 = btr ? bc : br, c2 = btr ? br : bc;
        need(c1 == r2, "dimension mismatch");
        auto at = [](const hec_ciphertext *const *M, uint64_t rows, int tr, uint64_t i, uint64_t j) {
            return M[(tr ? j : i) + rows * (tr ? i : j)];
        };
        const std::size_t l = A[0]->level, N = c.N, S3 = 3 * l * N, So = 2 * (l - 1) * N;
        for (uint64_t k = 0; k < ar * ac; ++k) {
            check_ct(ctx, A[k]);
            need(A[k]->size == 2 && A[k]->level == l, "encrypted1 and encrypted2 parameter mismatch");
        }
        for (uint64_t k = 0; k < br * bc; ++k) {
            check_ct(ctx, B[k]);
            need(B[k]->size == 2 && B[k]->level == l, "encrypted1 and encrypted2 parameter mismatch");
        }
        if (l < 2) throw std::invalid_argument("end of modulus switching chain reached");
        const uint64_t no = r1 * c2;
        std::vector<double> sc(no);
        for (uint64_t j = 0; j < c2; ++j)
            for (uint64_t i = 0; i < r1; ++i)
                for (uint64_t k = 0; k < c1; ++k) {
                    const double s = at(A, ar, atr, i, k)->scale * at(B, br, btr, k, j)->scale;
                    need(scale_ok(c, s, l), "scale out of bounds");
                    if (k == 0) sc[i + r1 * j] = s;
                    else need(are_close(sc[i + r1 * j], s), "scale mismatch");
                }
        Scratch s(c, no * (S3 + So) + S3 + ks_words(c, no, l) + rescale_words(c, no, 2, l) + 512);
        u64 *AC = s.take(no * S3), *T = s.take(S3), *O = s.take(no * So);
        const PolyArr one{nullptr, 0, l * N};
        for (uint64_t j = 0; j < c2; ++j)
            for (uint64_t i = 0; i < r1; ++i) {  // he_linalg.cpp:218-228
                u64 *dst = AC + (i + r1 * j) * S3;
                for (uint64_t k = 0; k < c1; ++k) {
                    const hec_ciphertext *x = at(A, ar, atr, i, k), *y = at(B, br, btr, k, j);
                    ct_multiply(c, x->d, 2, y->d, 2, k == 0 ? dst : T, (int)l);
                    if (k) ew_add(c, PolyArr{dst, 0, l * N}, PolyArr{T, 0, l * N}, PolyArr{dst, 0, l * N}, 1, 3,
                                  (int)l, 0);
                }
            }
        (void)one;
        relin_rescale(c, s, AC, rk->d, (int)no, (int)l, PolyArr{O, So, (l - 1) * N});
        for (uint64_t o = 0; o < no; ++o) store_ct(c, out[o], O + o * So, 2, l - 1, sc[o] / (double)c.q[l - 1]);
    });
}

// ------------------------------------------------------------------ primitives ------------
int hec_ntt_forward(hec_context *ctx, uint64_t *d, uint64_t limb0, uint64_t nl, uint64_t np)
{
    return guard([&] {
        set_device(ctx);
        need(d && nl >= 1 && limb0 + nl <= ctx->c.K && nl <= HEC_MAXL + 1, "invalid limb range");
        int pm[HEC_MAXL + 1];
        for (uint64_t i = 0; i < nl; ++i) pm[i] = (int)(limb0 + i);
        // one scope per pass: each reads and writes every limb once (SURVEY 8(d)'s 2 N 8 B per limb-NTT)
        {
            ProfScope k(ctx->c, "k:k_ntt/fwd_a", 2.0 * nl * np);
            ntt_strided(ctx->c, false, d, nl * ctx->c.N, d, nl * ctx->c.N, (int)nl, pm, (int)(nl * np), 1, 1);
        }
        ProfScope k(ctx->c, "k:k_ntt/fwd_b", 2.0 * nl * np);
        ntt_strided(ctx->c, false, d, nl * ctx->c.N, d, nl * ctx->c.N, (int)nl, pm, (int)(nl * np), 1, 2);
    });
}
int hec_ntt_inverse(hec_context *ctx, uint64_t *d, uint64_t limb0, uint64_t nl, uint64_t np)
{
    return guard([&] {
        set_device(ctx);
        need(d && nl >= 1 && limb0 + nl <= ctx->c.K && nl <= HEC_MAXL + 1, "invalid limb range");
        int pm[HEC_MAXL + 1];
        for (uint64_t i = 0; i < nl; ++i) pm[i] = (int)(limb0 + i);
        {
            ProfScope k(ctx->c, "k:k_ntt/inv_b", 2.0 * nl * np);
            ntt_strided(ctx->c, true, d, nl * ctx->c.N, d, nl * ctx->c.N, (int)nl, pm, (int)(nl * np), 1, 1);
        }
        ProfScope k(ctx->c, "k:k_ntt/inv_a", 2.0 * nl * np);
        ntt_strided(ctx->c, true, d, nl * ctx->c.N, d, nl * ctx->c.N, (int)nl, pm, (int)(nl * np), 1, 2);
    });
}
int hec_dyadic_multiply(hec_context *ctx, const uint64_t *a, const uint64_t *b, uint64_t *out, uint64_t limb0,
                        uint64_t nl, uint64_t np)
{
    return guard([&] {
        set_device(ctx);
        need(a && b && out && limb0 + nl <= ctx->c.K, "invalid limb range");
        ProfScope k(ctx->c, "k:k_dyadic", 3.0 * nl * np);
        ew_dyadic(ctx->c, a, b, out, (int)limb0, (int)nl, (int)np);
    });
}
int hec_device_alloc(hec_context *ctx, uint64_t bytes, void **out)
{
    return guard([&] {
        set_device(ctx);
        HEC_HIP(hipMalloc(out, bytes ? bytes : 8));
    });
}
int hec_device_free(hec_context *ctx, void *p)
{
    return guard([&] {
        set_device(ctx);
        HEC_HIP(hipStreamSynchronize(ctx->c.stream));
        HEC_HIP(hipFree(p));
    });
}
int hec_memcpy_h2d(hec_context *ctx, void *dst, const void *src, uint64_t bytes)
{
    return guard([&] {
        set_device(ctx);
        HEC_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->c.stream));
        HEC_HIP(hipStreamSynchronize(ctx->c.stream));
    });
}
int hec_memcpy_d2h(hec_context *ctx, void *dst, const void *src, uint64_t bytes)
{
    return guard([&] {
        set_device(ctx);
        HEC_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->c.stream));
        HEC_HIP(hipStreamSynchronize(ctx->c.stream));
    });
}

int hec_time_ntt_forward(hec_context *ctx, uint64_t *d, uint64_t nl, uint64_t np, int reps, double *ms)
{
    return guard([&] {
        set_device(ctx);
        need(d && ms && reps >= 1 && nl <= ctx->c.K, "invalid argument");
        Ctx &c = ctx->c;
        int pm[HEC_MAXL + 1];
        for (uint64_t i = 0; i < nl; ++i) pm[i] = (int)i;
        hipEvent_t e0, e1;
        HEC_HIP(hipEventCreate(&e0));
        HEC_HIP(hipEventCreate(&e1));
        HEC_HIP(hipEventRecord(e0, c.stream));
        for (int r = 0; r < reps; ++r)
            ntt_strided(c, false, d, nl * c.N, d, nl * c.N, (int)nl, pm, (int)(nl * np));
        HEC_HIP(hipEventRecord(e1, c.stream));
        HEC_HIP(hipEventSynchronize(e1));
        float t = 0;
        HEC_HIP(hipEventElapsedTime(&t, e0, e1));
        *ms = t / reps;
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
    });
}

int hec_profile_enable(hec_context *ctx, int mode)
{
    return guard([&] {
        need(ctx != nullptr && mode >= 0 && mode <= 2, "invalid argument");
        Ctx &c = ctx->c;
        set_device(ctx);
        prof_resolve(c);
        c.prof_mode = mode;
        if (mode) c.prof_tab.clear();
    });
}
int hec_profile_read_ex(hec_context *ctx, const char *cls, double *total_ms, uint64_t *scopes, double *alg_bytes,
                        uint64_t *kernel_launches)
{
    return guard([&] {
        need(ctx && cls, "null");
        set_device(ctx);
        prof_resolve(ctx->c);
        auto it = ctx->c.prof_tab.find(cls);
        const bool has = it != ctx->c.prof_tab.end();
        if (total_ms) *total_ms = has ? it->second.ms : 0;
        if (scopes) *scopes = has ? it->second.n : 0;
        if (alg_bytes) *alg_bytes = has ? it->second.bytes : 0;
        if (kernel_launches) *kernel_launches = has ? it->second.kl : 0;
    });
}
uint64_t hec_profile_classes(hec_context *ctx, char *buf, uint64_t cap)
{
    if (!ctx) return 0;
    std::string all;
    try {
        set_device(ctx);
        prof_resolve(ctx->c);
    } catch (...) {
        return 0;
    }
    for (const auto &kv : ctx->c.prof_tab) all += kv.first + "\n";
    if (buf && cap) {
        const std::size_t n = std::min<std::size_t>(all.size(), cap - 1);
        std::memcpy(buf, all.data(), n);
        buf[n] = 0;
    }
    return all.size() + 1;
}
int hec_profile_read(hec_context *ctx, const char *cls, double *total_ms, uint64_t *launches)
{
    return guard([&] {
        need(ctx && cls, "null");
        set_device(ctx);
        prof_resolve(ctx->c);
        auto it = ctx->c.prof_tab.find(cls);
        if (total_ms) *total_ms = it == ctx->c.prof_tab.end() ? 0 : it->second.ms;
        if (launches) *launches = it == ctx->c.prof_tab.end() ? 0 : it->second.n;
    });
}

}  // extern "C"
