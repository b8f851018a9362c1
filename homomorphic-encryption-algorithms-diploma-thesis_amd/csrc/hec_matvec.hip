// The he::linalg drivers of the CKKS engine: the rotation prefix trie and its (hoisted) walk, the diag x col matvec
// (matvec_core) and its batch lanes, the baby-step giant-step schedules (bsgs_core for ct x pt and ct x ct,
// colcolt_bsgs for col x col^T), and the C-ABI of hec_matmul_*, hec_bsgs_plan, hec_colcolT_bsgs_plan and
// hec_matrix_matmul.  The sharded matvec (hec_shard.hip) runs matvec_check and matvec_lanes from here.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <mutex>
#include <numeric>
#include <thread>
#include <tuple>

#include "hec_engine.h"

using namespace hec;

namespace {

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

// HEC_DEBUG_LANES: a checksum of every key's sign-mask NTTs W and key sums KW at this level, compared with the first one
// seen (they are built once and must never change)
// first-seen checksums of the per-key tables, keyed by (key set, Galois element, level, table) -- not by device
// address, which a freed table hands on to another key set; a key set's entries leave with it
// (debug_key_tables_forget from hec_galois_keys_destroy)
std::mutex g_dbg_mu;
std::map<std::tuple<const hec_galois_keys *, u32, int, int>, u64> g_dbg_first;

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

}  // namespace

namespace hec {

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

void debug_key_tables_forget(const hec_galois_keys *gk)
{
    std::lock_guard<std::mutex> lock(g_dbg_mu);
    for (auto it = g_dbg_first.begin(); it != g_dbg_first.end();)
        it = std::get<0>(it->first) == gk ? g_dbg_first.erase(it) : std::next(it);
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

}  // namespace hec

// =============================================================================== C-ABI =====
extern "C" {

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

}  // extern "C"
