// The key switch of the CKKS engine: the mod-downs, keyswitch(), the hoisted mod-up of a rotation-trie node and its
// children, the per-key tables of a Galois key, and the batched building blocks over them (galois_ks, rescale_batch,
// relin_rescale).  All of it is batched over B ciphertexts in one strided array.
//
// Key switch dataflow (SEAL 4.1 Evaluator::switch_key_inplace, per-prime digits + special prime P,
// SURVEY §8(a) a5), B targets T[b] (NTT form, l limbs):
//   (1) D[b][J]    = INTT_J(T[b][J])                                    ntt_strided (inverse)
//   (2) E[b][I][J] = NTT_I(D[b][J] mod q_I),  I in {0..l-1, P}, I != J   ks_modup (reduction fused)
//   (3) ACC[b][k][I] = sum_J E[b][I][J] * key[J][k][I]   (E[b][I][I] = T[b][I])   ks_mac
//   (4) y = INTT_P(ACC[b][k][P])                                        ntt_strided (inverse)
//   (5) OUT[b][k][i] = IN[b][k][i] + (ACC[b][k][i] - NTT_i(round(y))) * P^-1     divide_round
#include <algorithm>
#include <optional>

#include "hec_engine.h"

using namespace hec;

namespace {

// the separate add of a key switch's optional addend: OUT += ADD (both polys), where the last stage did not add it
static void add_after(Ctx &c, PolyArr OUT, PolyArr ADD, int B, int l)
{
    ProfScope k(c, "k:k_ew_add/rot_add", 6.0 * B * l);  // two ciphertexts read, one written
    ew_add(c, OUT, ADD, OUT, B, 2, l, 0);
}

// key-switch mod-down (SEAL switch_key_inplace step 4): the P-limb INTT's first pass, the fan-out that
// finishes it and forms the rounding limbs, and divide_round's pass B (OUT = IN + (ACC_i - r) P^-1)
// single-pass form (c.moddown1, N = 2^15): the P limbs' whole INTT in place, then k_moddown1 forms each data limb's
// rounding limb, transforms it and divides-and-rounds in one kernel (no Z round trip, no fan-out, no pass B)
// ADD (optional, ng == 1): a second addend of both polys, unpermuted, added in the kernel's store (may be OUT[0])
static bool moddown_single(Ctx &c, u64 *ACC, PolyArr IN, int in_nk, const PolyArr *OUT, const u32 *elts, int ng, int B,
                           int l, PolyArr ADD = PolyArr{})
{
    if (!c.moddown1 || c.logN != 15) return false;
    if (ADD.p && ng != 1) throw std::logic_error("moddown_single: an addend with sibling rotations");
    const u64 N = c.N, sacc = (u64)B * 2 * (l + 1) * N;
    ProfScope ps(c, "ks_moddown");
    const int pP[1] = {(int)c.K - 1};
    {  // both passes of the P limbs' INTT: read + write 2 B ng limbs per pass
        ProfScope k(c, "k:k_ntt/moddown_intt", 8.0 * B * ng, 2);
        ntt_strided(c, true, ACC + l * N, (l + 1) * N, ACC + l * N, (l + 1) * N, 1, pP, 2 * B * ng, 1, 3);
    }
    for (int q = 0; q < ng; ++q) {  // P limb (2B, once per (b, k)), ACC (2Bl), IN (in_nk B l), OUT (2Bl), ADD (2Bl)
        ProfScope k(c, ADD.p ? "k:k_moddown1/moddown_add" : "k:k_moddown1/moddown",
                    (2.0 + (4.0 + in_nk + (ADD.p ? 2.0 : 0.0)) * l) * B, 2);  // one launch per class
        moddown1(c, ACC + q * sacc + l * N, 2 * (l + 1) * N, (l + 1) * N, PolyArr{ACC + q * sacc, 2 * (l + 1) * N, (l + 1) * N},
                 IN, in_nk, OUT[q], B, 2, l, (int)c.K - 1, elts[q], ADD);
    }
    return true;
}

}  // namespace

namespace hec {

// ------------------------------------------------------------------ batched building blocks
std::size_t ks_words(const Ctx &c, std::size_t B, std::size_t l)
{
    return c.N * B * (l + (l + 1) * l + 2 * (l + 1) + 2 * l) + 4 * 64;
}

// ADD (optional): OUT = ... + ADD as well, both polys, unpermuted (may be OUT).  k_moddown1 adds it in its store; the
// two-pass forms run k_ew_add after themselves
void moddown(Ctx &c, u64 *ACC, u64 *Z, PolyArr IN, int in_nk, PolyArr OUT, int B, int l, u32 elt,
             PolyArr ADD)
{
    if (moddown_single(c, ACC, IN, in_nk, &OUT, &elt, 1, B, l, ADD)) return;
    const u64 N = c.N;
    const bool fan = c.fan_out;
    ProfScope ps(c, "ks_moddown");
    const int pP[1] = {(int)c.K - 1};
    {  // P limbs of both key polys: read + write 2B limbs per pass
        ProfScope k(c, fan ? "k:k_ntt/moddown_intt" : "k:k_ntt/moddown_intt2", 4.0 * B, fan ? 1 : 2);
        ntt_strided(c, true, ACC + l * N, (l + 1) * N, ACC + l * N, (l + 1) * N, 1, pP, 2 * B, 1, fan ? 1 : 3);
    }
    if (fan) {  // 2B P limbs -> 2B l rounding limbs (pass-A domain)
        ProfScope k(c, "k:k_fan2/moddown", 2.0 * B * (l + 1));
        fan_divide_round(c, ACC + l * N, 2 * (l + 1) * N, (l + 1) * N, Z, B, 2, l, (int)c.K - 1);
    }
    {  // Z (2Bl), ACC data limbs (2Bl), IN (in_nk B l), OUT (2Bl)
        ProfScope k(c, fan ? "k:k_ntt/divround_b" : "k:k_ntt/divround2", (6.0 + in_nk) * B * l, fan ? 1 : 2);
        divide_round(c, ACC + l * N, 2 * (l + 1) * N, (l + 1) * N, PolyArr{ACC, 2 * (l + 1) * N, (l + 1) * N}, IN,
                     in_nk, OUT, B, 2, l, (int)c.K - 1, c.p_inv.data(), c.p_inv_q.data(), Z, elt, fan ? 2 : 3);
    }
    if (ADD.p) add_after(c, OUT, ADD, B, l);
}

// The mod-downs of ng sibling rotations of one node at once: ACC[q] = ACC + q B 2 (l+1) N (contiguous), IN the
// node's ciphertexts read through each child's permutation.  The P-limb INTT pass and the fan-out (small,
// latency-bound launches) run over all ng B entries in one launch each; divide_round's pass B per child.
void moddown_group(Ctx &c, u64 *ACC, u64 *Z, PolyArr IN, int in_nk, const PolyArr *OUT, const u32 *elts, int ng,
                   int B, int l)
{
    const u64 N = c.N, sacc = (u64)B * 2 * (l + 1) * N, sz = (u64)B * 2 * l * N;
    if (moddown_single(c, ACC, IN, in_nk, OUT, elts, ng, B, l)) return;
    if (!c.fan_out || ng == 1) {
        for (int q = 0; q < ng; ++q) moddown(c, ACC + q * sacc, Z, IN, in_nk, OUT[q], B, l, elts[q]);
        return;
    }
    ProfScope ps(c, "ks_moddown");
    const int pP[1] = {(int)c.K - 1};
    {
        ProfScope k(c, "k:k_ntt/moddown_intt", 4.0 * B * ng);
        ntt_strided(c, true, ACC + l * N, (l + 1) * N, ACC + l * N, (l + 1) * N, 1, pP, 2 * B * ng, 1, 1);
    }
    {
        ProfScope k(c, "k:k_fan2/moddown", 2.0 * B * ng * (l + 1));
        fan_divide_round(c, ACC + l * N, 2 * (l + 1) * N, (l + 1) * N, Z, B * ng, 2, l, (int)c.K - 1);
    }
    for (int q = 0; q < ng; ++q) {
        ProfScope k(c, "k:k_ntt/divround_b", (6.0 + in_nk) * B * l);
        divide_round(c, ACC + q * sacc + l * N, 2 * (l + 1) * N, (l + 1) * N,
                     PolyArr{ACC + q * sacc, 2 * (l + 1) * N, (l + 1) * N}, IN, in_nk, OUT[q], B, 2, l, (int)c.K - 1,
                     c.p_inv.data(), c.p_inv_q.data(), Z + q * sz, elts[q], 2);
    }
}

// T (the target polys) and IN (added to the output) are read through the Galois permutation of elt
// (elt = 1: as they are).  OUT must not overlap T or IN when elt != 1 (the reads gather).
// ADD (optional): a second addend of both output polys, OUT = (acc - NTT(z)) P^-1 + perm(IN) + ADD, read unpermuted at
// the words a thread writes, so ADD may be OUT: the accumulate step acc' = acc + rotate(src, step) of a sum over
// slots as one key switch.  Added in the last stage's store by k_bmac's divide-and-round epilogue and by k_moddown1
// (option "rot_add" = 1, the default); by a k_ew_add launch after every other path, and after all with "rot_add" = 0
void keyswitch(Ctx &c, Scratch &s, PolyArr T, const u64 *key, PolyArr IN, int in_nk, PolyArr OUT, int B, int l,
               u32 elt, PolyArr ADD)
{
    if (ADD.p && !c.rot_add) {
        keyswitch(c, s, T, key, IN, in_nk, OUT, B, l, elt);
        add_after(c, OUT, ADD, B, l);
        return;
    }
    const u64 N = c.N;
    const std::size_t top = s.top;
    u64 *D = s.take(B * l * N), *E = s.take((u64)B * (l + 1) * l * N), *ACC = s.take((u64)B * 2 * (l + 1) * N),
        *Z = s.take((u64)B * 2 * l * N);
    int pmap[HEC_MAXL + 1];
    for (int i = 0; i <= HEC_MAXL; ++i) pmap[i] = i;
    const bool fan = c.fan_out && c.fused_modup_mac;
    const double K = l + 1;
    {
        ProfScope ps(c, "ks_intt");  // with fan-out only its first pass; the fan kernel finishes it
        ProfScope k(c, fan ? "k:k_ntt/intt_b" : "k:k_ntt/intt2", 2.0 * B * l, fan ? 1 : 2);
        ntt_strided(c, true, T.p, T.sb, D, l * N, l, pmap, B * l, elt, fan ? 1 : 3);
    }
    if (c.fused_modup_mac) {  // mod-up pass A, then pass B fused with the key MAC (no E round trip)
        {
            ProfScope ps(c, "ks_modup_a");
            ProfScope k(c, fan ? "k:k_fan2j/modup" : "k:k_ntt/modup_a", (double)B * l * (l + 1), 1);
            if (fan) fan_modup(c, D, E, B, l);
            else ks_modup_mac(c, D, E, T, key, ACC, B, l, 1, elt);
        }
        if (fan && c.mac_divround && !(c.moddown1 && c.logN == 15)) {
            // the special-prime target first; its INTT and the fan-out give the rounding limbs Z, and the data
            // targets' launch divides-and-rounds its accumulators in its epilogue: ACC's data limbs are never stored
            const int pP[1] = {(int)c.K - 1};
            {  // digits E[b][P] (B l) + key (2 l) -> ACC's P limbs (2 B)
                ProfScope ps(c, "ks_bmac");
                ProfScope k(c, "k:k_bmac/p", (double)B * l + 2.0 * l + 2.0 * B, 1);
                ks_modup_mac(c, D, E, T, key, ACC, B, l, 2, elt, nullptr, 1);
            }
            {
                ProfScope ps(c, "ks_moddown");
                {
                    ProfScope k(c, "k:k_ntt/moddown_intt", 4.0 * B, 1);
                    ntt_strided(c, true, ACC + l * N, (l + 1) * N, ACC + l * N, (l + 1) * N, 1, pP, 2 * B, 1, 1);
                }
                ProfScope k(c, "k:k_fan2/moddown", 2.0 * B * (l + 1));
                fan_divide_round(c, ACC + l * N, 2 * (l + 1) * N, (l + 1) * N, Z, B, 2, l, (int)c.K - 1);
            }
            {  // digits E (B l (l - 1)) + targets (B l) + key (2 l l) + Z (2 B l) + IN (in_nk B l) -> OUT (2 B l);
               // with ADD its 2 B l as well
                ProfScope ps(c, "ks_bmac");
                ProfScope k(c, ADD.p ? "k:k_bmac/divround_add" : "k:k_bmac/divround",
                            (double)B * l * l + 2.0 * l * l + (4.0 + in_nk + (ADD.p ? 2.0 : 0.0)) * B * l, 1);
                BmacDR dr{};
                dr.Z = Z; dr.IN = IN; dr.OUT = OUT; dr.in_nk = in_nk;
                for (int i = 0; i < l; ++i) { dr.inv[i] = c.p_inv[i]; dr.inv_q[i] = c.p_inv_q[i]; }
                ks_modup_mac(c, D, E, T, key, ACC, B, l, 2, elt, &dr, 2, ADD.p ? &ADD : nullptr);
            }
            s.top = top;
            return;
        }
        {  // digits E (B l^2) + the I == J targets (B l) + key (2 l K) -> ACC (2 B K)
            ProfScope ps(c, "ks_bmac");
            ProfScope k(c, "k:k_bmac", (double)B * l * l + (double)B * l + 2.0 * l * K + 2.0 * B * K,
                        1);
            ks_modup_mac(c, D, E, T, key, ACC, B, l, 2, elt);
        }
    } else {
        {
            ProfScope ps(c, "ks_modup");
            ks_modup(c, D, E, B, l);
        }
        {
            ProfScope ps(c, "ks_mac");
            ks_mac(c, T, E, key, ACC, B, l, elt);
        }
    }
    moddown(c, ACC, Z, IN, in_nk, OUT, B, l, elt, ADD);
    s.top = top;
}

std::size_t hoist_words(const Ctx &c, std::size_t B, std::size_t l)
{
    return c.N * B * (l + (l + 1) * l + (std::size_t)HOIST_GROUP * 2 * (l + 1)) +
           ((1 + B * l * (HEC_ZCAP + 1)) * sizeof(int) + 7) / 8 + 4 * 64;
}
Hoist hoist_alloc(const Ctx &c, Scratch &s, int B, int l)
{
    Hoist h;
    h.D = s.take((u64)B * l * c.N);
    h.E = s.take((u64)B * (l + 1) * l * c.N);
    h.zl = reinterpret_cast<int *>(s.take(((1 + (u64)B * l * (HEC_ZCAP + 1)) * sizeof(int) + 7) / 8));
    h.sacc = (u64)B * 2 * (l + 1) * c.N;
    h.acc0 = s.take((u64)HOIST_GROUP * h.sacc);
    return h;
}
void hoist_node(Ctx &c, PolyArr X, int B, int l, const Hoist &h)
{
    const u64 N = c.N;
    int pmap[HEC_MAXL + 1];
    for (int i = 0; i <= HEC_MAXL; ++i) pmap[i] = i;
    if (c.hoist_scan) {  // the fan-out finishes the INTT and lists the zeros: no D round trip
        {
            ProfScope ps(c, "ks_intt");
            ProfScope k(c, "k:k_ntt/intt_b", 2.0 * B * l);
            ntt_strided(c, true, X.p + X.sk, X.sb, h.D, l * N, l, pmap, B * l, 1, 1);
        }
        ProfScope ps(c, "ks_modup_h");
        {
            ProfScope k(c, "k:k_fan2j/hoist", (double)B * l * (l + 1));
            fan_modup(c, h.D, h.E, B, l, false, h.zl);
        }
        ProfScope k(c, "k:k_ntt/modup_h_b", 2.0 * B * l * l);
        ks_modup(c, h.D, h.E, B, l, 2, c.hmac_cfg != 0);  // pass B: NTT-form digits (k_hmacm: MAC form)
        return;
    }
    {
        ProfScope ps(c, "ks_intt");
        {
            ProfScope k(c, "k:k_ntt/intt_b", 2.0 * B * l);
            ntt_strided(c, true, X.p + X.sk, X.sb, h.D, l * N, l, pmap, B * l, 1, 1);
        }
        {
            ProfScope k(c, "k:k_ntt/intt_a", 2.0 * B * l);
            ntt_strided(c, true, h.D, l * N, h.D, l * N, l, pmap, B * l, 1, 2);
        }
        ProfScope k(c, "k:k_zscan", (double)B * l);
        zero_scan(c, h.D, B * l, h.zl);
    }
    ProfScope ps(c, "ks_modup_h");
    {
        ProfScope k(c, "k:k_fan2j/hoist", (double)B * l * (l + 1));
        fan_modup(c, h.D, h.E, B, l, true);  // pass A of every NTT_I(D_J mod q_I), from the canonical D
    }
    ProfScope k(c, "k:k_ntt/modup_h_b", 2.0 * B * l * l);
    ks_modup(c, h.D, h.E, B, l, 2, c.hmac_cfg != 0);  // pass B: NTT-form digits (k_hmacm: MAC form)
}
// one child of a hoisted node: OUT = key switch of apply_galois(X, elt) (X: the node's ciphertexts)
void hoisted_child(Ctx &c, Scratch &s, PolyArr X, const Hoist &h, const u64 *W, const u64 *key, PolyArr OUT, int B,
                   int l, u32 elt)
{
    const u64 N = c.N;
    const std::size_t top = s.top;
    u64 *ACC = s.take((u64)B * 2 * (l + 1) * N), *Z = s.take((u64)B * 2 * l * N);
    {
        ProfScope ps(c, "ks_hmac");
        hoisted_mac(c, PolyArr{X.p + X.sk, X.sb, 0}, h.E, W, h.zl, key, ACC, B, l, elt);
    }
    moddown(c, ACC, Z, PolyArr{X.p, X.sb, X.sk}, 1, OUT, B, l, elt);
    s.top = top;
}
std::size_t hoisted_child_words(const Ctx &c, std::size_t B, std::size_t l)
{
    return c.N * B * std::max(2 * (l + 1) + 2 * l, (std::size_t)HOIST_GROUP * 2 * l) + 2 * 64;
}

// the sign-mask NTTs of a Galois key (built on first use): W[I] = NTT_I(m), m[t] = 1 iff coefficient t of
// apply_galois(x, elt) is a negated coefficient of x, i.e. t elt^-1 mod 2N >= N
const u64 *galois_negw(hec_context *ctx, hec_galois_keys &gk, u32 elt)
{
    auto it = gk.negw.find(elt);
    if (it != gk.negw.end()) return it->second;
    Ctx &c = ctx->c;
    const u64 N = c.N, m2 = 2 * N;
    const u64 einv = invm(elt, m2);
    std::vector<u64> mask(c.K * N);
    for (u64 t = 0; t < N; ++t) mask[t] = ((t * einv) % m2) >= N ? 1 : 0;
    for (std::size_t i = 1; i < c.K; ++i) std::copy(mask.begin(), mask.begin() + N, mask.begin() + i * N);
    u64 *W = dalloc(c.K * N);
    HEC_HIP(hipMemcpyAsync(W, mask.data(), c.K * N * sizeof(u64), hipMemcpyHostToDevice, c.stream));
    int pmap[HEC_MAXL + 1];
    for (int i = 0; i <= HEC_MAXL; ++i) pmap[i] = i;
    ntt_strided(c, false, W, c.K * N, W, c.K * N, (int)c.K, pmap, (int)c.K);
    HEC_HIP(hipStreamSynchronize(c.stream));  // the host mask goes out of scope
    gk.negw[elt] = W;
    return W;
}

// the sign-mask key sums of a Galois key at level l (built on first use, see k_keyw)
const u64 *galois_kw(hec_context *ctx, hec_galois_keys &gk, u32 elt, int l)
{
    auto it = gk.kw.find({elt, l});
    if (it != gk.kw.end()) return it->second;
    Ctx &c = ctx->c;
    u64 *KW = dalloc((std::size_t)2 * (l + 1) * c.N);
    key_wsum(c, gk.keys.at(elt), KW, l);
    gk.kw[{elt, l}] = KW;
    return KW;
}

// the MAC-form key table of a Galois key (built on first use, see mac_key_table)
const u64 *galois_mkey(hec_context *ctx, hec_galois_keys &gk, u32 elt)
{
    auto it = gk.mkey.find(elt);
    if (it != gk.mkey.end()) return it->second;
    Ctx &c = ctx->c;
    u64 *MK = dalloc((std::size_t)c.L * 2 * c.K * c.N);
    mac_key_table(c, gk.keys.at(elt), MK, (u32)invm(elt, 2 * c.N));
    gk.mkey[elt] = MK;
    return MK;
}

// X (size 2) -> OUT = apply_galois(X, elt) followed by key switching (SEAL apply_galois_inplace).
// When OUT does not alias X the permutation is applied inside the key switch's loads (the INTT of c1,
// the target reuse in the MAC, the c0 add in the mod-down) and never materialised; otherwise X is
// first permuted into scratch.
// ADD (optional): OUT = that + ADD (keyswitch's second addend; ADD may be OUT, and may be X when OUT is not)
void galois_ks(Ctx &c, Scratch &s, PolyArr X, PolyArr OUT, int B, int l, u32 elt, const u64 *key,
               PolyArr ADD)
{
    const u64 N = c.N;
    const bool alias = OUT.p == X.p || !c.fuse_galois;
    if (!alias) {
        keyswitch(c, s, PolyArr{X.p + X.sk, X.sb, 0}, key, PolyArr{X.p, X.sb, X.sk}, 1, OUT, B, l, elt, ADD);
        return;
    }
    const std::size_t top = s.top;
    u64 *S = s.take((u64)2 * B * l * N);
    {
        ProfScope ps(c, "galois");
        galois_permute(c, X, PolyArr{S, l * N, (u64)B * l * N}, B, 2, l, elt);
    }
    keyswitch(c, s, PolyArr{S + (u64)B * l * N, l * N, 0}, key, PolyArr{S, l * N, 0}, 1, OUT, B, l, 1, ADD);
    s.top = top;
}

// divide-and-round by q_{l-1}: X = B entries of nk polys at level l -> OUT at level l-1
void rescale_batch(Ctx &c, Scratch &s, PolyArr X, int B, int nk, int l, PolyArr OUT)
{
    ProfScope ps(c, "rescale");
    const u64 N = c.N;
    const std::size_t top = s.top;
    u64 *Y = s.take((u64)B * nk * N), *Z = s.take((u64)B * nk * (l - 1) * N);
    const int pm[1] = {l - 1};
    for (int k = 0; k < nk; ++k)
        ntt_strided(c, true, X.p + k * X.sk + (u64)(l - 1) * N, X.sb, Y + k * N, nk * N, 1, pm, B);
    divide_round(c, Y, nk * N, N, X, PolyArr{}, 0, OUT, B, nk, l - 1, l - 1, c.ql_inv[l].data(),
                 c.ql_inv_q[l].data(), Z);
    s.top = top;
}
std::size_t rescale_words(const Ctx &c, std::size_t B, std::size_t nk, std::size_t l)
{
    return c.N * B * nk * (1 + 2 * l) + 3 * 64;
}

// The tail of every ct x ct product (relinearize, rescale_to_next): the B size-3 entries A3 ([B][3][l][N]) are
// relinearized in place, then their first two polys divided-and-rounded into OUT at level l - 1.  relin_scope names a
// profile class around the key switch alone; ProfScope keeps the pointer, so it is a string literal
void relin_rescale(Ctx &c, Scratch &s, u64 *A3, const u64 *rk, int B, int l, PolyArr OUT, const char *relin_scope)
{
    const u64 N = c.N, S3 = 3 * (u64)l * N;
    const PolyArr Aa{A3, S3, (u64)l * N};
    {
        std::optional<ProfScope> pr;
        if (relin_scope) pr.emplace(c, relin_scope);
        keyswitch(c, s, PolyArr{A3 + 2 * (u64)l * N, S3, 0}, rk, Aa, 2, Aa, B, l);
    }
    rescale_batch(c, s, Aa, B, 2, l, OUT);
}

}  // namespace hec
