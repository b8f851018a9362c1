// Host orchestration + C-ABI of the CKKS engine (include/hecdna.h).
//
// Every public entry point restates one seal::Evaluator call that the reference's he_operators /
// he_linalg layer makes (file:line cited per function in hecdna.h), on device-resident SEAL-layout
// objects.  Internally all ciphertext work is BATCHED: the key switch, rotation and rescale
// routines take B ciphertexts in one strided array so that one launch sequence (and one read of
// the key) serves the whole batch; the single-object C-ABI calls are the B = 1 case.
//
// This file holds the error string, the host number theory, the workspace, context setup and options, the device
// objects' lifecycle and every object's calls (the keys and the SEAL wire-format glue among them), the primitives and
// the profile calls.  The rest of the engine is split by concern: the key switch in hec_keyswitch.hip, the he::linalg
// drivers in hec_matvec.hip, the multi-GPU calls in hec_shard.hip, encode, decrypt / decode, keygen and encrypt in
// hec_client.hip, the one-object Evaluator calls in hec_evaluator.hip; what crosses between these files is declared in
// hec_engine.h.  The library-level layers over many ciphertexts (he::fft, he::math, he::linalg's element-wise
// products and slot sums) live in hec_batched.hip, written over the building blocks that hec_host.h declares; the
// object structs, the error guard, Scratch and ProfScope are in hec_host.h as well.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

#include "hec_engine.h"
#include "hec_live.h"

#include <unistd.h>

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

// ---------------------------------------------------------------- SEAL wire format on device objects
void seal_rc(int rc)
{
    if (rc == HEC_EINVAL) throw std::invalid_argument(hec_seal_last_error());
    if (rc != HEC_OK) throw std::logic_error(hec_seal_last_error());
}
// Decompressed-size limit of a KSwitchKeys object loaded into this context (the bytes come from a client socket,
// server.cpp:110-122): `lists` key lists of L PublicKeys of u64[2][K][N], the object's N list-length words, and at
// most 256 B of SEALHeader / parms_id / ciphertext metadata per PublicKey.  The loader inflates the whole object into
// host memory before parsing it, so the default number of non-empty GaloisKeys lists is a fixed cap that does not
// depend on the device: four times SEAL's default set (create_galois_keys(), the reference's only form:
// matrix_operations.cpp:771,872,1064, holds 2 log2(N) - 1 lists), at least 64, at most N, and no more than half of the
// host's available physical memory can hold.  The same bound applies whether the object is compressed (the inflate
// budget) or not (counted as the lists are parsed).  hec_galois_keys_load_seal_ex takes an explicit limit instead.
uint64_t galois_lists_default(const Ctx &c)
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
uint64_t seal_keys_max_bytes(const Ctx &c, uint64_t lists)
{
    return lists * c.L * (2 * c.K * c.N * 8 + 256) + c.N * 8 + 4096;
}

}  // namespace

// The building blocks that another file calls (hec_host.h declares them for hec_batched.hip, hec_engine.h for the
// engine's other files); the helpers above are this file's alone.
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
bool are_close(double a, double b)  // SEAL util::are_close
{
    const double sf = std::max({std::fabs(a), std::fabs(b), 1.0});
    return std::fabs(a - b) < std::numeric_limits<double>::epsilon() * sf;
}
bool scale_ok(const Ctx &c, double scale, std::size_t level)  // SEAL is_scale_within_bounds
{
    return !(scale <= 0 || (int)std::log2(scale) >= c.total_bits(level));
}
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

// ------------------------------------------------------------------ device objects ---------
void bind(DevObject &o, hec_context *ctx)
{
    o.ctx = ctx;
    o.ctx_gen = ctx->gen;
    o.device = ctx->c.device;
}
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
// ------------------------------------------------------------------ keys ------------------
std::size_t key_words(const Ctx &c) { return c.L * 2 * c.K * c.N; }
void gk_check_elt(const Ctx &c, u32 elt)
{
    need((elt & 1) && elt < 2 * c.N, "Galois element is not valid");
}

}  // namespace hec

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

// ------------------------------------------------------------------ keys ------------------
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

// ---------------------------------------------------------------- SEAL wire format on device objects
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
