// The client half of the CKKS engine: the encoder's host tables and hec_encode / hec_encode_scalar, hec_decrypt,
// hec_decode and hec_decrypt_decode over one shared driver, and KeyGenerator and Encryptor (hec_keygen_*, hec_encrypt,
// hec_encrypt_symmetric) over the seeded samplers.  The kernels are in hec_encode.hip, hec_decode.hip and
// hec_keygen.hip; the key objects' upload, download and destroy are with the other objects in hec_engine.hip.
#include <algorithm>
#include <array>
#include <cmath>
#include <complex>
#include <cstring>

#include "hec_engine.h"
#include "hec_keygen_host.h"

using namespace hec;
using u128 = unsigned __int128;

namespace {

// ------------------------------------------------------------------ CKKS encoder ----------
// host tables of the GPU encoder (hec_encode.hip), built once per context, as SEAL 4.1's CKKSEncoder constructor
// builds them: matrix_reps_index_map_ (generator 3, bit-reversed positions) and inv_root_powers_[i] =
// conj(ComplexRoots(2N).get_root(bitrev(i - 1, logN) + 1)), where ComplexRoots holds (cos t, sin t),
// t = (i 6.283185307179586) / 2N for i <= 2N / 8 (glibc cos and sin as separate calls) and get_root extends them by
// the 8-fold symmetry
std::complex<double> seal_root(u64 m, const std::vector<std::complex<double>> &roots, u64 index)
{
    index &= m - 1;
    if (index <= m / 8) return roots[index];
    if (index <= m / 4) {
        const auto a = roots[m / 4 - index];
        return {a.imag(), a.real()};
    }
    if (index <= m / 2) {
        const auto a = seal_root(m, roots, m / 2 - index);
        return {-a.real(), a.imag()};
    }
    if (index <= 3 * m / 4) {
        const auto a = seal_root(m, roots, index - m / 2);
        return {-a.real(), -a.imag()};
    }
    const auto a = seal_root(m, roots, m - index);
    return {a.real(), -a.imag()};
}

// the residue mod q of a non-negative integer-valued double a (exactly the integer a, as SEAL's 64-bit, 128-bit
// (fmod / division by 2^64) and multi-word decompositions give it)
u64 exact_residue(double a, u64 q)
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

// ------------------------------------------------------------------ decrypt / decode -------
// little-endian multi-word x times a word
std::vector<u64> big_mul(const std::vector<u64> &x, u64 s)
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
            const auto r = seal_root(m, roots, (u64)brev((u32)i, c.logN));
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
    for (std::size_t i = 0; i < level; ++i) Q = big_mul(Q, c.q[i]);
    const int wm = dec_wmax((int)big_mul(Q, level).size());  // the composition's sum is below level Q
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
            P = big_mul(P, c.q[j]);
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

// ------------------------------------------------------------------ KeyGenerator / Encryptor
// DESIGN.md 4.10.  Every call derives its sub-streams on the host (64-byte seeds), uploads them, and runs the
// generator, the samplers, the noise NTTs and the fused RLWE kernel over all of its samples at once (in chunks that
// bound the workspace).  The uniform sampler's redraws are resolved once per chunk: one read-back of the count, and
// only when it is not zero the host walk over the streams' continuations and one scatter kernel.
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
        const auto r = seal_root(m, roots, (u64)brev((u32)(i - 1), c.logN) + 1);
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

// =============================================================================== C-ABI =====
extern "C" {

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

}  // extern "C"
