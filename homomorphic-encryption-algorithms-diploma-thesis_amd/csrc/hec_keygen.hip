// KeyGenerator / Encryptor on the GPU (include/hecdna.h): SEAL's Blake2xbPRNG as a kernel, the three
// samplers over its streams (uniform, ternary, centred binomial) and the fused RLWE sample
//   c1 = a,  c0 = -(a s + NTT(e)) (+ plaintext | + (P mod q_J) newkey on limb J).
//
// BLAKE2Xb (SEAL util/blake2xb.c): buffer k of a stream (4096 bytes) is 64 leaf hashes of one root hash,
//   root = BLAKE2b(key block = the 64-byte seed, then the 8-byte counter k; parameter block: digest 64, key 64,
//                  fanout 1, depth 1, xof length 4096)                                    two compressions
//   leaf i = BLAKE2b(root; parameter block: digest 64, fanout 0, depth 0, leaf length 64, node offset i,
//                  xof length 4096, inner length 64)                                      one compression
// One wavefront makes a buffer's 64 leaves, lane i leaf i; the roots of the few buffers a wavefront takes are computed
// by as many of its lanes side by side and broadcast through LDS (k_prng).  64-bit add / xor / rotate only.
#include "hec_internal.h"

namespace hec {

namespace {

__device__ __forceinline__ u64 rotr64(u64 x, int n) { return (x >> n) | (x << (64 - n)); }

#define HEC_B2_G(a, b, c, d, x, y)      \
    do {                                \
        v[a] = v[a] + v[b] + (x);       \
        v[d] = rotr64(v[d] ^ v[a], 32); \
        v[c] = v[c] + v[d];             \
        v[b] = rotr64(v[b] ^ v[c], 24); \
        v[a] = v[a] + v[b] + (y);       \
        v[d] = rotr64(v[d] ^ v[a], 16); \
        v[c] = v[c] + v[d];             \
        v[b] = rotr64(v[b] ^ v[c], 63); \
    } while (0)

__constant__ const u64 kB2IV[8] = {0x6a09e667f3bcc908ULL, 0xbb67ae8584caa73bULL, 0x3c6ef372fe94f82bULL, 0xa54ff53a5f1d36f1ULL,
                          0x510e527fade682d1ULL, 0x9b05688c2b3e6c1fULL, 0x1f83d9abfb41bd6bULL, 0x5be0cd19137e2179ULL};
__constant__ const unsigned char kB2Sigma[12][16] = {{0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15},
                                            {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
                                            {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4},
                                            {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
                                            {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13},
                                            {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
                                            {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11},
                                            {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
                                            {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5},
                                            {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0},
                                            {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15},
                                            {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3}};

// RFC 7693 compression F: h the chaining value, m the 16 message words, t the byte counter (< 2^64), last the
// final-block flag.  The rounds are fully unrolled, so every sigma lookup is a compile-time register choice.
__device__ __forceinline__ void b2_compress(u64 h[8], const u64 m[16], u64 t, bool last)
{
    u64 v[16];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        v[i] = h[i];
        v[i + 8] = kB2IV[i];
    }
    v[12] ^= t;
    if (last) v[14] = ~v[14];
#pragma unroll
    for (int r = 0; r < 12; ++r) {
        HEC_B2_G(0, 4, 8, 12, m[kB2Sigma[r][0]], m[kB2Sigma[r][1]]);
        HEC_B2_G(1, 5, 9, 13, m[kB2Sigma[r][2]], m[kB2Sigma[r][3]]);
        HEC_B2_G(2, 6, 10, 14, m[kB2Sigma[r][4]], m[kB2Sigma[r][5]]);
        HEC_B2_G(3, 7, 11, 15, m[kB2Sigma[r][6]], m[kB2Sigma[r][7]]);
        HEC_B2_G(0, 5, 10, 15, m[kB2Sigma[r][8]], m[kB2Sigma[r][9]]);
        HEC_B2_G(1, 6, 11, 12, m[kB2Sigma[r][10]], m[kB2Sigma[r][11]]);
        HEC_B2_G(2, 7, 8, 13, m[kB2Sigma[r][12]], m[kB2Sigma[r][13]]);
        HEC_B2_G(3, 4, 9, 14, m[kB2Sigma[r][14]], m[kB2Sigma[r][15]]);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) h[i] ^= v[i] ^ v[i + 8];
}

constexpr u64 kBufBytes = 4096, kBufWords = 512;

// the root hash of buffer `counter` of the stream keyed with seed[8]: two compressions
__device__ __forceinline__ void b2x_root(const u64 *__restrict__ seed, u64 counter, u64 root[8])
{
    u64 m[16];
#pragma unroll
    for (int i = 0; i < 8; ++i) root[i] = kB2IV[i];
    root[0] ^= 64ull | (64ull << 8) | (1ull << 16) | (1ull << 24);  // digest, key length, fanout, depth
    root[1] ^= kBufBytes << 32;                                      // node offset 0, xof length
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        m[i] = seed[i];
        m[i + 8] = 0;
    }
    b2_compress(root, m, 128, false);  // the key block
#pragma unroll
    for (int i = 0; i < 16; ++i) m[i] = 0;
    m[0] = counter;
    b2_compress(root, m, 128 + 8, true);  // the input: the u64 counter
}
// the 8 words of leaf `lane` of a buffer with that root: one compression
__device__ __forceinline__ void b2x_leaf(const u64 *root, u32 lane, u64 out[8])
{
    u64 m[16];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        m[i] = root[i];  // the leaf's message is the root
        m[i + 8] = 0;
        out[i] = kB2IV[i];
    }
    out[0] ^= 64ull | (64ull << 32);          // digest 64, key 0, fanout 0, depth 0, leaf length 64
    out[1] ^= (u64)lane | (kBufBytes << 32);  // node offset, xof length
    out[2] ^= 64ull << 8;                     // node depth 0, inner length 64
    b2_compress(out, m, 64, true);
}

// A work item is one buffer (stream, buffer index); a wavefront takes `group` consecutive items (1 .. kMaxGroup).  Its
// lanes t < group first compute the items' roots side by side (two compressions, whatever the group size) and leave
// them in LDS; then for each item every lane reads that root (an LDS broadcast) and computes its own leaf, one
// compression.  So a buffer costs 1 + 2 / group compressions per lane; the launcher picks the group size that still
// fills the device.
// UNIFORM: SEAL's sample_poly_uniform fused into the leaves: each word is reduced mod its limb's prime and stored; the
// words the host routine redraws are appended to rej with one atomic per wavefront and item (the 8 ballots give every
// lane its slot).  With SEAL's primes (q just below 2^k) a redraw has probability about 2^(k - 64) per word.
constexpr u32 kMaxGroup = 16;
template <bool UNIFORM>
__global__ void __launch_bounds__(256)
    k_prng(const u64 *__restrict__ seeds, u64 *const *__restrict__ dst, u64 nitems, u32 nbuf, u32 group, u64 nwords,
           int logN, UniSpec spec, u64 *__restrict__ rej, u32 *__restrict__ rej_n, u32 rej_cap)
{
    __shared__ u64 roots[4][kMaxGroup][8];
    const u32 wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const u64 first = ((u64)blockIdx.x * 4 + wv) * group;
    const u32 cnt = first < nitems ? (u32)(nitems - first < group ? nitems - first : group) : 0;  // per wavefront
    if (lane < cnt) {
        const u64 item = first + lane;
        u64 r[8];
        b2x_root(seeds + (item / nbuf) * 8, item % nbuf, r);
#pragma unroll
        for (int k = 0; k < 8; ++k) roots[wv][lane][k] = r[k];
    }
    __syncthreads();
#pragma unroll 1
    for (u32 t = 0; t < cnt; ++t) {  // whole wavefronts: the ballots below see every lane
        const u64 item = first + t;
        const u32 s = (u32)(item / nbuf), buf = (u32)(item % nbuf);
        u64 w[8];
        b2x_leaf(roots[wv][t], lane, w);
        const u64 g0 = (u64)buf * kBufWords + lane * 8;  // N >= 8: the 8 words lie in one limb
        u64 *__restrict__ out = dst[s];
        const bool live = g0 < nwords;  // nwords is a multiple of 8
        if (!UNIFORM) {
            if (live) {
#pragma unroll
                for (int k = 0; k < 8; ++k) out[g0 + k] = w[k];
            }
            continue;
        }
        const int limb = live ? (int)(g0 >> logN) : 0;
        const u64 q = spec.q[limb], ratio = spec.ratio[limb], maxm = spec.maxm[limb];
        u64 mask[8];
        u32 total = 0, before = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const bool r = live && w[k] >= maxm;
            mask[k] = __ballot(r);
            total += (u32)__popcll(mask[k]);
        }
        if (live) {
#pragma unroll
            for (int k = 0; k < 8; ++k) out[g0 + k] = barrett64(w[k], q, ratio);
        }
        if (total == 0) continue;  // wavefront-uniform: the common path ends here
        u32 base = 0;
        if (lane == 0) base = atomicAdd(rej_n, total);
        base = (u32)__shfl((int)base, 0);
        const u64 below = (1ull << lane) - 1;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if ((mask[k] >> lane) & 1) {
                const u32 slot = base + before + (u32)__popcll(mask[k] & below);
                if (slot < rej_cap) rej[slot] = ((u64)s << 32) | (g0 + k);
            }
            before += (u32)__popcll(mask[k]);
        }
    }
}

__global__ void __launch_bounds__(64)
    k_scatter(u64 *const *__restrict__ dst, const u64 *__restrict__ pos, const u64 *__restrict__ val, int n)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    dst[pos[i] >> 32][pos[i] & 0xffffffffull] = val[i];
}

// SEAL 4.1 sample_poly_cbd: coefficient i from stream bytes 6i .. 6i + 5, bytes 2 and 5 masked to 5 bits;
// e = popcount(b0) + popcount(b1) + popcount(b2) - popcount(b3) - popcount(b4) - popcount(b5) in [-21, 21]
__global__ void __launch_bounds__(256)
    k_sample_cbd(const u64 *__restrict__ raw, u64 raw_stride, u64 *__restrict__ E, int nl, int logN, u64 total,
                 const DevPrime *__restrict__ primes)
{
    const u64 idx = (u64)blockIdx.x * 256 + threadIdx.x;  // (stream, i)
    if (idx >= total) return;
    const u64 s = idx >> logN, i = idx & ((1ull << logN) - 1);
    const unsigned char *b = reinterpret_cast<const unsigned char *>(raw + s * raw_stride) + 6 * i;
    const int e = __popc((u32)b[0]) + __popc((u32)b[1]) + __popc((u32)(b[2] & 0x1F)) - __popc((u32)b[3]) -
                  __popc((u32)b[4]) - __popc((u32)(b[5] & 0x1F));
    u64 *o = E + ((s * nl) << logN) + i;
    for (int j = 0; j < nl; ++j) o[(u64)j << logN] = e < 0 ? primes[j].q - (u64)(-e) : (u64)e;
}

__global__ void __launch_bounds__(256)
    k_ternary_expand(const u64 *__restrict__ t, u64 *__restrict__ out, int nl, int logN, u64 total,
                     const DevPrime *__restrict__ primes)
{
    const u64 idx = (u64)blockIdx.x * 256 + threadIdx.x;  // (b, i)
    if (idx >= total) return;
    const u64 b = idx >> logN, i = idx & ((1ull << logN) - 1);
    const u64 v = t[idx];  // 0, 1, 2 -> -1, 0, 1
    u64 *o = out + ((b * nl) << logN) + i;
    for (int j = 0; j < nl; ++j) o[(u64)j << logN] = v == 0 ? primes[j].q - 1 : v - 1;
}

__global__ void __launch_bounds__(256)
    k_rlwe(const RlweJob *__restrict__ jobs, const u64 *__restrict__ sk, const u64 *__restrict__ E, int nl, int logN,
           u64 total, const DevPrime *__restrict__ primes)
{
    const u64 idx = (u64)blockIdx.x * 256 + threadIdx.x;  // (b, j, i)
    if (idx >= total) return;
    const u64 per = (u64)nl << logN;
    const u64 b = idx / per, ji = idx % per;
    const int j = (int)(ji >> logN);
    const RlweJob jb = jobs[b];
    const DevPrime pr = primes[j];
    u64 x = addmod(mulmod(jb.c1[ji], sk[ji], pr), E[idx], pr.q);
    x = x ? pr.q - x : 0;
    if (jb.add) {
        if (jb.add_limb < 0) x = addmod(x, jb.add[ji], pr.q);
        else if (jb.add_limb == j) x = addmod(x, mulmod(jb.add_mul, jb.add[ji], pr), pr.q);
    }
    jb.c0[ji] = x;
}

__global__ void __launch_bounds__(256)
    k_rlwe_pk(const u64 *__restrict__ U, const u64 *__restrict__ pk, u64 pk_sk, u64 *__restrict__ E, int nl, int logN,
              u64 total, const DevPrime *__restrict__ primes)
{
    const u64 idx = (u64)blockIdx.x * 256 + threadIdx.x;  // (b, j, i)
    if (idx >= total) return;
    const u64 per = (u64)nl << logN;
    const u64 b = idx / per, ji = idx % per;
    const DevPrime pr = primes[ji >> logN];
    const u64 u = U[idx];
    u64 *e = E + b * 2 * per + ji;
    e[0] = addmod(mulmod(u, pk[ji], pr), e[0], pr.q);
    e[per] = addmod(mulmod(u, pk[pk_sk + ji], pr), e[per], pr.q);
}

__global__ void __launch_bounds__(256)
    k_ct_store(const u64 *__restrict__ O, u64 *const *__restrict__ ct, const u64 *const *__restrict__ pt, int l,
               int logN, u64 total, const DevPrime *__restrict__ primes)
{
    const u64 idx = (u64)blockIdx.x * 256 + threadIdx.x;  // (b, k, j, i)
    if (idx >= total) return;
    const u64 per = (u64)l << logN;
    const u64 b = idx / (2 * per), kji = idx % (2 * per);
    u64 x = O[idx];
    if (kji < per) x = addmod(x, pt[b][kji], primes[kji >> logN].q);
    ct[b][kji] = x;
}

unsigned blocks256(u64 total) { return (unsigned)((total + 255) / 256); }

}  // namespace

void prng_streams(Ctx &c, const u64 *seeds, u64 *const *dst, int nstreams, u64 nwords, const UniSpec *spec, u64 *rej,
                  u32 *rej_n, u32 rej_cap)
{
    if (nstreams <= 0 || !nwords) return;
    if (nwords % 8) throw std::logic_error("prng_streams: a stream's words come in whole leaves");
    const u32 nbuf = (u32)((nwords + kBufWords - 1) / kBufWords);
    const u64 nitems = (u64)nstreams * nbuf;
    // buffers per wavefront: as many as leave about eight wavefronts for every SIMD of the device (256 CUs x 4)
    const u32 group = c.prng_group ? (u32)std::min<int>(c.prng_group, (int)kMaxGroup)
                                   : (u32)std::min<u64>(kMaxGroup, std::max<u64>(1, nitems / 8192));
    const u64 waves = (nitems + group - 1) / group;
    const unsigned grid = (unsigned)((waves + 3) / 4);
    if (spec)
        k_prng<true><<<grid, 256, 0, c.stream>>>(seeds, dst, nitems, nbuf, group, nwords, c.logN, *spec, rej, rej_n,
                                                 rej_cap);
    else
        k_prng<false><<<grid, 256, 0, c.stream>>>(seeds, dst, nitems, nbuf, group, nwords, c.logN, UniSpec{}, nullptr,
                                                  nullptr, 0);
    HEC_HIP(hipGetLastError());
}

void scatter_words(Ctx &c, u64 *const *dst, const u64 *pos, const u64 *val, int n)
{
    if (n <= 0) return;
    k_scatter<<<(unsigned)((n + 63) / 64), 64, 0, c.stream>>>(dst, pos, val, n);
    HEC_HIP(hipGetLastError());
}

void sample_cbd(Ctx &c, const u64 *raw, u64 raw_stride, u64 *E, int nstreams, int nl)
{
    const u64 total = (u64)nstreams * c.N;
    if (!total) return;
    k_sample_cbd<<<blocks256(total), 256, 0, c.stream>>>(raw, raw_stride, E, nl, c.logN, total, c.primes);
    HEC_HIP(hipGetLastError());
}

void ternary_expand(Ctx &c, const u64 *t, u64 *out, int B, int nl)
{
    const u64 total = (u64)B * c.N;
    if (!total) return;
    k_ternary_expand<<<blocks256(total), 256, 0, c.stream>>>(t, out, nl, c.logN, total, c.primes);
    HEC_HIP(hipGetLastError());
}

void rlwe_c0(Ctx &c, const RlweJob *jobs, const u64 *sk, const u64 *E, int B, int nl)
{
    const u64 total = (u64)B * nl * c.N;
    if (!total) return;
    k_rlwe<<<blocks256(total), 256, 0, c.stream>>>(jobs, sk, E, nl, c.logN, total, c.primes);
    HEC_HIP(hipGetLastError());
}

void rlwe_pk(Ctx &c, const u64 *U, const u64 *pk, u64 pk_sk, u64 *E, int B, int nl)
{
    const u64 total = (u64)B * nl * c.N;
    if (!total) return;
    k_rlwe_pk<<<blocks256(total), 256, 0, c.stream>>>(U, pk, pk_sk, E, nl, c.logN, total, c.primes);
    HEC_HIP(hipGetLastError());
}

void ct_store(Ctx &c, const u64 *O, u64 *const *ct, const u64 *const *pt, int B, int l)
{
    const u64 total = (u64)B * 2 * l * c.N;
    if (!total) return;
    k_ct_store<<<blocks256(total), 256, 0, c.stream>>>(O, ct, pt, l, c.logN, total, c.primes);
    HEC_HIP(hipGetLastError());
}

}  // namespace hec
