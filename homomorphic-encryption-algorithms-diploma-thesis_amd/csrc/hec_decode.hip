// The client half on the GPU: seal::Decryptor::decrypt and seal::CKKSEncoder::decode for batches of ciphertexts /
// plaintexts, the last two calls of every reference demo (src/demos/matrix_operations.cpp:107,126-127,1153-1156;
// client.cpp, fft.cpp and math_operations.cpp end the same way).
//
// The sequence is SEAL 4.1's, as far as it can be recalled here: SEAL is not part of this repository, and unlike the
// encoder (hec_encode.hip) no step of the decoder was pinned against the reference's binary, so the check of this
// file is a derived floating-point tolerance against the CPU restatement (tests/test_gpu_decode.py), NOT bit parity
// with SEAL.  Decryption is integer work and bit-exact by construction.
//   1. k_decrypt: Decryptor::decrypt's dot_product_ct_sk_array, out = c0 + s (c1 + s (c2 + ...)) per limb and
//      coefficient with canonical modular products (Horner, so s^2 is formed on the fly and no second key is
//      stored; any evaluation order gives the same canonical residue).  With size 1 it is the copy of a plaintext
//      into the work area (decode must not transform the caller's plaintext in place).
//   2. per limb the inverse NTT (the engine's ntt_strided).
//   3. k_dec_crt_upper: per coefficient the exact CRT composition  y_i = x_i (Q/q_i)^-1 mod q_i,
//      acc = sum_i y_i (Q/q_i) (W 64-bit words in registers, W = words(level Q) <= level), acc mod Q, the comparison
//      with the upper-half threshold (Q + 1) / 2, and the sum of the (Q - acc for the upper half) words into a
//      double, least significant first, each times (1 / scale) 2^(64 j) as SEAL's decode_internal sums them.  The
//      composition must be exact: a coefficient of 2^40 .. 2^80 against Q ~ 2^400 leaves nothing of a floating CRT.
//      Level 1 needs no composition.  The same kernel then runs the upper layers of step 4 on the 2^TS points
//      r + t C of column r: each thread parks its composed doubles in its own LDS column (the composition loops over
//      the points, the layers want them in registers), so no composed value travels through HBM as an integer.
//   4. DWTHandler::transform_to_rev over root_powers_ (root_powers_[i] = the 2N-th root at bitrev(i), host table by
//      the same glibc cos / sin route as the encoder's): Cooley-Tukey layers gap N/2 .. 1, v = y w, x' = x + v,
//      y' = x - v; the layer of m groups uses roots m .. 2m - 1.  Layers gap >= C in step 3, the rest inside
//      contiguous C-point chunks in LDS (k_dec_dwt_lds), the encoder's split run the other way.
//   5. k_dec_gather: slot i = point matrix_reps_index_map_[i] (the encoder's table), the first n_values of them.
// Built with -ffp-contract=off like the encoder, so every butterfly is the IEEE result of the stated expression.
#include "hec_internal.h"

#pragma clang fp contract(off)

namespace hec {

namespace {

__device__ __forceinline__ double2 cmul(double2 x, double2 w)  // __muldc3 for finite operands
{
    return make_double2(x.x * w.x - x.y * w.y, x.x * w.y + x.y * w.x);
}
__device__ __forceinline__ void ct(double2 &X, double2 &Y, double2 w)
{
    const double2 u = X, v = cmul(Y, w);
    X = make_double2(u.x + v.x, u.y + v.y);
    Y = make_double2(u.x - v.x, u.y - v.y);
}

// step 1: one thread per (entry b = blockIdx.z, limb i = blockIdx.y, coefficient t)
__global__ void __launch_bounds__(256) k_decrypt(const u64 *const *__restrict__ src, const u64 *__restrict__ sk,
                                                 int size, int level, int logN, const DevPrime *__restrict__ primes,
                                                 u64 *__restrict__ out)
{
    const u64 N = 1ull << logN;
    const u64 t = (u64)blockIdx.x * 256 + threadIdx.x;
    if (t >= N) return;
    const int i = blockIdx.y;
    const u64 b = blockIdx.z;
    const u64 *cp = src[b] + (u64)i * N + t;
    const u64 ps = (u64)level * N;  // words per polynomial
    u64 acc = cp[(u64)(size - 1) * ps];
    if (size > 1) {
        const DevPrime p = cprime(primes, i);
        const u64 s = sk[(u64)i * N + t];
        for (int k = size - 2; k >= 0; --k) acc = addmod(mulmod(acc, s, p), cp[(u64)k * ps], p.q);
    }
    out[(b * level + i) * N + t] = acc;
}

// acc[0 .. WM) += x[0 .. WM) * s (x zero-padded to WM words; the sum is known to fit)
template <int WM>
__device__ __forceinline__ void mw_mac(u64 (&acc)[WM], const u64 *__restrict__ x, u64 s)
{
    u64 carry = 0;
#pragma unroll
    for (int j = 0; j < WM; ++j) {
        u64 lo, hi;
        mul128(x[j], s, lo, hi);
        lo += carry;
        hi += lo < carry;  // hi <= 2^64 - 2 before: no overflow
        acc[j] += lo;
        carry = hi + (acc[j] < lo);
    }
}
template <int WM>
__device__ __forceinline__ bool mw_geq(const u64 (&a)[WM], const u64 *__restrict__ b)  // a >= b
{
    bool geq = true;  // equal so far, from the least significant word up: the last differing word decides
#pragma unroll
    for (int j = 0; j < WM; ++j) {
        const u64 bj = b[j];
        if (a[j] != bj) geq = a[j] > bj;
    }
    return geq;
}
template <int WM>
__device__ __forceinline__ void mw_sub(u64 (&a)[WM], const u64 *__restrict__ b)  // a -= b (a >= b)
{
    u64 borrow = 0;
#pragma unroll
    for (int j = 0; j < WM; ++j) {
        const u64 bj = b[j], d = a[j] - bj;
        const u64 nb = (a[j] < bj) | (d < borrow);
        a[j] = d - borrow;
        borrow = nb;
    }
}
template <int WM>
__device__ __forceinline__ void mw_rsub(u64 (&a)[WM], const u64 *__restrict__ b)  // a = b - a (b >= a)
{
    u64 borrow = 0;
#pragma unroll
    for (int j = 0; j < WM; ++j) {
        const u64 bj = b[j], d = bj - a[j];
        const u64 nb = (bj < a[j]) | (d < borrow);
        a[j] = d - borrow;
        borrow = nb;
    }
}

// The level's CRT table (device words, built by the host once per level): Q, (Q + 1) / 2, then per prime i < level
// Q / q_i, all WM = dec_wmax(level) words, zero-padded; then (Q / q_i)^-1 mod q_i per prime.
// Steps 3 and the upper layers of step 4.  x: [count][level][N] coefficient form; a: [count][N] complex work area.
constexpr int DEC_BLK = 128;
template <int TS, int WM>
__global__ void __launch_bounds__(DEC_BLK) k_dec_crt_upper(const u64 *__restrict__ x, const u64 *__restrict__ crt,
                                                           const double *__restrict__ inv_scale,
                                                           const double2 *__restrict__ roots, int logN, int logC,
                                                           int level, const DevPrime *__restrict__ primes,
                                                           double2 *__restrict__ a)
{
    constexpr int R = 1 << TS;
    __shared__ double park[R][DEC_BLK];
    const u64 N = 1ull << logN, C = 1ull << logC;
    const u64 r = (u64)blockIdx.x * DEC_BLK + threadIdx.x;
    if (r >= C) return;  // no barrier below: every thread reads only its own LDS column
    const u64 v = blockIdx.y;
    const u64 *xv = x + v * (u64)level * N;
    const double is = inv_scale[v];
    const u64 *Q = crt, *half = crt + WM, *Qi = crt + 2 * WM, *inv = crt + (2 + level) * WM;
#pragma unroll 1
    for (int t = 0; t < R; ++t) {
        const u64 k = r + (u64)t * C;
        double d = 0.0;
        bool neg = false;
        if (level == 1) {  // no composition: the residue, centred on q_0
            u64 w = xv[k];
            neg = w >= half[0];
            if (neg) w = Q[0] - w;
            if (w) d = (double)w * is;
        } else {
            u64 acc[WM];
#pragma unroll
            for (int j = 0; j < WM; ++j) acc[j] = 0;
#pragma unroll 1
            for (int i = 0; i < level; ++i) {
                const DevPrime p = cprime(primes, i);
                const u64 y = mulmod(xv[(u64)i * N + k], inv[i], p);
                mw_mac<WM>(acc, Qi + i * WM, y);
            }
            // acc < level Q: at most level - 1 subtractions
#pragma unroll 1
            for (int i = 1; i < level && mw_geq<WM>(acc, Q); ++i) mw_sub<WM>(acc, Q);
            neg = mw_geq<WM>(acc, half);
            if (neg) mw_rsub<WM>(acc, Q);
            double s = is;
#pragma unroll
            for (int j = 0; j < WM; ++j) {
                if (acc[j]) d += (double)acc[j] * s;
                s *= 0x1.0p64;
            }
        }
        park[t][threadIdx.x] = neg ? -d : d;
    }
    double2 z[R];
#pragma unroll
    for (int t = 0; t < R; ++t) z[t] = make_double2(park[t][threadIdx.x], 0.0);
    // layer st = 0 .. TS - 1: gap N / 2^(st + 1) = C 2^(TS - 1 - st), m = 2^st groups; point r + t C lies in group
    // t >> (TS - st) and pairs with t + 2^(TS - 1 - st)
#pragma unroll
    for (int st = 0; st < TS; ++st) {
        const int h = 1 << (TS - 1 - st);
#pragma unroll
        for (int t = 0; t < R; ++t) {
            if (t & h) continue;
            ct(z[t], z[t + h], roots[(1 << st) + (t >> (TS - st))]);
        }
    }
    double2 *av = a + (v << logN);
#pragma unroll
    for (int t = 0; t < R; ++t) av[r + (u64)t * C] = z[t];
}

// step 4, layers gap = C/2 .. 1 inside contiguous chunks of C = 2^LOGC points staged in LDS.  The layer of gap 2^lg
// has m = N >> (lg + 1) groups; group g uses root_powers_[m + g].
template <int LOGC>
__global__ void __launch_bounds__(256) k_dec_dwt_lds(double2 *__restrict__ a, const double2 *__restrict__ roots,
                                                     int logN)
{
    constexpr int C = 1 << LOGC;
    __shared__ double2 s[C];
    const u64 N = 1ull << logN, base = (u64)blockIdx.x * C;
    double2 *av = a + ((u64)blockIdx.y << logN) + base;
    for (int k = threadIdx.x; k < C; k += 256) s[k] = av[k];
    __syncthreads();
#pragma unroll 1
    for (int lg = LOGC - 1; lg >= 0; --lg) {
        const int gap = 1 << lg;
        const double2 *w = roots + (N >> (lg + 1));
        for (int b = threadIdx.x; b < C / 2; b += 256) {
            const int j = b & (gap - 1);
            const int x = ((b >> lg) << (lg + 1)) + j;    // upper element of the pair, local index
            const u64 grp = (base + (u64)x) >> (lg + 1);  // global group index
            ct(s[x], s[x + gap], w[grp]);
        }
        __syncthreads();
    }
    for (int k = threadIdx.x; k < C; k += 256) av[k] = s[k];
}

// step 5: one thread per (row blockIdx.y, slot i < nv)
__global__ void __launch_bounds__(256) k_dec_gather(const double2 *__restrict__ a, const u32 *__restrict__ map, u64 nv,
                                                    int logN, const u32 *__restrict__ row, double *__restrict__ re,
                                                    double *__restrict__ im)
{
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i >= nv) return;
    const double2 z = a[((u64)blockIdx.y << logN) + map[i]];
    const u64 o = (u64)row[blockIdx.y] * nv + i;
    re[o] = z.x;
    if (im) im[o] = z.y;
}

template <int WM>
void launch_crt_upper(Ctx &c, int ts, dim3 g, const u64 *x, const u64 *crt, const double *is, const double2 *roots,
                      int logc, int level, double2 *a)
{
#define HEC_DEC_CASE(T)                                                                                            \
    case T:                                                                                                        \
        k_dec_crt_upper<T, WM><<<g, DEC_BLK, 0, c.stream>>>(x, crt, is, roots, c.logN, logc, level, c.primes, a); \
        break;
    switch (ts) {
        HEC_DEC_CASE(1)
        HEC_DEC_CASE(2)
        HEC_DEC_CASE(3)
        HEC_DEC_CASE(4)
        HEC_DEC_CASE(5)
    default: throw std::invalid_argument("decode: N must be 2^10 .. 2^16");
    }
#undef HEC_DEC_CASE
}

}  // namespace

int dec_wmax(int words)
{
    if (words <= 4) return 4;
    if (words <= 8) return 8;
    if (words <= 11) return 11;
    if (words <= 17) return 17;
    throw std::invalid_argument("decode: the coefficient modulus of this level is too wide");
}

void decrypt_batch(Ctx &c, const u64 *const *src, const u64 *sk, int size, int level, int count, u64 *out)
{
    if (count > 65535 || level > 65535) throw std::invalid_argument("decrypt: batch too large");
    k_decrypt<<<dim3((unsigned)((c.N + 255) / 256), level, count), 256, 0, c.stream>>>(src, sk, size, level, c.logN,
                                                                                       c.primes, out);
    HEC_HIP(hipGetLastError());
}

void decode_batch(Ctx &c, u64 *x, int count, int level, const u64 *crt, int wmax, const double *inv_scale,
                  double *work, u64 nv, const u32 *row, double *re, double *im)
{
    const int logN = c.logN;
    const u64 N = c.N;
    if (count > 65535) throw std::invalid_argument("decode: batch too large");
    int pmap[HEC_MAXL + 1];
    for (int i = 0; i <= HEC_MAXL; ++i) pmap[i] = i;
    ntt_strided(c, true, x, (u64)level * N, x, (u64)level * N, level, pmap, count * level);
    const int logc = logN - 1 < 11 ? logN - 1 : 11, ts = logN - logc;
    const double2 *roots = reinterpret_cast<const double2 *>(c.dec_tw);
    double2 *a = reinterpret_cast<double2 *>(work);
    const dim3 gu((unsigned)(((N >> ts) + DEC_BLK - 1) / DEC_BLK), count);
    switch (wmax) {
    case 4: launch_crt_upper<4>(c, ts, gu, x, crt, inv_scale, roots, logc, level, a); break;
    case 8: launch_crt_upper<8>(c, ts, gu, x, crt, inv_scale, roots, logc, level, a); break;
    case 11: launch_crt_upper<11>(c, ts, gu, x, crt, inv_scale, roots, logc, level, a); break;
    case 17: launch_crt_upper<17>(c, ts, gu, x, crt, inv_scale, roots, logc, level, a); break;
    default: throw std::logic_error("decode: no kernel for this word count");
    }
    HEC_HIP(hipGetLastError());
    const dim3 gl((unsigned)(N >> logc), count);
    switch (logc) {
    case 11: k_dec_dwt_lds<11><<<gl, 256, 0, c.stream>>>(a, roots, logN); break;
    case 10: k_dec_dwt_lds<10><<<gl, 256, 0, c.stream>>>(a, roots, logN); break;
    case 9: k_dec_dwt_lds<9><<<gl, 256, 0, c.stream>>>(a, roots, logN); break;
    default: throw std::invalid_argument("decode: N must be 2^10 .. 2^16");
    }
    HEC_HIP(hipGetLastError());
    if (nv) {
        k_dec_gather<<<dim3((unsigned)((nv + 255) / 256), count), 256, 0, c.stream>>>(a, c.enc_map, nv, logN, row, re,
                                                                                      im);
        HEC_HIP(hipGetLastError());
    }
}

}  // namespace hec
