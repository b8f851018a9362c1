// The library-level layers over many ciphertexts: he::fft (hec_fft, hec_bfft), he::math (hec_math_*,
// hec_drop_chain_levels) and he::linalg's element-wise products and slot sums (hec_multiply_relin_rescale_many,
// hec_sum_elems_many), C-ABI of include/hecdna.h.
//
// Each layer is host orchestration over the engine's building blocks (hec_host.h: the key switch with its Galois and
// relinearize-and-rescale forms, the output store, the checks; defined in the engine's files) and the stage kernels behind
// hec_internal.h.  A call checks everything first, gathers its inputs into slots of one Scratch workspace, runs its
// stages over the whole batch in passes, and stores the outputs after the last stage.  The plumbing the three layers
// share comes first.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <vector>

#include "hec_host.h"

using namespace hec;

extern "C" {

// ------------------------------------------------------------------ plumbing of the batched layers
namespace {
constexpr int MAX_Y_JOBS = 65535;               // blocks along y of one NTT pass
constexpr std::size_t BATCH_AUTO_CHUNK = 256;  // automatic ciphertexts per pass at most (workspace size)

// ciphertexts per pass of n at level l: the key switch's mod-up pass B runs (l + 1) l blocks along y per ciphertext;
// option "math_chunk" caps it
std::size_t batch_chunk(const Ctx &c, std::size_t l, std::size_t n)
{
    std::size_t Bc = std::min<std::size_t>(BATCH_AUTO_CHUNK, std::max<std::size_t>(1, MAX_Y_JOBS / ((l + 1) * l)));
    if (c.math_chunk > 0) Bc = std::min<std::size_t>(Bc, (std::size_t)c.math_chunk);
    return std::min(Bc, n);
}

// the checks of a batch that runs as one: every input valid and of size 2, every output the context's, one level and
// bitwise one scale; the lowest failing entry is the call's error
void check_uniform_batch(const hec_context *ctx, const hec_ciphertext *const *in, hec_ciphertext *const *out,
                         uint64_t count)
{
    for (uint64_t i = 0; i < count; ++i) {
        check_ct(ctx, in[i]);
        check_obj(ctx, out[i], BAD_CT);
        need(in[i]->size == 2, "encrypted size must be 2");
        need(in[i]->level == in[0]->level, "encrypted1 and encrypted2 parameter mismatch");
        need(std::memcmp(&in[i]->scale, &in[0]->scale, sizeof(double)) == 0, "scale mismatch");
    }
}

// the front half of a fused multiply-rescale stage at level l: the batched INTT of the last-limb products Y (nsrc
// entries of 2 polys) and their rounding limbs Z (divide_round's pass A).  The layer names its two profile classes
// (string literals: ProfScope keeps the pointers)
void stage_round_limbs(Ctx &c, u64 *Y, u64 *Z, int nsrc, int l, const char *intt_class, const char *round_class)
{
    {
        ProfScope k(c, intt_class, 8.0 * nsrc, 2);
        const int pm[1] = {l - 1};
        ntt_strided(c, true, Y, c.N, Y, c.N, 1, pm, 2 * nsrc);
    }
    ProfScope k(c, round_class, 2.0 * nsrc * l);
    fft_round_limbs(c, Y, Z, nsrc, 2, l);
}
}  // namespace

// ------------------------------------------------------------------ he::fft ----------------
// Both transforms walk a chain of multiply_plain + rescale stages (reference src/core/he_fft.cpp).  A stage runs over
// all of its ciphertexts in a fixed number of launches: the stage's plaintexts from the batched encoder, the
// last-limb products, their batched INTT, the rounding limbs (divide_round's pass A) and the fused
// multiply-rescale-sum pass (hec_kernels.hip FftIOB); the in-slot FFT adds its two batched rotations.  The twiddles
// and diagonals come from hec_fft_host.cpp alone.  Outputs are written after the last stage, so an error leaves them
// untouched.
namespace {
struct FftPlan {
    std::size_t n = 0, B = 0, l0 = 0;
    int stages = 0, total = 0;  // total = stages + the inverse's 1/n step
    double scale = 0;
    std::vector<double> sc;     // the scale entering step s; sc[total] the result's
    // the checks shared by hec_fft and hec_bfft: `count` ciphertexts, n the transform size (a class member: no C
    // language linkage inside the C-ABI block)
    static FftPlan make(hec_context *ctx, const hec_ciphertext *const *in, uint64_t count, uint64_t n, int inverse,
                        hec_ciphertext *const *out);
};

FftPlan FftPlan::make(hec_context *ctx, const hec_ciphertext *const *in, uint64_t count, uint64_t n, int inverse,
                      hec_ciphertext *const *out)
{
    need(ctx && in && out && count >= 1, "null argument");
    const Ctx &c = ctx->c;
    need(n >= 1 && !(n & (n - 1)), "n must be a power of two");
    check_uniform_batch(ctx, in, out, count);
    FftPlan p;
    p.n = n;
    p.l0 = in[0]->level;
    while ((std::size_t(1) << p.stages) < n) ++p.stages;
    p.total = p.stages + (inverse ? 1 : 0);
    if (p.total > 0 && p.l0 < (std::size_t)p.total + 1)
        throw std::invalid_argument("end of modulus switching chain reached");
    // every step encodes at the operands' scale and level, multiplies (the scale squares) and rescales
    double sc = in[0]->scale;
    p.sc.push_back(sc);
    for (int s = 0; s < p.total; ++s) {
        const std::size_t l = p.l0 - s;
        need(scale_ok(c, sc, l), "scale out of bounds");
        need(scale_ok(c, sc * sc, l), "scale out of bounds");
        sc = sc * sc / (double)c.q[l - 1];
        p.sc.push_back(sc);
    }
    return p;
}

// the encoder's "encoded values are too large" check over the maxima of `count` encoded vectors at `level`
void fft_check_maxabs(const Ctx &c, const u64 *mx, std::size_t count, std::size_t level)
{
    for (std::size_t v = 0; v < count; ++v) {
        double maxabs;
        std::memcpy(&maxabs, &mx[v], sizeof(double));
        if (!std::isfinite(maxabs)) throw std::invalid_argument("encoded values are too large");
        const int max_bits = (int)std::ceil(std::log2(std::max(maxabs, 1.0))) + 1;
        if (max_bits >= c.total_bits(level)) throw std::invalid_argument("encoded values are too large");
    }
}

// one multiply-rescale-sum stage over source entries W (nsrc entries of 2 polys at level l) -> OUT (nout entries at
// level l - 1); P = the stage's plaintexts [..][l][N]; half / nb / nt as FftIOB
void fft_stage_core(Ctx &c, const u64 *W, const u64 *P, u64 *Y, u64 *Z, u64 *OUT, int nsrc, int nout, int l, int half,
                    int nb, int nt, int npt)
{
    const u64 N = c.N, sb = 2 * (u64)l * N, sk = (u64)l * N;
    {
        ProfScope k(c, "k:k_fft_lastprod/fft", 4.0 * nsrc + npt);
        fft_lastprod(c, W, sb, sk, P, sk, Y, nsrc, 2, l, half, nb);
    }
    stage_round_limbs(c, Y, Z, nsrc, l, "k:k_ntt/fft_intt", "k:k_ntt/fft_round_a");
    {  // Z and the source data limbs read once each, the plaintexts' data limbs, the outputs
        ProfScope k(c, "k:k_ntt/fft_mrs", (4.0 * nsrc + 2.0 * nout + npt) * (l - 1));
        fft_mrs(c, Z, W, sb, sk, P, sk, PolyArr{OUT, 2 * (u64)(l - 1) * N, (u64)(l - 1) * N}, nout, 2, l, half, nb, nt);
    }
}

// the inverse's last step: every entry times the scalar plaintext of 1 / n, rescaled
void fft_scale_step(Ctx &c, const u64 *W, u64 *P, u64 *Y, u64 *Z, u64 *OUT, int cnt, int l, double n, double scale)
{
    u64 words[HEC_MAXL + 1];
    scalar_words(c, 1.0 / n, scale, (std::size_t)l, words);
    fill_limbs(c, P, l, words);
    fft_stage_core(c, W, P, Y, Z, OUT, cnt, cnt, l, 0, cnt, 1, 1);
}

void fft_store(Ctx &c, const u64 *W, hec_ciphertext *const *out, std::size_t cnt, std::size_t l, double scale)
{
    for (std::size_t i = 0; i < cnt; ++i) store_ct(c, out[i], W + i * 2 * l * c.N, 2, l, scale);
}
}  // namespace

int hec_fft(hec_context *ctx, const hec_ciphertext *const *in, uint64_t n, int inverse, hec_ciphertext *const *out)
{
    return guard([&] {
        set_device(ctx);
        const FftPlan p = FftPlan::make(ctx, in, n, n, inverse, out);
        Ctx &c = ctx->c;
        const std::size_t N = c.N, l0 = p.l0, S0 = 2 * l0 * N;
        if (p.total == 0) {  // n = 1 forward: copies
            if (out[0] != in[0]) store_ct(c, out[0], in[0]->d, 2, l0, in[0]->scale);
            return;
        }
        need(n * 2 * (l0 - 1) <= (uint64_t)MAX_Y_JOBS, "too many ciphertexts for one stage");
        // twiddles of every stage, uploaded once: stage m holds 1 (the identity plaintext) and w_m^k, k < m / 2
        std::vector<double> tre, tim;
        for (std::size_t m = 2; m <= n; m <<= 1) {
            const std::size_t o = tre.size();
            tre.resize(o + 1 + m / 2);
            tim.resize(o + 1 + m / 2);
            tre[o] = 1.0;
            tim[o] = 0.0;
            need(hec_fft_twiddles(m, inverse, &tre[o + 1], &tim[o + 1]) == HEC_OK, "n must be a power of two");
        }
        const std::size_t ntw = tre.size(), npmax = n / 2 + 1;
        encoder_tables(c);
        Scratch s(c, 2 * n * S0 + npmax * l0 * N + 2 * n * N + 2 * n * (l0 - 1) * N + npmax * 2 * N + 3 * ntw +
                         16 * 64);
        u64 *Wa = s.take(n * S0), *Wb = s.take(n * S0), *P = s.take(npmax * l0 * N), *Y = s.take(2 * n * N);
        u64 *Z = s.take(std::max<std::size_t>(2 * n * (l0 - 1) * N, 1));
        double *work = reinterpret_cast<double *>(s.take(npmax * 2 * N));
        double *dre = reinterpret_cast<double *>(s.take(ntw)), *dim = reinterpret_cast<double *>(s.take(ntw));
        u64 *dmx = s.take(ntw);
        if (ntw) {
            HEC_HIP(hipMemcpyAsync(dre, tre.data(), ntw * sizeof(double), hipMemcpyHostToDevice, c.stream));
            HEC_HIP(hipMemcpyAsync(dim, tim.data(), ntw * sizeof(double), hipMemcpyHostToDevice, c.stream));
        }
        int lg = 0;
        while ((std::size_t(1) << lg) < n) ++lg;
        for (std::size_t j = 0; j < n; ++j)  // the working array: the input in bit-reversed order
            d2d(c, Wa + j * S0, in[lg ? brev((u32)j, lg) : 0]->d, S0);
        std::size_t l = l0, off = 0;
        int step = 0;
        for (std::size_t m = 2; m <= n; m <<= 1, ++step, --l) {
            ProfScope ps(c, "fft_stage");
            const int np = (int)(m / 2 + 1);
            {
                ProfScope k(c, "fft_encode");
                encode_batch(c, dre + off, dim + off, N / 2, np, p.sc[step], (int)l, work, P, dmx + off, 1);
            }
            fft_stage_core(c, Wa, P, Y, Z, Wb, (int)n, (int)n, (int)l, (int)(m / 2), 0, 2, np);
            std::swap(Wa, Wb);
            off += np;
        }
        if (inverse) {
            ProfScope ps(c, "fft_stage");
            fft_scale_step(c, Wa, P, Y, Z, Wb, (int)n, (int)l, (double)n, p.sc[step]);
            std::swap(Wa, Wb);
            --l;
        }
        std::vector<u64> mx(ntw);
        if (ntw) HEC_HIP(hipMemcpyAsync(mx.data(), dmx, ntw * sizeof(u64), hipMemcpyDeviceToHost, c.stream));
        HEC_HIP(hipStreamSynchronize(c.stream));
        off = 0;
        for (std::size_t m = 2, ll = l0; m <= n; m <<= 1, --ll) {
            fft_check_maxabs(c, mx.data() + off, m / 2 + 1, ll);
            off += m / 2 + 1;
        }
        fft_store(c, Wa, out, n, l, p.sc[p.total]);
    });
}

int hec_bfft(hec_context *ctx, const hec_ciphertext *const *in, uint64_t B, uint64_t n, int inverse,
             const hec_galois_keys *gk, hec_ciphertext *const *out)
{
    return guard([&] {
        set_device(ctx);
        need(n <= ctx->c.N / 2 || (n & (n - 1)), "n must be at most slot_count");
        const FftPlan p = FftPlan::make(ctx, in, B, n, inverse, out);
        check_obj(ctx, gk, BAD_GK);
        Ctx &c = ctx->c;
        const std::size_t N = c.N, l0 = p.l0, S0 = 2 * l0 * N;
        if (p.total == 0) {
            for (uint64_t i = 0; i < B; ++i)
                if (out[i] != in[i]) store_ct(c, out[i], in[i]->d, 2, l0, in[i]->scale);
            return;
        }
        // the rotations of every stage (hec_rotate_vector_inplace's rule: one key, else the NAF terms), found before
        // any work; diagonals of every stage, n values each, uploaded once
        std::vector<std::vector<u32>> eltL(p.stages), eltR(p.stages);
        std::vector<double> dre_h, dim_h;
        std::vector<int> nterm(p.stages);
        for (int i = 1; i <= p.stages; ++i) {
            const uint64_t k = uint64_t(1) << i;
            const int steps = (int)(n / k);
            rotation_elts(c, steps, *gk, eltL[i - 1]);
            if (i > 1) rotation_elts(c, -steps, *gk, eltR[i - 1]);
            nterm[i - 1] = i > 1 ? 3 : 2;
            for (int d = 0; d < nterm[i - 1]; ++d) {
                const std::size_t o = dre_h.size();
                dre_h.resize(o + n);
                dim_h.resize(o + n);
                need(hec_bfft_diagonal(d, k, n, inverse, &dre_h[o], &dim_h[o]) == HEC_OK, "n must be a power of two");
            }
        }
        const std::size_t nd = dre_h.size(), nvec = nd / n;
        encoder_tables(c);
        // chunks of ciphertexts: one pass of 3 Bc x 2 x (l0 - 1) blocks
        const std::size_t Bc = std::min<std::size_t>(B, std::max<std::size_t>(1, MAX_Y_JOBS / (6 * l0)));
        Scratch s(c, 6 * Bc * S0 + 3 * l0 * N + 6 * Bc * N + 6 * Bc * (l0 - 1) * N + 3 * 2 * N + 2 * nd + nvec +
                         ks_words(c, Bc, l0) + 2 * Bc * l0 * N + 16 * 64);
        u64 *Wa = s.take(3 * Bc * S0), *Wb = s.take(3 * Bc * S0), *P = s.take(3 * l0 * N), *Y = s.take(6 * Bc * N);
        u64 *Z = s.take(std::max<std::size_t>(6 * Bc * (l0 - 1) * N, 1));
        double *work = reinterpret_cast<double *>(s.take(3 * 2 * N));
        double *dre = reinterpret_cast<double *>(s.take(nd)), *dim = reinterpret_cast<double *>(s.take(nd));
        u64 *dmx = s.take(nvec);
        HEC_HIP(hipMemcpyAsync(dre, dre_h.data(), nd * sizeof(double), hipMemcpyHostToDevice, c.stream));
        HEC_HIP(hipMemcpyAsync(dim, dim_h.data(), nd * sizeof(double), hipMemcpyHostToDevice, c.stream));
        std::vector<u64> mx(nvec);
        for (std::size_t b0 = 0; b0 < B; b0 += Bc) {
            const std::size_t cnt = std::min(Bc, B - b0);
            for (std::size_t b = 0; b < cnt; ++b) d2d(c, Wa + b * S0, in[b0 + b]->d, S0);
            std::size_t l = l0, off = 0;
            for (int i = 1; i <= p.stages; ++i, --l) {
                ProfScope ps(c, "bfft_stage");
                const int nt = nterm[i - 1];
                const u64 sb = 2 * (u64)l * N, sk = (u64)l * N;
                {
                    ProfScope k(c, "fft_encode");
                    encode_batch(c, dre + off * n, dim + off * n, N / 2, nt, p.sc[i - 1], (int)l, work, P, dmx + off, n);
                }
                // the two rotations of the batch, back to back: entries [cnt, 2 cnt) and [2 cnt, 3 cnt) of the array
                const PolyArr X{Wa, sb, sk};
                for (int t = 1; t < nt; ++t) {
                    const std::vector<u32> &elts = t == 1 ? eltL[i - 1] : eltR[i - 1];
                    const PolyArr R{Wa + (u64)t * cnt * sb, sb, sk};
                    for (std::size_t e = 0; e < elts.size(); ++e)
                        galois_ks(c, s, e == 0 ? X : R, R, (int)cnt, (int)l, elts[e], gk->keys.at(elts[e]));
                }
                fft_stage_core(c, Wa, P, Y, Z, Wb, nt * (int)cnt, (int)cnt, (int)l, 0, (int)cnt, nt, nt);
                std::swap(Wa, Wb);
                off += nt;
            }
            if (inverse) {
                ProfScope ps(c, "bfft_stage");
                fft_scale_step(c, Wa, P, Y, Z, Wb, (int)cnt, (int)l, (double)n, p.sc[p.stages]);
                std::swap(Wa, Wb);
                --l;
            }
            if (b0 == 0) {
                HEC_HIP(hipMemcpyAsync(mx.data(), dmx, nvec * sizeof(u64), hipMemcpyDeviceToHost, c.stream));
                HEC_HIP(hipStreamSynchronize(c.stream));
                for (std::size_t v = 0, st = 0; st < (std::size_t)p.stages; ++st)
                    for (int d = 0; d < nterm[st]; ++d, ++v) fft_check_maxabs(c, mx.data() + v, 1, l0 - st);
            }
            fft_store(c, Wa, out + b0, cnt, l, p.sc[p.total]);
        }
        HEC_HIP(hipStreamSynchronize(c.stream));  // the host diagonals go out of scope
    });
}

// ------------------------------------------------------------------ he::math ---------------
// signed_inv / inv_sqrt_twice / sqrt / abs (reference src/core/he_math.cpp:22-269) and he::util::drop_chain_levels on
// a batch of ciphertexts of one level and scale.  Each schedule is written once, over MathRun, whose operations do the
// host bookkeeping of the per-operation sequence (every scalar encode's checks, every product scale and its bound,
// every division by q, every are_close, the end of the chain) in that sequence's order, and, when the run has a
// device side, launch the stage over the whole batch.  A call walks its schedule twice: first without a device side
// (the plan: the first failing check is the call's error, nothing has been written, and the peak number of live
// iterates is known), then on the device.  hec_math_plan is the first walk alone.
// Two stage kinds (hec_kernels.hip): the scalar stage OUT = rescale(A (*) c) +- d (math_lastprod, the batched INTT,
// fft_round_limbs, math_cstage) and the product stage OUT = rescale(relin(A (*) (B' + d))) (math_tensor, then
// keyswitch and rescale_batch as hec_matmul_finish runs them).  The iterates live in slots of one Scratch workspace.
// hec_math_poly (an extension: Paterson-Stockmeyer evaluation of a real polynomial) walks the same way
// over MathRun::poly and adds a third stage kind, the linear combination OUT = rescale(sum_t A_t (*) c_t) + d of up to
// HEC_MATH_MAXT values (math_lincomb_last, the same INTT and rounding limbs, math_lincomb), and views: a value read
// below the level its slot was written at (MathRun::down), which is what mod_switch_to_next costs here.
namespace {
// The product stage over B ciphertexts at level l: OUT = rescale(relin(A (*) (Bp [+ dw]))) at level l - 1.  A and Bp
// may be one array (the squares); T3: 3 B l N words for the size-3 products.  he::math's products and
// hec_multiply_relin_rescale_many (dw == nullptr) run it
void product_stage(Ctx &c, Scratch &s, PolyArr A, PolyArr Bp, const u64 *dw, u64 *T3, const u64 *rk, int B, int l,
                   PolyArr OUT)
{
    const bool same = A.p == Bp.p;
    {
        ProfScope k(c, "k:k_math_tensor/math", ((same ? 2.0 : 4.0) + 3.0) * B * l);
        math_tensor(c, A, Bp, dw, T3, B, l);
    }
    relin_rescale(c, s, T3, rk, B, l, OUT);
}

struct MathVal {
    int slot = -1;
    std::size_t level = 0;
    double scale = 0;
    std::size_t alloc = 0;  // limbs per poly of the slot's layout when it is read below the level it was written at
                            // (a view, MathRun::down); 0: level
};

struct MathRun {
    Chain ch;
    // device side; c == nullptr is the planning walk
    Ctx *c = nullptr;
    Scratch *s = nullptr;
    const u64 *rk = nullptr;
    int B = 0;
    std::vector<u64 *> slot;
    u64 *T3 = nullptr, *Y = nullptr, *Z = nullptr;
    // slot bookkeeping, the same on both walks
    std::vector<char> busy;
    int peak = 0;
    // poly(): block size, the powers computed so far with the uses each still has, the counts hec_math_poly_plan
    // reports, and every leaf's table in the order of the walk: its coefficient words, then three words per source
    // (offset from slot 0, entry stride, poly stride), as math_lincomb reads them.  tab_dev: the plan's table on the
    // device; slot_words: the distance of two slots (they are carved back to back); ring: N, 0 on a host-only plan
    std::size_t bs = 0, nprod = 0, nleaf = 0, slot_words = 0, ring = 0;
    MathVal x1;
    std::map<std::size_t, MathVal> pw;
    std::map<std::size_t, int> uses;
    std::vector<u64> tab;
    const u64 *tab_dev = nullptr;

    int take()
    {
        std::size_t i = 0;
        while (i < busy.size() && busy[i]) ++i;
        if (i == busy.size()) busy.push_back(0);
        busy[i] = 1;
        peak = std::max(peak, (int)i + 1);
        return (int)i;
    }
    void drop(MathVal &v)
    {
        if (v.slot >= 0) busy[(std::size_t)v.slot] = 0;
        v.slot = -1;
    }
    PolyArr arr(const MathVal &v) const
    {
        const std::size_t al = v.alloc ? v.alloc : v.level;
        return PolyArr{slot[(std::size_t)v.slot], 2 * al * c->N, al * c->N};
    }
    // mod_switch_to_next down to `level`: the same slot read at fewer limbs.  No copy and no launch; the checks are
    // mod_switch_to_next's, one per level
    MathVal down(const MathVal &v, std::size_t level) const
    {
        MathVal r = v;
        r.alloc = v.alloc ? v.alloc : v.level;
        for (std::size_t l = v.level; l > level; --l) need(ch.scale_ok(v.scale, l - 1), "scale out of bounds");
        r.level = std::min(v.level, level);
        return r;
    }

    // rescale(a (*) encode(cval, a.level, pscale)) [+- encode(dval) at the result's level and scale]: multiply_plain,
    // rescale_to_next, add_plain / sub_plain.  dmode 0 none, 1 add, 2 subtract; pscale 0: a's own scale; oscale
    // non-zero: the result's scale is assigned ("scale := oscale") before d is encoded
    MathVal cstage(const MathVal &a, double cval, int dmode = 0, double dval = 0, double pscale = 0, double oscale = 0)
    {
        const std::size_t l = a.level;
        u64 cw[HEC_MAXL + 1], dw[HEC_MAXL + 1];
        if (pscale == 0) pscale = a.scale;
        scalar_words_chain(ch, cval, pscale, l, cw);
        const double ns = a.scale * pscale;
        need(ch.scale_ok(ns, l), "scale out of bounds");
        if (l == 1) throw std::invalid_argument("end of modulus switching chain reached");
        MathVal o;
        o.level = l - 1;
        o.scale = oscale != 0 ? oscale : ns / (double)ch.q[l - 1];
        if (dmode) {
            scalar_words_chain(ch, dval, o.scale, o.level, dw);
            need(are_close(o.scale, o.scale), "scale mismatch");  // add_plain's check; the plaintext has o's scale
            if (dmode == 2)
                for (std::size_t i = 0; i < o.level; ++i) dw[i] = dw[i] ? ch.q[i] - dw[i] : 0;
        }
        o.slot = take();
        if (c) {
            const PolyArr pa = arr(a);
            const u64 sb = pa.sb, sk = pa.sk;
            const u64 *A = pa.p;
            {
                ProfScope k(*c, "k:k_math_lastprod/math", 4.0 * B);
                math_lastprod(*c, A, sb, sk, Y, B, 2, (int)l, cw[l - 1]);
            }
            stage_round_limbs(*c, Y, Z, B, (int)l, "k:k_ntt/math_intt", "k:k_ntt/math_round_a");
            {  // Z, the source's data limbs and the outputs, once each
                ProfScope k(*c, "k:k_ntt/math_cstage", 6.0 * B * (l - 1));
                math_cstage(*c, Z, A, sb, sk, arr(o), B, 2, (int)l, cw, dmode ? dw : nullptr);
            }
        }
        return o;
    }

    // rescale(relin(a (*) (b [+ encode(dval, b.level, b.scale)]))): add_plain, multiply / square, relinearize,
    // rescale_to_next.  a and b may be one value (the square)
    MathVal prod(const MathVal &a, const MathVal &b, bool has_d = false, double dval = 0)
    {
        u64 dw[HEC_MAXL + 1];
        if (has_d) {
            scalar_words_chain(ch, dval, b.scale, b.level, dw);
            need(are_close(b.scale, b.scale), "scale mismatch");  // add_plain's check; the plaintext has b's scale
        }
        need(a.level == b.level, "encrypted1 and encrypted2 parameter mismatch");
        const std::size_t l = a.level;
        const double ns = a.scale * b.scale;
        need(ch.scale_ok(ns, l), "scale out of bounds");
        if (l == 1) throw std::invalid_argument("end of modulus switching chain reached");
        MathVal o;
        o.level = l - 1;
        o.scale = ns / (double)ch.q[l - 1];
        o.slot = take();
        if (c) product_stage(*c, *s, arr(a), arr(b), has_d ? dw : nullptr, T3, rk, B, (int)l, arr(o));
        return o;
    }

    // a - b into a's slot (sub_inplace)
    void sub(MathVal &a, const MathVal &b)
    {
        need(a.level == b.level, "encrypted1 and encrypted2 parameter mismatch");
        need(are_close(a.scale, b.scale), "scale mismatch");
        if (c) ew_add(*c, arr(a), arr(b), arr(a), B, 2, (int)a.level, 1);
    }

    // a + b into a's slot (add_inplace)
    void add(MathVal &a, const MathVal &b)
    {
        need(a.level == b.level, "encrypted1 and encrypted2 parameter mismatch");
        need(are_close(a.scale, b.scale), "scale mismatch");
        if (c) ew_add(*c, arr(a), arr(b), arr(a), B, 2, (int)a.level, 0);
    }

    // a + encode(dval, a.level, a.scale) into a's slot (add_plain_inplace of a scalar)
    void add_const(MathVal &a, double dval)
    {
        u64 dw[HEC_MAXL + 1];
        scalar_words_chain(ch, dval, a.scale, a.level, dw);
        need(are_close(a.scale, a.scale), "scale mismatch");
        if (c) {
            ProfScope k(*c, "k:k_math_addconst/math", 2.0 * B * a.level);
            math_addconst(*c, arr(a), dw, B, (int)a.level);
        }
    }

    // ------------------------------------------------------------ poly: Paterson-Stockmeyer
    static std::size_t clog2(std::size_t j) { return j <= 1 ? 0 : 64 - (std::size_t)__builtin_clzll(j - 1); }
    using Coeffs = std::vector<double>;
    static void trim(Coeffs &p)
    {
        while (p.size() > 1 && p.back() == 0.0) p.pop_back();
    }
    static bool above0(const Coeffs &p)  // a non-zero coefficient above index 0
    {
        for (std::size_t j = 1; j < p.size(); ++j)
            if (p[j] != 0.0) return true;
        return false;
    }
    // g = bs 2^k, k the largest with g <= degree
    std::size_t split_at(const Coeffs &p) const
    {
        std::size_t g = bs;
        while (2 * g <= p.size() - 1) g *= 2;
        return g;
    }
    // the level a sub-polynomial's value can be had at (may go below 1: long arithmetic in a signed type)
    long long need_level(Coeffs p) const
    {
        trim(p);
        const long long l0 = (long long)x1.level;
        if (p.size() - 1 < bs) {
            long long v = l0;
            for (std::size_t j = 1; j < p.size(); ++j)
                if (p[j] != 0.0) v = std::min(v, l0 - (long long)clog2(j));
            return v - 1;
        }
        const std::size_t g = split_at(p);
        const Coeffs quo(p.begin() + (std::ptrdiff_t)g, p.end()), rem(p.begin(), p.begin() + (std::ptrdiff_t)g);
        long long v = l0 - (long long)clog2(g) - 1;
        if (above0(quo)) v = std::min(v, need_level(quo) - 1);
        if (above0(rem)) v = std::min(v, need_level(rem));
        return v;
    }
    // the uses of every power, by the steps and by the powers above it: a power leaves its slot after the last
    void count_use(std::size_t j)
    {
        if (j == 1) return;
        if (!uses.count(j)) {
            uses[j] = 0;
            count_use((j + 1) / 2);
            count_use(j / 2);
        }
        ++uses[j];
    }
    void count_eval(Coeffs p)
    {
        trim(p);
        if (p.size() - 1 < bs) {
            for (std::size_t j = 1; j < p.size(); ++j)
                if (p[j] != 0.0) count_use(j);
            return;
        }
        const std::size_t g = split_at(p);
        const Coeffs quo(p.begin() + (std::ptrdiff_t)g, p.end()), rem(p.begin(), p.begin() + (std::ptrdiff_t)g);
        count_use(g);
        if (above0(quo)) count_eval(quo);
        if (above0(rem)) count_eval(rem);
    }
    MathVal power(std::size_t j)
    {
        if (j == 1) return x1;
        auto it = pw.find(j);
        if (it != pw.end()) return it->second;
        const std::size_t a = (j + 1) / 2, b = j / 2;
        const MathVal A = power(a), Bv = power(b);
        const std::size_t lv = std::min(A.level, Bv.level);
        const MathVal r = prod(down(A, lv), down(Bv, lv));
        ++nprod;
        release(a);
        release(b);
        pw[j] = r;
        return r;
    }
    void release(std::size_t j)
    {
        if (j == 1) return;
        if (--uses[j] == 0) {
            drop(pw[j]);
            pw.erase(j);
        }
    }

    // Eval(p, Lt, St): a value at level Lt whose scale is St exactly
    MathVal eval(Coeffs p, std::size_t Lt, double St)
    {
        trim(p);
        const std::size_t e = p.size() - 1;
        if (e < bs) {  // leaf: one linear-combination stage
            const std::size_t l = Lt + 1, off = tab.size();
            const double T = St * (double)ch.q[Lt];
            std::vector<MathVal> v;
            std::vector<std::size_t> js;
            for (std::size_t j = 1; j <= e; ++j) {
                if (p[j] == 0.0) continue;
                const MathVal t = down(power(j), l);
                const double ps = T / t.scale;
                tab.resize(tab.size() + l);
                scalar_words_chain(ch, p[j], ps, l, tab.data() + tab.size() - l);
                need(ch.scale_ok(t.scale * ps, l), "scale out of bounds");
                if (!v.empty()) need(are_close(T, T), "scale mismatch");  // add's check: both scales were assigned T
                v.push_back(t);
                js.push_back(j);
            }
            const std::size_t doff = tab.size();
            for (const MathVal &t : v) {
                const std::size_t al = t.alloc ? t.alloc : t.level;
                tab.push_back((u64)t.slot * slot_words);
                tab.push_back(2 * al * ring);
                tab.push_back(al * ring);
            }
            u64 dw[HEC_MAXL + 1];
            MathVal o;
            o.level = Lt;
            o.scale = St;
            if (p[0] != 0.0) {
                scalar_words_chain(ch, p[0], St, Lt, dw);
                need(are_close(St, St), "scale mismatch");
            }
            o.slot = take();
            ++nleaf;
            if (c) {
                const int nt = (int)v.size();
                {  // nt sources' last limbs in, the sums out
                    ProfScope k(*c, "k:k_math_lincomb_last/math", 2.0 * (nt + 1) * B);
                    math_lincomb_last(*c, slot[0], tab_dev + off, tab_dev + doff, nt, Y, B, 2, (int)l);
                }
                stage_round_limbs(*c, Y, Z, B, (int)l, "k:k_ntt/math_intt", "k:k_ntt/math_round_a");
                {  // Z, every source's data limbs and the outputs, once each
                    ProfScope k(*c, "k:k_ntt/math_lincomb", 2.0 * (nt + 2) * B * (l - 1));
                    math_lincomb(*c, Z, slot[0], tab_dev + off, tab_dev + doff, nt, arr(o), B, 2, (int)l,
                                 p[0] != 0.0 ? dw : nullptr);
                }
            }
            for (std::size_t j : js) release(j);
            return o;
        }
        const std::size_t g = split_at(p);
        const Coeffs quo(p.begin() + (std::ptrdiff_t)g, p.end()), rem(p.begin(), p.begin() + (std::ptrdiff_t)g);
        const MathVal X = down(power(g), Lt + 1);
        const double qs = St * (double)ch.q[Lt] / X.scale;
        const bool rem_poly = above0(rem);
        MathVal r;
        if (above0(quo)) {
            MathVal Q = eval(quo, Lt + 1, qs);
            r = prod(Q, X);
            ++nprod;
            drop(Q);
            r.scale = St;
            if (!rem_poly && rem[0] != 0.0) add_const(r, rem[0]);
        } else {  // a constant quotient: the scalar stage, the remainder's constant folded into it
            const bool dc = !rem_poly && rem[0] != 0.0;
            r = cstage(X, quo[0], dc ? 1 : 0, dc ? rem[0] : 0.0, qs, St);
        }
        release(g);
        if (rem_poly) {
            MathVal R = eval(rem, Lt, St);
            add(r, R);
            drop(R);
        }
        return r;
    }

    // the whole schedule; x at slot 0.  coeffs trimmed and not constant, bs a power of two in [2, 16]
    MathVal poly(const Coeffs &coeffs, std::size_t bsize, std::size_t level, double scale)
    {
        busy.assign(1, 1);
        peak = 1;
        bs = bsize;
        nprod = nleaf = 0;
        pw.clear();
        uses.clear();
        tab.clear();
        x1 = MathVal{};
        x1.slot = 0;
        x1.level = level;
        x1.scale = scale;
        if (need_level(coeffs) < 1) throw std::invalid_argument("end of modulus switching chain reached");
        count_eval(coeffs);
        return eval(coeffs, (std::size_t)need_level(coeffs), scale);
    }

    // he_math.cpp:22-90
    MathVal signed_inv(const MathVal &x, double a, std::size_t iters)
    {
        MathVal y = cstage(x, -a * a, 1, 2 * a);
        if (iters == 1) return y;
        MathVal e = cstage(x, a, 2, 1.0);
        MathVal t = cstage(y, 1.0, 0, 0, e.scale);  // y drops one level with the plaintext 1 encoded for e
        drop(y);
        y = t;
        for (std::size_t i = 1; i < iters; ++i) {
            t = prod(e, e);
            drop(e);
            e = t;
            t = prod(y, e, true, 1.0);  // y (e^2 + 1)
            drop(y);
            y = t;
        }
        drop(e);
        return y;
    }

    // he_math.cpp:95-164 (the `#if 1` form)
    MathVal inv_sqrt_twice(const MathVal &x, double a, std::size_t iters)
    {
        const double y0 = a;
        MathVal xl = x;  // x, dropped alongside the iterate; the caller's value is never released here
        bool own = false;
        MathVal y = cstage(x, -y0 * y0 * y0, 1, 3.0 / 2 * y0);
        for (std::size_t i = 1; i < iters; ++i) {
            MathVal yp = y;
            MathVal t = cstage(yp, 3.0 / 2);
            y = cstage(t, 1.0);
            drop(t);
            for (std::size_t j = 0; j < (i > 1 ? 2u : 1u); ++j) {
                t = cstage(xl, 1.0);
                if (own) drop(xl);
                xl = t;
                own = true;
            }
            MathVal xy = prod(xl, yp);
            t = prod(yp, yp);
            drop(yp);
            yp = prod(t, xy);
            drop(t);
            drop(xy);
            sub(y, yp);
            drop(yp);
        }
        if (own) drop(xl);
        return y;
    }

    // he_math.cpp:211-232; the level difference in size_t, as he::util::reach_chain_level takes it
    MathVal sqrt(const MathVal &x, double a, std::size_t iters)
    {
        MathVal y = inv_sqrt_twice(x, 1 / a / std::sqrt(2), iters);
        MathVal sv = cstage(x, std::sqrt(2));
        const std::size_t n = (sv.level - 1) - (y.level - 1);
        for (std::size_t k = 0; k < n; ++k) {
            MathVal t = cstage(sv, 1.0);
            drop(sv);
            sv = t;
        }
        MathVal o = prod(y, sv);
        drop(y);
        drop(sv);
        return o;
    }

    // he_math.cpp:237-269
    MathVal abs(const MathVal &x, double a, std::size_t iters)
    {
        MathVal sq = prod(x, x);
        MathVal y = inv_sqrt_twice(sq, 1 / a / std::sqrt(2), iters);
        MathVal t = cstage(sq, std::sqrt(2));
        drop(sq);
        sq = t;
        const std::size_t n = (sq.level - 1) - (y.level - 1);
        for (std::size_t k = 0; k < n; ++k) {
            t = cstage(sq, 1.0);
            drop(sq);
            sq = t;
        }
        MathVal o = prod(y, sq);
        drop(y);
        drop(sq);
        return o;
    }

    // he_util.h:27-48
    MathVal drop_levels(const MathVal &x, std::size_t levels)
    {
        MathVal v = x;
        for (std::size_t k = 0; k < levels; ++k) {
            MathVal t = cstage(v, 1.0);
            if (k) drop(v);
            v = t;
        }
        return v;
    }

    // fn: HEC_MATH_*, or -1 for drop_levels with iters levels.  The input occupies slot 0
    MathVal run(int fn, double a, std::size_t iters, std::size_t level, double scale)
    {
        busy.assign(1, 1);
        peak = 1;
        MathVal x;
        x.slot = 0;
        x.level = level;
        x.scale = scale;
        switch (fn) {
        case -1: return drop_levels(x, iters);
        case HEC_MATH_SIGNED_INV: return signed_inv(x, a, iters);
        case HEC_MATH_INV_SQRT_TWICE: return inv_sqrt_twice(x, a, iters);
        case HEC_MATH_SQRT: return sqrt(x, a, iters);
        case HEC_MATH_ABS: return abs(x, a, iters);
        default: throw std::invalid_argument("unknown he::math function");
        }
    }
};

void math_batch(hec_context *ctx, int fn, const hec_ciphertext *const *x, uint64_t B, double a, uint64_t iters,
                const hec_kswitch_key *rk, hec_ciphertext *const *out)
{
    need(ctx && x && out && B >= 1, "null argument");
    set_device(ctx);
    check_uniform_batch(ctx, x, out, B);
    if (fn >= 0) {
        need(iters >= 1, "iter_num must be positive");
        check_obj(ctx, rk, BAD_RK);
    }
    Ctx &c = ctx->c;
    const std::size_t N = c.N, l0 = x[0]->level, S0 = 2 * l0 * N;
    MathRun plan;
    plan.ch = Chain{c.q.data(), c.L};
    const MathVal res = plan.run(fn, a, iters, l0, x[0]->scale);
    if (res.slot == 0) return;  // no level to drop: the inputs are the results
    const std::size_t Bc = batch_chunk(c, l0, B);
    const std::size_t nslot = (std::size_t)plan.peak;
    Scratch s(c, nslot * Bc * S0 + Bc * 3 * l0 * N + 2 * Bc * N + 2 * Bc * l0 * N + ks_words(c, Bc, l0) +
                     rescale_words(c, Bc, 2, l0) + (nslot + 16) * 64);
    MathRun dev;
    dev.ch = plan.ch;
    dev.c = &c;
    dev.s = &s;
    dev.rk = rk ? rk->d : nullptr;
    for (std::size_t i = 0; i < nslot; ++i) dev.slot.push_back(s.take(Bc * S0));
    dev.T3 = s.take(Bc * 3 * l0 * N);
    dev.Y = s.take(2 * Bc * N);
    dev.Z = s.take(2 * Bc * l0 * N);
    const std::size_t So = 2 * res.level * N;
    for (std::size_t b0 = 0; b0 < B; b0 += Bc) {
        const std::size_t cnt = std::min(Bc, B - b0);
        dev.B = (int)cnt;
        for (std::size_t b = 0; b < cnt; ++b) d2d(c, dev.slot[0] + b * S0, x[b0 + b]->d, S0);
        const MathVal r = dev.run(fn, a, iters, l0, x[0]->scale);
        for (std::size_t b = 0; b < cnt; ++b)
            store_ct(c, out[b0 + b], dev.slot[(std::size_t)r.slot] + b * So, 2, r.level, r.scale);
    }
}

// hec_math_poly's argument checks, shared with hec_math_poly_plan: the trimmed coefficients and the block size
std::size_t poly_args(const double *coeffs, uint64_t degree, uint64_t bs, std::vector<double> &p)
{
    need(coeffs, "null argument");
    need(degree < 65536, "degree must be below 2^16");
    p.assign(coeffs, coeffs + degree + 1);
    for (double v : p) need(std::isfinite(v), "coefficients must be finite");
    MathRun::trim(p);
    need(p.size() >= 2, "polynomial must not be constant");
    if (bs == 0) {
        const std::size_t m = std::min<std::size_t>(4, std::max<std::size_t>(1, (MathRun::clog2(p.size()) + 1) / 2));
        bs = uint64_t(1) << m;
    }
    need(bs >= 2 && bs <= 16 && !(bs & (bs - 1)), "bs must be a power of two in [2, 16]");
    return (std::size_t)bs;
}

void poly_batch(hec_context *ctx, const hec_ciphertext *const *x, uint64_t B, const double *coeffs, uint64_t degree,
                uint64_t bs, const hec_kswitch_key *rk, hec_ciphertext *const *out)
{
    need(ctx && x && out && B >= 1, "null argument");
    set_device(ctx);
    check_uniform_batch(ctx, x, out, B);
    check_obj(ctx, rk, BAD_RK);
    std::vector<double> p;
    const std::size_t bse = poly_args(coeffs, degree, bs, p);
    Ctx &c = ctx->c;
    const std::size_t N = c.N, l0 = x[0]->level, S0 = 2 * l0 * N;
    const std::size_t Bc = batch_chunk(c, l0, B);
    MathRun plan;
    plan.ch = Chain{c.q.data(), c.L};
    plan.ring = N;
    plan.slot_words = Bc * S0;  // a multiple of 64: the carves below are back to back
    const MathVal res = plan.poly(p, bse, l0, x[0]->scale);
    const std::size_t nslot = (std::size_t)plan.peak, ntab = std::max<std::size_t>(plan.tab.size(), 1);
    Scratch s(c, nslot * Bc * S0 + Bc * 3 * l0 * N + 2 * Bc * N + 2 * Bc * l0 * N + ks_words(c, Bc, l0) +
                     rescale_words(c, Bc, 2, l0) + ntab + (nslot + 17) * 64);
    MathRun dev;
    dev.ch = plan.ch;
    dev.c = &c;
    dev.s = &s;
    dev.rk = rk->d;
    dev.ring = N;
    dev.slot_words = plan.slot_words;
    for (std::size_t i = 0; i < nslot; ++i) {
        dev.slot.push_back(s.take(Bc * S0));
        if (dev.slot[i] != dev.slot[0] + i * plan.slot_words) throw std::logic_error("he::math slots are not contiguous");
    }
    dev.T3 = s.take(Bc * 3 * l0 * N);
    dev.Y = s.take(2 * Bc * N);
    dev.Z = s.take(2 * Bc * l0 * N);
    // every leaf's coefficient words, once per call, ahead of the first pass on the context's stream
    u64 *tabd = s.take(ntab);
    if (!plan.tab.empty()) {
        HEC_HIP(hipMemcpyAsync(tabd, plan.tab.data(), plan.tab.size() * sizeof(u64), hipMemcpyHostToDevice, c.stream));
        HEC_HIP(hipStreamSynchronize(c.stream));  // the copy has left the host table before anything can throw
    }
    dev.tab_dev = tabd;
    const std::size_t So = 2 * res.level * N;
    for (std::size_t b0 = 0; b0 < B; b0 += Bc) {
        const std::size_t cnt = std::min(Bc, B - b0);
        dev.B = (int)cnt;
        for (std::size_t b = 0; b < cnt; ++b) d2d(c, dev.slot[0] + b * S0, x[b0 + b]->d, S0);
        const MathVal r = dev.poly(p, bse, l0, x[0]->scale);
        for (std::size_t b = 0; b < cnt; ++b)
            store_ct(c, out[b0 + b], dev.slot[(std::size_t)r.slot] + b * So, 2, r.level, r.scale);
    }
}
}  // namespace

int hec_math_poly_plan(const uint64_t *coeff_modulus, uint64_t K, const double *coeffs, uint64_t degree, uint64_t bs,
                       uint64_t level, double scale, uint64_t *out_level, double *out_scale, uint64_t *bs_eff,
                       uint64_t *products, uint64_t *leaves)
{
    return guard([&] {
        need(coeff_modulus && out_level && out_scale && bs_eff && products && leaves, "null argument");
        need(K >= 2 && K - 1 <= HEC_MAXL, "coeff_modulus size is not valid");
        need(level >= 1 && level <= K - 1, BAD_CT);
        std::vector<double> p;
        const std::size_t bse = poly_args(coeffs, degree, bs, p);
        MathRun plan;
        plan.ch = Chain{coeff_modulus, (std::size_t)(K - 1)};
        const MathVal r = plan.poly(p, bse, level, scale);
        *out_level = r.level;
        *out_scale = r.scale;
        *bs_eff = bse;
        *products = plan.nprod;
        *leaves = plan.nleaf;
    });
}

int hec_math_poly(hec_context *ctx, const hec_ciphertext *const *x, uint64_t B, const double *coeffs, uint64_t degree,
                  uint64_t bs, const hec_kswitch_key *rk, hec_ciphertext *const *out)
{
    return guard([&] { poly_batch(ctx, x, B, coeffs, degree, bs, rk, out); });
}

int hec_math_plan(const uint64_t *coeff_modulus, uint64_t K, int fn, double a, uint64_t iter_num, uint64_t level,
                  double scale, uint64_t *out_level, double *out_scale)
{
    return guard([&] {
        need(coeff_modulus && out_level && out_scale, "null argument");
        need(K >= 2 && K - 1 <= HEC_MAXL, "coeff_modulus size is not valid");
        need(fn >= HEC_MATH_SIGNED_INV && fn <= HEC_MATH_ABS, "unknown he::math function");
        need(level >= 1 && level <= K - 1, BAD_CT);
        need(iter_num >= 1, "iter_num must be positive");
        MathRun plan;
        plan.ch = Chain{coeff_modulus, (std::size_t)(K - 1)};
        const MathVal r = plan.run(fn, a, iter_num, level, scale);
        *out_level = r.level;
        *out_scale = r.scale;
    });
}

int hec_math_signed_inv(hec_context *ctx, const hec_ciphertext *const *x, uint64_t B, double a, uint64_t iter_num,
                        const hec_kswitch_key *rk, hec_ciphertext *const *out)
{
    return guard([&] { math_batch(ctx, HEC_MATH_SIGNED_INV, x, B, a, iter_num, rk, out); });
}
int hec_math_inv_sqrt_twice(hec_context *ctx, const hec_ciphertext *const *x, uint64_t B, double a, uint64_t iter_num,
                            const hec_kswitch_key *rk, hec_ciphertext *const *out)
{
    return guard([&] { math_batch(ctx, HEC_MATH_INV_SQRT_TWICE, x, B, a, iter_num, rk, out); });
}
int hec_math_sqrt(hec_context *ctx, const hec_ciphertext *const *x, uint64_t B, double a, uint64_t iter_num,
                  const hec_kswitch_key *rk, hec_ciphertext *const *out)
{
    return guard([&] { math_batch(ctx, HEC_MATH_SQRT, x, B, a, iter_num, rk, out); });
}
int hec_math_abs(hec_context *ctx, const hec_ciphertext *const *x, uint64_t B, double a, uint64_t iter_num,
                 const hec_kswitch_key *rk, hec_ciphertext *const *out)
{
    return guard([&] { math_batch(ctx, HEC_MATH_ABS, x, B, a, iter_num, rk, out); });
}
int hec_drop_chain_levels(hec_context *ctx, hec_ciphertext *const *cts, uint64_t B, uint64_t levels)
{
    return guard([&] { math_batch(ctx, -1, cts, B, 0.0, levels, nullptr, cts); });
}

// ------------------------------------------------------------------ he::linalg over many ciphertexts ------
// Matrix::operator*=, BatchedMatrix::operator*= / square_inplace / sum_bvec_elems_inplace (reference
// src/core/he_linalg.cpp) as stages over a batch.  The entries are grouped by level on the host (as dec_run groups
// its inputs); a group's inputs are gathered into Scratch slots once, its stages run over the whole group (in passes
// of at most 65,535 / ((l + 1) l) entries, as math_batch), and the outputs are scattered after the last stage.  Scales
// are per entry and host bookkeeping only.
namespace {
struct LinalgPlan {  // class members: no C language linkage inside the C-ABI block
// the caller's entries by level (ascending), the caller's order kept inside a level
static std::map<std::size_t, std::vector<std::size_t>> by_level(const hec_ciphertext *const *x, uint64_t B)
{
    std::map<std::size_t, std::vector<std::size_t>> g;
    for (uint64_t i = 0; i < B; ++i) g[x[i]->level].push_back(i);
    return g;
}
};

// The schedule of BatchedVector::sum_elems_inplace (he_linalg.cpp:667-713), written once over three operations on
// slots of one Scratch workspace: rot, add and drop.  As MathRun, a call walks it twice: first without a device side
// (the plan: the rotation steps in order, whose keys the call requires before anything is written, and the peak
// number of live slots), then on the device over a pass of B ciphertexts at level l.  hec_sum_elems_plan is the first
// walk alone.
struct SumRun {
    // device side; c == nullptr is the planning walk
    Ctx *c = nullptr;
    Scratch *s = nullptr;
    const hec_galois_keys *gk = nullptr;
    int B = 0, l = 0;
    std::vector<u64 *> slot;
    // the same on both walks
    std::vector<int> steps;  // every rotation's step, in order
    std::vector<char> busy;
    int peak = 0;

    PolyArr arr(int i) const { return PolyArr{slot[(std::size_t)i], 2 * (u64)l * c->N, (u64)l * c->N}; }
    void drop(int i) { busy[(std::size_t)i] = 0; }

    // rotate(src, step) [+ addend] into a free slot: a rotation's reads gather, so it cannot run in place, and an
    // accumulate step reads its addend at the words it writes.  discard: the reference rotates and throws the result
    // away (dim = 1), so the step's key is required, nothing is launched and src stands
    int rot(int src, int step, int addend, bool discard = false)
    {
        steps.push_back(step);
        if (discard) return src;
        std::size_t dst = 0;
        while (dst < busy.size() && busy[dst]) ++dst;
        if (dst == busy.size()) busy.push_back(0);
        busy[dst] = 1;
        peak = std::max(peak, (int)dst + 1);
        if (c) {
            const u32 e = elt_from_step(*c, step);
            galois_ks(*c, *s, arr(src), arr((int)dst), B, l, e, gk->keys.at(e), addend >= 0 ? arr(addend) : PolyArr{});
        }
        return (int)dst;
    }
    // r += p (bvec += partial)
    void add(int r, int p)
    {
        if (!c) return;
        ProfScope k(*c, "k:k_ew_add/sum", 6.0 * B * l);
        ew_add(*c, arr(r), arr(p), arr(r), B, 2, l, 0);
    }

    // bvec (r), to_sum (t) and the partial sums as slots; the input occupies slot 0, the result's slot is returned
    int run(uint64_t dim)
    {
        need(dim >= 1, "dim must be positive");
        need(dim < (1ull << 31), "step count too large");  // `window` is an int
        steps.clear();
        busy.assign(1, 1);
        peak = 1;
        int r = 0, t = 0;
        bool have = false;  // bvec holds a term already
        int window = 1;
        if (dim & 1) {
            have = true;
            t = rot(t, window, -1, dim == 1);
        }
        for (uint64_t bits = dim >> 1; bits != 0; bits >>= 1) {
            window <<= 1;
            if (!(bits & 1)) continue;
            int st = window >> 1;
            int acc = rot(t, st, t);  // acc = to_sum + (to_sum << st)
            if (!have && r != t) drop(r);
            for (st >>= 1; st != 0; st >>= 1) {  // acc += acc << st
                const int n = rot(acc, st, acc);
                drop(acc);
                acc = n;
            }
            if (have) {
                add(r, acc);
                drop(acc);
            } else {
                r = acc;
                have = true;
            }
            if (bits != 1) {
                const int n = rot(t, window, -1);
                if (t != r) drop(t);
                t = n;
            }
        }
        return r;
    }
};

void product_many(hec_context *ctx, const hec_ciphertext *const *a, const hec_ciphertext *const *b, uint64_t B,
                  const hec_kswitch_key *rk, hec_ciphertext *const *out)
{
    need(ctx != nullptr, "context is null");
    if (B == 0) return;
    need(a && b && out, "null argument");
    set_device(ctx);
    Ctx &c = ctx->c;
    for (uint64_t i = 0; i < B; ++i) {  // multiply / square, relinearize, rescale_to_next on entry i
        check_ct(ctx, a[i]);
        check_ct(ctx, b[i]);
        check_obj(ctx, out[i], BAD_CT);
        need(a[i]->size == 2 && b[i]->size == 2, "encrypted size must be 2");
        need(a[i]->level == b[i]->level, "encrypted1 and encrypted2 parameter mismatch");
        need(scale_ok(c, a[i]->scale * b[i]->scale, a[i]->level), "scale out of bounds");
        check_obj(ctx, rk, BAD_RK);
        if (a[i]->level == 1) throw std::invalid_argument("end of modulus switching chain reached");
    }
    check_out_alias({a, b}, out, B);
    const std::size_t N = c.N;
    const auto groups = LinalgPlan::by_level(a, B);
    std::size_t words = 0;
    for (const auto &g : groups) {
        const std::size_t l = g.first, Bc = batch_chunk(c, l, g.second.size());
        words = std::max(words, Bc * (2 * 2 * l * N + 2 * (l - 1) * N + 3 * l * N) + ks_words(c, Bc, l) +
                                    rescale_words(c, Bc, 2, l) + 8 * 64);
    }
    Scratch s(c, words);
    for (const auto &g : groups) {
        const std::size_t l = g.first, S0 = 2 * l * N, So = 2 * (l - 1) * N, Bc = batch_chunk(c, l, g.second.size());
        s.top = 0;
        u64 *A = s.take(Bc * S0), *Bp = s.take(Bc * S0), *O = s.take(Bc * So), *T3 = s.take(Bc * 3 * l * N);
        for (std::size_t b0 = 0; b0 < g.second.size(); b0 += Bc) {
            const std::size_t cnt = std::min(Bc, g.second.size() - b0);
            bool same = true;
            for (std::size_t k = 0; k < cnt; ++k) {
                const std::size_t i = g.second[b0 + k];
                d2d(c, A + k * S0, a[i]->d, S0);
                same = same && a[i] == b[i];
            }
            if (!same)
                for (std::size_t k = 0; k < cnt; ++k) d2d(c, Bp + k * S0, b[g.second[b0 + k]]->d, S0);
            const PolyArr Aa{A, S0, l * N};
            product_stage(c, s, Aa, same ? Aa : PolyArr{Bp, S0, l * N}, nullptr, T3, rk->d, (int)cnt, (int)l,
                          PolyArr{O, So, (l - 1) * N});
            for (std::size_t k = 0; k < cnt; ++k) {
                const std::size_t i = g.second[b0 + k];
                // out[i] may be a[i] or b[i]: the scales are read before the store
                store_ct(c, out[i], O + k * So, 2, l - 1, a[i]->scale * b[i]->scale / (double)c.q[l - 1]);
            }
        }
    }
}

void sum_elems_many(hec_context *ctx, const hec_ciphertext *const *x, uint64_t B, uint64_t dim,
                    const hec_galois_keys *gk, hec_ciphertext *const *out)
{
    need(ctx != nullptr, "context is null");
    if (B == 0) return;
    need(x && out, "null argument");
    set_device(ctx);
    Ctx &c = ctx->c;
    SumRun plan;
    plan.run(dim);
    for (uint64_t i = 0; i < B; ++i) {  // the schedule's first rotation on entry i, then (once) the others' keys
        check_ct(ctx, x[i]);
        check_obj(ctx, out[i], BAD_CT);
        check_obj(ctx, gk, BAD_GK);
        need(x[i]->size == 2, "encrypted size must be 2");
        if (i == 0)
            for (int st : plan.steps)  // powers of two: no NAF decomposition stands in for an absent key
                need(gk->keys.count(elt_from_step(c, st)) > 0, "Galois key not present");
        need(dim == 1 || are_close(x[i]->scale, x[i]->scale), "scale mismatch");  // the adds' check
    }
    check_out_alias({x}, out, B);
    const std::size_t N = c.N, nslot = (std::size_t)plan.peak;
    const auto groups = LinalgPlan::by_level(x, B);
    std::size_t words = 0;
    for (const auto &g : groups) {
        const std::size_t l = g.first, Bc = batch_chunk(c, l, g.second.size());
        words = std::max(words, nslot * Bc * 2 * l * N + 2 * Bc * l * N + ks_words(c, Bc, l) + (nslot + 4) * 64);
    }
    Scratch s(c, words);
    SumRun dev;
    dev.c = &c;
    dev.s = &s;
    dev.gk = gk;
    for (const auto &g : groups) {
        const std::size_t l = g.first, S0 = 2 * l * N, Bc = batch_chunk(c, l, g.second.size());
        s.top = 0;
        dev.l = (int)l;
        dev.slot.clear();
        for (std::size_t i = 0; i < nslot; ++i) dev.slot.push_back(s.take(Bc * S0));
        for (std::size_t b0 = 0; b0 < g.second.size(); b0 += Bc) {
            dev.B = (int)std::min(Bc, g.second.size() - b0);
            for (int k = 0; k < dev.B; ++k) d2d(c, dev.slot[0] + k * S0, x[g.second[b0 + k]]->d, S0);
            const int r = dev.run(dim);
            for (int k = 0; k < dev.B; ++k) {
                const std::size_t i = g.second[b0 + k];
                store_ct(c, out[i], dev.slot[(std::size_t)r] + k * S0, 2, l, x[i]->scale);  // out[i] may be x[i]
            }
        }
    }
}
}  // namespace

int hec_multiply_relin_rescale_many(hec_context *ctx, const hec_ciphertext *const *a, const hec_ciphertext *const *b,
                                    uint64_t B, const hec_kswitch_key *rk, hec_ciphertext *const *out)
{
    return guard([&] { product_many(ctx, a, b, B, rk, out); });
}
int hec_sum_elems_many(hec_context *ctx, const hec_ciphertext *const *x, uint64_t B, uint64_t dim,
                       const hec_galois_keys *gk, hec_ciphertext *const *out)
{
    return guard([&] { sum_elems_many(ctx, x, B, dim, gk, out); });
}
int hec_sum_elems_plan(uint64_t dim, int *steps, uint64_t cap, uint64_t *count)
{
    return guard([&] {
        need(count != nullptr && (steps != nullptr || cap == 0), "null argument");
        SumRun plan;
        plan.run(dim);
        const std::vector<int> &st = plan.steps;
        *count = st.size();
        for (std::size_t i = 0; i < st.size() && i < cap; ++i) steps[i] = st[i];
    });
}

}  // extern "C"
