// Host-side internals shared by the engine's files (hec_engine.hip: context, objects, primitives; hec_keyswitch.hip:
// the key switch; hec_matvec.hip: the he::linalg drivers; hec_shard.hip: the multi-GPU calls; hec_client.hip: encode,
// decode, keygen, encrypt; hec_evaluator.hip: the one-object calls; what crosses between those alone is in
// hec_engine.h) and hec_batched.hip (he::fft, he::math and he::linalg over many ciphertexts): the device objects behind
// the C-ABI's opaque types, the error guard, the workspace carver, the profile scope, and declarations of the engine's
// building blocks that the batched layers are written over (defined in hec_engine.hip, hec_keyswitch.hip and
// hec_client.hip).
#pragma once
#include <cmath>
#include <cstddef>
#include <exception>
#include <map>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "hec_internal.h"
#include "hecdna.h"

// =============================================================================== objects ===
// The communicator of the sharded matvec (one process per GPU): RCCL over xGMI (hec_comm_init) or a caller's host
// collectives (hec_comm_init_ops).  shard_agree needs only allreduce_f64; the data exchange sums the ranks' partial
// accumulators in u64.
struct HecComm {
    virtual ~HecComm() = default;
    // in place over the world, host memory: op HEC_REDUCE_MIN / HEC_REDUCE_MAX
    virtual void allreduce_f64(double *host, std::size_t n, int op, hipStream_t s) = 0;
    // in place over the world, a device buffer ordered on stream s: the sum (exact: world <= 8, residues < 2^60)
    virtual void allreduce_u64_sum(u64 *dev, std::size_t n, hipStream_t s) = 0;
};
struct hec_context {
    hec::Ctx c;
    // batch lanes (matvec_lanes): contexts sharing this one's device tables, each with its own HIP
    // stream, workspace and zero flag, built on first use
    std::vector<hec_context *> lanes;
    // persistent events of matvec_lanes (created with the first lane, destroyed with the context): the lanes
    // wait on lanes_start, the context stream waits on each lane's lane_done.  An event destroyed right after
    // a hipStreamWaitEvent on it could let that wait pass early (a rare whole-lane race seen at full size).
    hipEvent_t lanes_start = nullptr, lane_done = nullptr;
    // multi-GPU (hec_comm_init): this process's rank in a world of one process per GPU, RCCL communicator
    int rank = 0, world = 1;
    HecComm *comm = nullptr;
    u64 gen = 0;  // this context's entry in the live-context registry (hec_live.h)
};
// Every device object records its context by address and generation (hec_live.h) and its device, so that its destroy
// can free its memory after the context is gone.  bind() is the only place that sets these.
struct DevObject {
    hec_context *ctx = nullptr;
    u64 ctx_gen = 0;
    int device = 0;
};
struct hec_ciphertext : DevObject {
    u64 *d = nullptr;
    std::size_t cap = 0;  // words
    std::size_t size = 0, level = 0;
    double scale = 1.0;
};
struct hec_plaintext : DevObject {
    u64 *d = nullptr;
    std::size_t cap = 0;
    std::size_t level = 0;
    double scale = 1.0;
};
struct hec_kswitch_key : DevObject {
    u64 *d = nullptr;
};
struct hec_secret_key : DevObject {  // seal::SecretKey: u64[K][N], NTT form, key level
    u64 *d = nullptr;
    std::size_t words = 0;
};
struct hec_public_key : DevObject {  // seal::PublicKey: u64[2][K][N], NTT form, key level
    u64 *d = nullptr;
};
struct hec_galois_keys : DevObject {
    std::map<u32, u64 *> keys;
    std::map<u32, u64 *> negw;  // hoisted mod-up: W_elt[I] = NTT_I(sign mask of elt), built on first use
    // hoisted MAC: KW[elt, l][k][I] = sum_{J<l, J!=I} (q_J mod q_I) key_elt[J][k][I] mod q_I, built on first
    // use per level, dropped when the key is replaced
    std::map<std::pair<u32, int>, u64 *> kw;
    std::map<u32, u64 *> mkey;  // hoisted MAC: the key in MAC form and source order (mac_key_table), first use
    void drop_kw(u32 elt)  // the tables derived from the key's words (KW at every level, MK)
    {
        if (auto m = mkey.find(elt); m != mkey.end()) {
            (void)hipFree(m->second);
            mkey.erase(m);
        }
        for (auto it = kw.begin(); it != kw.end();) {
            if (it->first.first == elt) {
                (void)hipFree(it->second);
                it = kw.erase(it);
            } else {
                ++it;
            }
        }
    }
};

namespace hec {

extern thread_local std::string g_err;  // the calling thread's last error (hec_last_error); defined in hec_engine.hip

template <class F>
int guard(F &&f)
{
    try {
        f();
        return HEC_OK;
    } catch (const HipError &e) {
        g_err = e.what();
        return HEC_EDEVICE;
    } catch (const std::invalid_argument &e) {
        g_err = e.what();
        return HEC_EINVAL;
    } catch (const std::logic_error &e) {
        g_err = e.what();
        return HEC_ELOGIC;
    } catch (const std::exception &e) {
        g_err = e.what();
        return HEC_EDEVICE;
    }
}

inline void need(bool cond, const char *msg)
{
    if (!cond) throw std::invalid_argument(msg);
}

// SEAL's is_valid_for messages, one per object kind
constexpr const char *BAD_CT = "encrypted is not valid for encryption parameters";
constexpr const char *BAD_PLAIN = "plain is not valid for encryption parameters";
constexpr const char *BAD_SK = "secret key is not valid for encryption parameters";
constexpr const char *BAD_PK = "public key is not valid for encryption parameters";
constexpr const char *BAD_RK = "relin_keys is not valid for encryption parameters";
constexpr const char *BAD_GK = "galois_keys is not valid for encryption parameters";

// stack-style carving of the context workspace; kernels are stream ordered, so a region released
// here may be reused by the next enqueued operation.
struct Scratch {
    Ctx &c;
    std::size_t top = 0;
    explicit Scratch(Ctx &cc, std::size_t words) : c(cc)
    {
        c.ws.reserve(words, c.stream);
        ++c.ws.depth;
    }
    ~Scratch()
    {
        if (--c.ws.depth == 0 && !c.ws.defer_free && !c.ws.retired.empty()) {
            try {
                c.ws.reclaim(c.stream);
            } catch (...) {  // keep them for release(); a destructor must not throw
            }
        }
    }
    Scratch(const Scratch &) = delete;
    Scratch &operator=(const Scratch &) = delete;
    u64 *take(std::size_t w)
    {
        w = (w + 63) & ~(std::size_t)63;
        if (top + w > c.ws.words) throw std::logic_error("workspace overflow");
        u64 *p = c.ws.base + top;
        top += w;
        if (c.poison) dev_fill(c, p, 0xFFFFFFFFu, w * sizeof(u64));
        return p;
    }
};

// Per-class GPU time of the engine's phases.  prof_mode 1: event pair + synchronize per scope;
// prof_mode 2: event pairs from a reusable pool recorded asynchronously (no host sync inside the
// call), resolved when the profile is read.
struct ProfScope {
    Ctx &c;
    const char *name;
    double bytes = 0;
    int kl = 1;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipEvent_t pool_event()
    {
        if (c.ev_used == c.ev_pool.size()) {
            hipEvent_t e;
            HEC_HIP(hipEventCreate(&e));
            c.ev_pool.push_back(e);
        }
        return c.ev_pool[c.ev_used++];
    }
    ProfScope(Ctx &cc, const char *n, double limbs = 0, int launches = 1)
        : c(cc), name(n), bytes(limbs * 8.0 * (double)cc.N), kl(launches)
    {
        if (!c.prof_mode) return;
        if (c.prof_mode == 2) {
            e0 = pool_event();
            e1 = pool_event();
        } else {
            HEC_HIP(hipEventCreate(&e0));
            HEC_HIP(hipEventCreate(&e1));
        }
        HEC_HIP(hipEventRecord(e0, c.stream));
    }
    ~ProfScope()
    {
        if (!c.prof_mode || !e0) return;
        (void)hipEventRecord(e1, c.stream);
        if (c.prof_mode == 2) {
            c.prof_pend.push_back({name, e0, e1, bytes, kl});
            return;
        }
        (void)hipEventSynchronize(e1);
        float ms = 0;
        (void)hipEventElapsedTime(&ms, e0, e1);
        auto &r = c.prof_tab[name];
        r.ms += ms;
        r.n += 1;
        r.bytes += bytes;
        r.kl += kl;
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
    }
};

// The data primes of a modulus chain on the host: what the scalar encoder and the scale checks need, with or without a
// device context (hec_math_plan has none)
struct Chain {
    const u64 *q = nullptr;
    std::size_t L = 0;
    int total_bits(std::size_t level) const
    {
        int b = 0;
        for (std::size_t i = 0; i < level; ++i) b += 64 - __builtin_clzll(q[i]);
        return b;
    }
    bool scale_ok(double scale, std::size_t level) const  // SEAL is_scale_within_bounds
    {
        return !(scale <= 0 || (int)std::log2(scale) >= total_bits(level));
    }
};

// ------------------------------------------------------------------ building blocks (hec_engine.hip, hec_keyswitch.hip,
// hec_client.hip)
// Only what hec_batched.hip calls.  keyswitch(), rescale_batch(), grow() and make() stay private to the engine (they
// cross its files through hec_engine.h): the batched layers reach them through galois_ks(), relin_rescale() and
// store_ct().
void set_device(hec_context *ctx);
// Calls that take a context: the object must belong to this very context
void check_obj(const hec_context *ctx, const DevObject *o, const char *msg);
void check_ct(const hec_context *ctx, const hec_ciphertext *a);
// The output-alias rule: out[i] may be entry i's own inputs ins[k][i]; an output listed twice, one that
// is another entry's input, or one of the n_never objects of `never` (inputs that every entry reads) is refused: an
// output written by one pass must not be an input that a later pass gathers.  ctx non-null: every out[i] is checked as
// an object of ctx in the loop of the duplicate test, so out = [x, x, invalid] answers "alias"
void check_out_alias(const std::vector<const hec_ciphertext *const *> &ins, hec_ciphertext *const *out, uint64_t B,
                     const hec_context *ctx = nullptr, const hec_ciphertext *const *never = nullptr,
                     uint64_t n_never = 0);
void d2d(Ctx &c, void *dst, const void *src, std::size_t words);
// the one output store: grow(o), copy size * level * N words from src, set o's size, level and scale
void store_ct(Ctx &c, hec_ciphertext *o, const u64 *src, std::size_t size, std::size_t level, double scale);
// workspace words of a key switch of B targets at level l, and of a rescale of B entries of nk polys
std::size_t ks_words(const Ctx &c, std::size_t B, std::size_t l);
std::size_t rescale_words(const Ctx &c, std::size_t B, std::size_t nk, std::size_t l);
// OUT = key switch of apply_galois(X, elt) [+ ADD] over B size-2 entries at level l
void galois_ks(Ctx &c, Scratch &s, PolyArr X, PolyArr OUT, int B, int l, u32 elt, const u64 *key,
               PolyArr ADD = PolyArr{});
// relinearize the B size-3 entries A3 ([B][3][l][N]) in place, then rescale them into OUT at level l - 1
void relin_rescale(Ctx &c, Scratch &s, u64 *A3, const u64 *rk, int B, int l, PolyArr OUT,
                   const char *relin_scope = nullptr);
bool scale_ok(const Ctx &c, double scale, std::size_t level);  // SEAL is_scale_within_bounds
bool are_close(double a, double b);                            // SEAL util::are_close
u32 elt_from_step(const Ctx &c, int step);                     // SEAL GaloisTool::get_elt_from_step
// SEAL Evaluator::rotate_internal flattened into the sequence of Galois elements it applies
void rotation_elts(const Ctx &c, int steps, const hec_galois_keys &gk, std::vector<u32> &out);
u32 brev(u32 x, int bits);
void encoder_tables(Ctx &c);  // the GPU encoder's host tables, built once per context
// SEAL 4.1 CKKSEncoder::encode_internal(double value, ...) up to its fill: the checks and the word of every limb
void scalar_words(const Ctx &c, double value, double scale, std::size_t level, u64 *words);
void scalar_words_chain(const Chain &c, double value, double scale, std::size_t level, u64 *words);

}  // namespace hec
