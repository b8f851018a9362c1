// The multi-GPU half of the CKKS engine (one process per GPU): the diagonal planner, RCCL loaded on first use and the
// two communicators behind HecComm (hec_host.h), the agreement step of the sharded matvec, and the C-ABI of
// hec_plan_diagonal_shards, hec_comm_*, hec_shard_agree, hec_context_comm and hec_matmul_diag_col_sharded.  The only
// file that includes rccl/rccl.h and dlfcn.h; hec_context_destroy deletes the communicator through HecComm.
#include <algorithm>
#include <cstring>
#include <limits>
#include <mutex>
#include <set>

#include "hec_engine.h"

#include <dlfcn.h>
#include <rccl/rccl.h>

using namespace hec;

namespace {

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

// =============================================================================== C-ABI =====
extern "C" {

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

}  // extern "C"
