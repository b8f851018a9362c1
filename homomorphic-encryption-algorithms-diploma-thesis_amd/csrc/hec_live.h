// The live-context registry (plain C++, no device code): which contexts exist, and the one way to touch a context
// from an object that may have outlived it.
//
// Objects may outlive their context (SEAL's objects hold their context by shared_ptr, so a caller may free them in
// any order, and a garbage collector finalising a reference cycle picks its own order and its own thread): every
// object records its context's address and generation.  An address reused by a later context carries a new
// generation, so it is never mistaken for the old one.
//
// Locking rule: while_alive(ctx, gen, f) runs f with the registry locked, and ctx_unregister takes the same lock, so
// a context's destroy waits for a running f and no later f sees that context.  The lock is not recursive: f must not
// create, destroy or check any context or object (it drains a stream, nothing more), and no caller holds the lock
// when it reaches a destroy (the failure paths of the constructors and the key loader's per-key callback run outside
// any f; the lane threads never take it).  One global lock held across a stream synchronise serialises destroys
// across contexts; destroys are not steady-state work, so that is accepted.
#pragma once
#include <cstdint>
#include <map>
#include <mutex>

namespace hec_live {
struct Registry {
    std::mutex mu;
    std::map<const void *, uint64_t> live;
    uint64_t gen = 0;
};
inline Registry &registry()
{
    static Registry r;
    return r;
}
// a new context: its generation, never 0 and never handed out twice
inline uint64_t ctx_register(const void *ctx)
{
    Registry &r = registry();
    std::lock_guard<std::mutex> lock(r.mu);
    return r.live[ctx] = ++r.gen;
}
// first step of a context's destroy, before anything of the context is freed
inline void ctx_unregister(const void *ctx)
{
    Registry &r = registry();
    std::lock_guard<std::mutex> lock(r.mu);
    r.live.erase(ctx);
}
// runs f with the registry locked when (ctx, gen) is live; false, and f not run, when that context is gone
template <class F>
bool while_alive(const void *ctx, uint64_t gen, F &&f)
{
    Registry &r = registry();
    std::lock_guard<std::mutex> lock(r.mu);
    const auto it = r.live.find(ctx);
    if (!ctx || it == r.live.end() || it->second != gen) return false;
    f();
    return true;
}
}  // namespace hec_live
