// Stand-alone host check of the live-context registry (no GPU, no Python): destroys racing with a context's
// own destroy.  Reader threads do what an object's destroy does, while_alive(ctx, gen, read a field of the context);
// the main thread does what hec_context_destroy does, unregister, then overwrite and delete.  A callable that ran on
// a context that was gone reads a wiped field or freed memory.  Meant for two sanitizer builds, both of which must end
// clean:
//   g++ -std=c++17 -g -O1 -pthread -fsanitize=thread \
//       -Ihomomorphic-encryption-algorithms-diploma-thesis_amd/csrc tools/live_host_check.cpp \
//       -o live_host_check_tsan && ./live_host_check_tsan
//   g++ -std=c++17 -g -O1 -pthread -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Ihomomorphic-encryption-algorithms-diploma-thesis_amd/csrc tools/live_host_check.cpp \
//       -o live_host_check_asan && ./live_host_check_asan
#include "hec_live.h"

#include <atomic>
#include <cstdio>
#include <thread>
#include <vector>

struct FakeContext {
    uint64_t stream = 0;  // stands for c.stream: what a destroy reads through the object's context pointer
};

int main()
{
    const int rounds = 2000, readers = 4;
    const uint64_t alive_mark = 0x5EA1C0DE, wiped = 0xDEADDEAD;
    std::atomic<long> ran{0}, refused{0}, bad{0};
    // what the readers' "objects" record of the current context; published before the round's start flag
    const void *ctx_of_round = nullptr;
    uint64_t gen_of_round = 0;
    std::atomic<int> round{0}, done{0};

    std::vector<std::thread> th;
    for (int t = 0; t < readers; ++t)
        th.emplace_back([&, t] {
            for (int r = 1; r <= rounds; ++r) {
                while (round.load(std::memory_order_acquire) < r) std::this_thread::yield();
                const void *ctx = ctx_of_round;
                const uint64_t gen = gen_of_round;
                // half of the readers hurry, the others give the destroy a head start: both outcomes occur
                for (int k = 0; k < 8; ++k) {
                    if ((t + r) & 1) std::this_thread::yield();
                    bool in_f = false;
                    const bool ok = hec_live::while_alive(ctx, gen, [&] {
                        in_f = true;
                        if (static_cast<const FakeContext *>(ctx)->stream != alive_mark) ++bad;
                    });
                    if (ok != in_f) ++bad;  // a refused call ran its callable, or the reverse
                    ++(ok ? ran : refused);
                }
                done.fetch_add(1, std::memory_order_release);
            }
        });

    for (int r = 1; r <= rounds; ++r) {
        auto *ctx = new FakeContext();
        ctx->stream = alive_mark;
        ctx_of_round = ctx;
        gen_of_round = hec_live::ctx_register(ctx);
        const long ran0 = ran.load();
        round.store(r, std::memory_order_release);
        // odd rounds: the destroy arrives while the readers are at work on the context; even rounds: before them
        if (r & 1)
            while (ran.load() == ran0) std::this_thread::yield();
        hec_live::ctx_unregister(ctx);  // waits for a running callable; none starts on this context afterwards
        ctx->stream = wiped;
        delete ctx;
        // a stale generation at a possibly reused address is refused as well
        if (hec_live::while_alive(ctx, gen_of_round, [&] { ++bad; })) ++bad;
        while (done.load(std::memory_order_acquire) < r * readers) std::this_thread::yield();
    }
    for (auto &t : th) t.join();

    std::printf("live_host_check: %ld ran, %ld refused, %ld bad\n", ran.load(), refused.load(), bad.load());
    if (bad.load() || !ran.load() || !refused.load()) {
        std::fprintf(stderr, "live_host_check: FAILED\n");
        return 1;
    }
    std::printf("live_host_check: ok\n");
    return 0;
}
