// BASELINE config 1 (25 sims/move, 1 sim thread) as the fine-grained drop-in with MANY host threads: N std::threads, each looping
// Coach::execute_episode (src/coach.rs:104-157) over an AsyncMcts on its own slot of one az_host::SharedMcts -- the shape of the
// reference's rayon pool of episode threads (src/coach.rs:202-205, :241-272) sharing one inference_thread
// (src/async_mcts.rs:117-189).  The engine coalesces the threads' get_action_prob calls into batched searches (az_tree_share).
// Prints one JSON line: moves/s for N in {1, 16, 64, 256} with the reference's stub net and with the bf16 C = 512 conv net.
// Build:  g++ -std=c++17 -O2 -pthread -I include examples/concurrent_dropin.cpp -o concurrent_dropin -L alphazero-rs_amd -laz_engine -Wl,-rpath,$PWD/alphazero-rs_amd
// Run:    ./concurrent_dropin [episodes per thread] [sims] [window_us]
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <thread>
#include <vector>

#include "az_host.hpp"

using namespace az_host;

// one warm-up round (graph capture, first-touch allocations), then the timed one; returns moves/s
static double run(Engine& e, int model_id, int threads, int per_thread, int sims, int window_us, std::array<uint64_t, 4>* st) {
    SharedMcts sh(e, (size_t)threads, 1000000, (size_t)sims, 1, 1000, (size_t)model_id, 1, window_us);
    double rate = 0;
    for (int pass = 0; pass < 2; ++pass) {
        const int episodes = pass ? threads * per_thread : threads;
        std::atomic<int> next{0};
        std::atomic<size_t> moves{0};
        std::atomic<bool> failed{false};
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<std::thread> pool;
        for (int w = 0; w < threads; ++w)
            pool.emplace_back([&] {
                try {
                    for (int ep; (ep = next.fetch_add(1)) < episodes;) {
                        AsyncMcts m = sh.mcts();
                        std::vector<uint8_t> mv;
                        execute_episode(m, 15, (size_t)ep, /*seed*/ 0, &mv);
                        moves += mv.size();
                    }
                } catch (const std::exception& ex) {
                    std::fprintf(stderr, "panic: %s\n", ex.what());
                    failed = true;
                }
            });
        for (auto& t : pool) t.join();
        if (failed) throw Panic("a worker failed");
        const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        rate = (double)moves / dt;
    }
    *st = sh.stats();
    return rate;
}

int main(int argc, char** argv) {
    const int per_thread = argc > 1 ? std::atoi(argv[1]) : 3;
    const int sims = argc > 2 ? std::atoi(argv[2]) : 25;
    const int window_us = argc > 3 ? std::atoi(argv[3]) : 0;
    try {
        Engine e(0, 256, 512);
        e.check(az_net_set_kind(e.raw(), 0, AZ_NET_STUB, 0));
        e.check(az_net_init_random(e.raw(), 1, 1));
        std::printf("{\"sims_per_move\": %d, \"episodes_per_thread\": %d, \"window_us\": %d", sims, per_thread, window_us);
        for (const auto& net : {std::make_pair("stub_net", 0), std::make_pair("conv_net", 1)}) {
            std::printf(", \"%s\": {", net.first);
            for (int n : {1, 16, 64, 256}) {
                std::array<uint64_t, 4> st{};
                const double r = run(e, net.second, n, per_thread, sims, window_us, &st);
                std::printf("%s\"%d\": {\"moves_per_sec\": %.1f, \"requests_per_batch\": %.2f}", n == 1 ? "" : ", ", n, r,
                            st[0] ? (double)st[1] / (double)st[0] : 0.0);
                std::fflush(stdout);
            }
            std::printf("}");
        }
        std::printf("}\n");
        return 0;
    } catch (const std::exception& ex) {
        std::fprintf(stderr, "panic: %s\n", ex.what());
        return 1;
    }
}
