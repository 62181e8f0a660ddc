// Config 5 in ONE process: the single-process version of connect_four_sharded.cpp.  `world` host threads, each with its own
// Engine, rank r on GPU r mod AZ_VISIBLE_GPUS, joined by one in-process communicator (az_comm_local_id: the collectives run inside
// the library, without RCCL) -- so a host that keeps the reference's one process (src/coach.rs:241-272 fans episodes out over a
// rayon pool) uses every GPU.  Each thread runs az_host::Coach::shard(r, world); rank 0 prints the same JSON line.
//
// Build:  g++ -std=c++17 -O2 -pthread -I include examples/connect_four_threads.cpp -o connect_four_threads -L alphazero-rs_amd -laz_engine
//         (and -Wl,-rpath,$PWD/alphazero-rs_amd)
// Run:    AZ_VISIBLE_GPUS=8 ./connect_four_threads 8 ./checkpoint [iters eps sims arena channels slots]
//
// Engines that share a device (world > AZ_VISIBLE_GPUS) are driven at once, so every engine runs with "search_graph" 0 and
// "train_graph" 0 (include/az_engine.h); one engine per device needs neither, but the options are kept equal on every rank.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <thread>
#include <vector>

#include "az_host.hpp"

int main(int argc, char** argv) {
    using namespace az_host;
    if (argc < 3) {
        std::fprintf(stderr, "usage: %s world checkpoint-dir [iters eps sims arena channels slots]\n", argv[0]);
        return 2;
    }
    const int world = std::atoi(argv[1]);
    const std::string dir = argv[2];
    const size_t iters = argc > 3 ? std::strtoul(argv[3], nullptr, 10) : 1;
    const size_t eps = argc > 4 ? std::strtoul(argv[4], nullptr, 10) : 64;
    const size_t sims = argc > 5 ? std::strtoul(argv[5], nullptr, 10) : 25;
    const size_t arena = argc > 6 ? std::strtoul(argv[6], nullptr, 10) : 40;
    const int channels = argc > 7 ? std::atoi(argv[7]) : 128;
    const size_t slots = argc > 8 ? std::strtoul(argv[8], nullptr, 10) : 8192;
    if (world < 1) { std::fprintf(stderr, "world %d < 1\n", world); return 2; }
    int ndev = 1;
    if (const char* v = std::getenv("AZ_VISIBLE_GPUS")) ndev = std::max(1, std::atoi(v));
    uint8_t id[AZ_COMM_ID_BYTES];
    try {
        Engine maker(0, 64, channels);
        maker.check(az_comm_local_id(maker.raw(), world, id));
    } catch (const std::exception& ex) {
        std::fprintf(stderr, "panic: %s\n", ex.what());
        return 1;
    }
    std::vector<int> rc((size_t)world, 0);
    std::vector<std::thread> threads;
    for (int rank = 0; rank < world; ++rank)
        threads.emplace_back([&, rank] {
            try {
                Engine e(rank % ndev, (int)slots, channels);
                e.check(az_set_option(e.raw(), "search_graph", 0));
                e.check(az_set_option(e.raw(), "train_graph", 0));
                if (az_net_load(e.raw(), 0, (dir + "/0.aznet").c_str()) != AZ_OK) e.check(az_net_init_random(e.raw(), 0, 0));
                Coach coach = Coach::setup(e, dir, 1000000, 0.6f, 15, 20, 200000, 1, slots, arena, iters, eps, sims, 1, 1000, 1);
                // after every rank's setup (az_comm_init returns once all have joined): no rank writes into dir before the others read it
                e.check(az_comm_init(e.raw(), rank, world, id));
                coach.shard(rank, world);
                coach.use_comm_at_world_1 = true;          // world 1 runs the same gather / all-reduce path through a one-rank communicator
                const auto t0 = std::chrono::steady_clock::now();
                const auto reports = coach.learn(false, /*seed*/ 0);
                const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
                e.check(az_comm_destroy(e.raw()));
                if (rank == 0) {
                    size_t samples = 0, nw = 0, pw = 0, dr = 0, acc = 0;
                    for (const auto& r : reports) { samples += r.samples; nw += r.nwins; pw += r.pwins; dr += r.draws; acc += r.accepted ? 1 : 0; }
                    std::printf("{\"example\": \"connect_four_threads\", \"world\": %d, \"iterations\": %zu, \"episodes_per_iteration\": %zu, \"sims\": %zu, "
                                "\"arena_games\": %zu, \"samples\": %zu, \"new_prev_draw\": [%zu, %zu, %zu], \"accepted\": %zu, \"seconds\": %.3f}\n",
                                world, reports.size(), eps, sims, arena, samples, nw, pw, dr, acc, secs);
                }
            } catch (const std::exception& ex) {        // the Engine is gone: its peers' collectives fail instead of waiting
                std::fprintf(stderr, "rank %d panic: %s\n", rank, ex.what());
                rc[(size_t)rank] = 1;
            }
        });
    for (auto& t : threads) t.join();
    for (int r : rc) if (r) return 1;
    return 0;
}
