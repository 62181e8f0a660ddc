// C++ host with Coach::reanalyse_sims (include/az_host.hpp).  Usage: test_coach_reanalyse <dir> <channels> <seed> <num_iters> <reanalyse_sims>
// [value_target_q].  num_iters iterations of a small configuration (16 episodes, 25 sims, 8 arena games, 1 epoch, a history of 3 windows),
// resuming from whatever <dir> holds; prints one JSON line with the per-iteration report.  tests/test_reanalyse_gpu.py compares it and the
// files written under <dir> with the Python host's run of the same configuration.
#include <cstdio>
#include <cstdlib>

#include "az_host.hpp"

using namespace az_host;

int main(int argc, char** argv) {
    if (argc < 6) { std::fprintf(stderr, "usage: test_coach_reanalyse <dir> <channels> <seed> <num_iters> <reanalyse_sims> [value_target_q]\n"); return 2; }
    const std::string dir = argv[1];
    const int channels = std::atoi(argv[2]);
    const uint64_t seed = std::strtoull(argv[3], nullptr, 10);
    const size_t num_iters = std::strtoull(argv[4], nullptr, 10);
    try {
        Engine e(0, 256, channels);
        e.check(az_net_init_random(e.raw(), 0, 3));
        e.check(az_set_option(e.raw(), "train_epochs", 1));
        Coach coach = Coach::setup(e, dir, 1000000, 0.55f, 15, 3, 100000, 1, 64, 8, num_iters, 16, 25, 1, 1000, 1);
        coach.reanalyse_sims = std::strtoull(argv[5], nullptr, 10);
        if (argc > 6) coach.value_target_q = std::atof(argv[6]);
        const auto rep = coach.learn(false, seed);
        std::printf("[");
        for (size_t i = 0; i < rep.size(); ++i) {
            const auto& r = rep[i];
            std::printf("%s{\"iteration\": %zu, \"samples\": %zu, \"nwins\": %zu, \"pwins\": %zu, \"draws\": %zu, \"accepted\": %s, \"model_id\": %zu, "
                        "\"reanalysed\": %zu}",
                        i ? ", " : "", r.iteration, r.samples, r.nwins, r.pwins, r.draws, r.accepted ? "true" : "false", r.model_id, r.reanalysed);
        }
        std::printf("]\n");
        return 0;
    } catch (const std::exception& ex) {
        std::fprintf(stderr, "panic: %s\n", ex.what());
        return 1;
    }
}
