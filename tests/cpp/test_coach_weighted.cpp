// C++ host with Coach::merge_weighted (include/az_host.hpp).  Usage: test_coach_weighted <dir> <channels> <seed> <iterations> <canonical>
// A tiny configuration (16 episodes, 25 sims, 8 arena games, 1 epoch) with merge_positions and merge_weighted on; prints one JSON line with
// the per-iteration report.  tests/test_train_samples_gpu.py compares it and the files written under <dir> with the Python host's run.
#include <cstdio>
#include <cstdlib>

#include "az_host.hpp"

using namespace az_host;

int main(int argc, char** argv) {
    if (argc < 6) { std::fprintf(stderr, "usage: test_coach_weighted <dir> <channels> <seed> <iterations> <canonical>\n"); return 2; }
    const std::string dir = argv[1];
    const int channels = std::atoi(argv[2]);
    const uint64_t seed = std::strtoull(argv[3], nullptr, 10);
    try {
        Engine e(0, 256, channels);
        e.check(az_net_init_random(e.raw(), 0, 3));
        e.check(az_set_option(e.raw(), "train_epochs", 1));
        Coach coach = Coach::setup(e, dir, 1000000, 0.55f, 15, 3, 100000, 1, 64, 8, (size_t)std::atoi(argv[4]), 16, 25, 1, 1000, 1);
        coach.merge_positions = true;
        coach.merge_canonical = std::atoi(argv[5]) != 0;
        coach.merge_weighted = true;
        const auto rep = coach.learn(false, seed);
        std::printf("[");
        for (size_t i = 0; i < rep.size(); ++i) {
            const auto& r = rep[i];
            std::printf("%s{\"iteration\": %zu, \"samples\": %zu, \"samples_raw\": %zu, \"samples_weight\": %zu, \"nwins\": %zu, \"pwins\": %zu, "
                        "\"draws\": %zu, \"accepted\": %s, \"model_id\": %zu}",
                        i ? ", " : "", r.iteration, r.samples, r.samples_raw, r.samples_weight, r.nwins, r.pwins, r.draws,
                        r.accepted ? "true" : "false", r.model_id);
        }
        std::printf("]\n");
        return 0;
    } catch (const std::exception& ex) {
        std::fprintf(stderr, "panic: %s\n", ex.what());
        return 1;
    }
}
