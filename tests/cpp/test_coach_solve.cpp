// C++ host with Coach::solve_min_stones / solve_max_nodes (include/az_host.hpp).  Usage: test_coach_solve <dir> <channels> <seed> <min_stones> <max_nodes>
// One iteration of the small configuration of test_coach_options.cpp (32 episodes, 25 sims, 8 arena games, 1 epoch); prints one JSON line with
// the per-iteration report, the move-quality tally included.  tests/test_solve_gpu.py compares it and the files written under <dir> with the
// Python host's run.
#include <cstdio>
#include <cstdlib>

#include "az_host.hpp"

using namespace az_host;

int main(int argc, char** argv) {
    if (argc < 6) { std::fprintf(stderr, "usage: test_coach_solve <dir> <channels> <seed> <min_stones> <max_nodes>\n"); return 2; }
    const std::string dir = argv[1];
    const int channels = std::atoi(argv[2]);
    const uint64_t seed = std::strtoull(argv[3], nullptr, 10);
    try {
        Engine e(0, 256, channels);
        e.check(az_net_init_random(e.raw(), 0, 3));
        e.check(az_set_option(e.raw(), "train_epochs", 1));
        Coach coach = Coach::setup(e, dir, 1000000, 0.55f, 15, 3, 100000, 1, 64, 8, 1, 32, 25, 1, 1000, 1);
        coach.solve_min_stones = (size_t)std::atoi(argv[4]);
        coach.solve_max_nodes = (uint32_t)std::strtoul(argv[5], nullptr, 10);
        const auto rep = coach.learn(false, seed);
        static const char* keys[6] = {"examined", "kept", "win_to_draw", "win_to_loss", "draw_to_loss", "unknown"};
        std::printf("[");
        for (size_t i = 0; i < rep.size(); ++i) {
            const auto& r = rep[i];
            std::printf("%s{\"iteration\": %zu, \"samples\": %zu, \"nwins\": %zu, \"pwins\": %zu, \"draws\": %zu, \"accepted\": %s, \"model_id\": %zu, \"quality\": {",
                        i ? ", " : "", r.iteration, r.samples, r.nwins, r.pwins, r.draws, r.accepted ? "true" : "false", r.model_id);
            for (int m = 0; m < 2; ++m) {
                std::printf("%s\"%s\": {", m ? ", " : "", m ? "old" : "new");
                for (int k = 0; k < 6; ++k) std::printf("%s\"%s\": %llu", k ? ", " : "", keys[k], (unsigned long long)r.quality[m][k]);
                std::printf("}");
            }
            std::printf("}}");
        }
        std::printf("]\n");
        return 0;
    } catch (const std::exception& ex) {
        std::fprintf(stderr, "panic: %s\n", ex.what());
        return 1;
    }
}
