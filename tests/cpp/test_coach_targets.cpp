// C++ host with the search-statistics targets of Coach (include/az_host.hpp: value_target_q, surprise_share).  Usage:
// test_coach_targets <dir> <channels> <seed> [value_target_q=L] [surprise_share=S] [num_eps=N]
// One iteration of a small configuration (25 sims, 8 arena games, 1 epoch); prints one JSON line with the per-iteration report.
// tests/test_search_targets_gpu.py compares it and the files written under <dir> with the Python host's run of the same configuration.
#include <cstdio>
#include <cstdlib>
#include <map>

#include "az_host.hpp"

using namespace az_host;

int main(int argc, char** argv) {
    if (argc < 4) { std::fprintf(stderr, "usage: test_coach_targets <dir> <channels> <seed> [name=value ...]\n"); return 2; }
    const std::string dir = argv[1];
    const int channels = std::atoi(argv[2]);
    const uint64_t seed = std::strtoull(argv[3], nullptr, 10);
    std::map<std::string, const char*> opt = {{"value_target_q", "0"}, {"surprise_share", "0"}, {"num_eps", "32"}};
    for (int i = 4; i < argc; ++i) {
        const std::string arg = argv[i];
        const size_t eq = arg.find('=');
        const auto it = eq == std::string::npos ? opt.end() : opt.find(arg.substr(0, eq));
        if (it == opt.end()) { std::fprintf(stderr, "test_coach_targets: unknown option '%s'\n", argv[i]); return 2; }
        it->second = argv[i] + eq + 1;
    }
    try {
        Engine e(0, 256, channels);
        e.check(az_net_init_random(e.raw(), 0, 3));
        e.check(az_set_option(e.raw(), "train_epochs", 1));
        Coach coach = Coach::setup(e, dir, 1000000, 0.55f, 15, 3, 100000, 1, 64, 8, 1, std::strtoull(opt["num_eps"], nullptr, 10), 25, 1, 1000, 1);
        coach.value_target_q = std::atof(opt["value_target_q"]);
        coach.surprise_share = std::atof(opt["surprise_share"]);
        const auto rep = coach.learn(false, seed);
        std::printf("[");
        for (size_t i = 0; i < rep.size(); ++i) {
            const auto& r = rep[i];
            std::printf("%s{\"iteration\": %zu, \"samples\": %zu, \"nwins\": %zu, \"pwins\": %zu, \"draws\": %zu, \"accepted\": %s, \"model_id\": %zu}",
                        i ? ", " : "", r.iteration, r.samples, r.nwins, r.pwins, r.draws, r.accepted ? "true" : "false", r.model_id);
        }
        std::printf("]\n");
        return 0;
    } catch (const std::exception& ex) {
        std::fprintf(stderr, "panic: %s\n", ex.what());
        return 1;
    }
}
