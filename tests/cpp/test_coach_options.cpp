// C++ host with the opt-in fields of Coach (include/az_host.hpp).  Usage: test_coach_options <dir> <channels> <seed> [name=value ...]
// with the names root_noise_eps, root_noise_alpha, playout_cap_sims, playout_cap_full, forced_playouts_k, policy_prune, eval_mirror,
// arena_opening_plies (the Coach fields, at their defaults when absent) and num_eps (the episodes, default 32).  One iteration of a small
// configuration (25 sims, 8 arena games, 1 epoch); prints one JSON line with the per-iteration report.  The GPU tests of those options compare
// it and the files written under <dir> with the Python host's run of the same configuration.
#include <cstdio>
#include <cstdlib>
#include <map>

#include "az_host.hpp"

using namespace az_host;

int main(int argc, char** argv) {
    if (argc < 4) { std::fprintf(stderr, "usage: test_coach_options <dir> <channels> <seed> [name=value ...]\n"); return 2; }
    const std::string dir = argv[1];
    const int channels = std::atoi(argv[2]);
    const uint64_t seed = std::strtoull(argv[3], nullptr, 10);
    std::map<std::string, const char*> opt = {{"root_noise_eps", "0"}, {"root_noise_alpha", "1"}, {"playout_cap_sims", "0"}, {"playout_cap_full", "0.25"},
                                              {"forced_playouts_k", "0"}, {"policy_prune", "0"}, {"eval_mirror", "0"}, {"arena_opening_plies", "0"},
                                              {"num_eps", "32"}};
    for (int i = 4; i < argc; ++i) {
        const std::string arg = argv[i];
        const size_t eq = arg.find('=');
        const auto it = eq == std::string::npos ? opt.end() : opt.find(arg.substr(0, eq));
        if (it == opt.end()) { std::fprintf(stderr, "test_coach_options: unknown option '%s'\n", argv[i]); return 2; }
        it->second = argv[i] + eq + 1;
    }
    try {
        Engine e(0, 256, channels);
        e.check(az_net_init_random(e.raw(), 0, 3));
        e.check(az_set_option(e.raw(), "train_epochs", 1));
        Coach coach = Coach::setup(e, dir, 1000000, 0.55f, 15, 3, 100000, 1, 64, 8, 1, std::strtoull(opt["num_eps"], nullptr, 10), 25, 1, 1000, 1);
        coach.root_noise_eps = std::atof(opt["root_noise_eps"]);
        coach.root_noise_alpha = std::atof(opt["root_noise_alpha"]);
        coach.playout_cap_sims = std::atol(opt["playout_cap_sims"]);
        coach.playout_cap_full = std::atof(opt["playout_cap_full"]);
        coach.forced_playouts_k = std::atof(opt["forced_playouts_k"]);
        coach.policy_prune = std::atoi(opt["policy_prune"]) != 0;
        coach.eval_mirror = std::atoi(opt["eval_mirror"]) != 0;
        coach.arena_opening_plies = std::atoll(opt["arena_opening_plies"]);
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
