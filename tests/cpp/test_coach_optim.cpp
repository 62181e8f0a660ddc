// C++ host with the optimiser rules of NNet::train on (Coach::weight_decay / clip_norm / lr_warmup_steps / lr_decay / lr_floor / ema_decay,
// include/az_host.hpp), modelled on test_coach_gumbel.cpp.  Usage: test_coach_optim <dir> <channels> <seed> [name=value ...] with those six
// names, num_sims (default 16) and num_eps (default 32).  One iteration of a small configuration (8 arena games, 1 epoch); prints one JSON
// line with the per-iteration report.  tests/test_coach_optim_gpu.py compares it and the files written under <dir> with the Python host's
// run of the same configuration.
#include <cstdio>
#include <cstdlib>
#include <map>

#include "az_host.hpp"

using namespace az_host;

int main(int argc, char** argv) {
    if (argc < 4) { std::fprintf(stderr, "usage: test_coach_optim <dir> <channels> <seed> [name=value ...]\n"); return 2; }
    const std::string dir = argv[1];
    const int channels = std::atoi(argv[2]);
    const uint64_t seed = std::strtoull(argv[3], nullptr, 10);
    std::map<std::string, const char*> opt = {{"weight_decay", "0"}, {"clip_norm", "0"}, {"lr_warmup_steps", "0"}, {"lr_decay", "0"}, {"lr_floor", "0"},
                                              {"ema_decay", "0"}, {"num_sims", "16"}, {"num_eps", "32"}};
    for (int i = 4; i < argc; ++i) {
        const std::string arg = argv[i];
        const size_t eq = arg.find('=');
        const auto it = eq == std::string::npos ? opt.end() : opt.find(arg.substr(0, eq));
        if (it == opt.end()) { std::fprintf(stderr, "test_coach_optim: unknown option '%s'\n", argv[i]); return 2; }
        it->second = argv[i] + eq + 1;
    }
    try {
        Engine e(0, 256, channels);
        e.check(az_net_init_random(e.raw(), 0, 3));
        e.check(az_set_option(e.raw(), "train_epochs", 1));
        Coach coach = Coach::setup(e, dir, 1000000, 0.55f, 15, 3, 100000, 1, 64, 8, 1, std::strtoull(opt["num_eps"], nullptr, 10),
                                   std::strtoull(opt["num_sims"], nullptr, 10), 1, 1000, 1);
        coach.weight_decay = std::atof(opt["weight_decay"]);
        coach.clip_norm = std::atof(opt["clip_norm"]);
        coach.lr_warmup_steps = std::atoll(opt["lr_warmup_steps"]);
        coach.lr_decay = std::atoll(opt["lr_decay"]);
        coach.lr_floor = std::atof(opt["lr_floor"]);
        coach.ema_decay = std::atof(opt["ema_decay"]);
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
