// C++ host with Coach::validation_share / keep_best / patience (include/az_host.hpp).
// Usage: test_coach_validation <dir> <channels> <seed> <epochs> <validation_share> <keep_best> <patience>
// One iteration of the small configuration of tests/cpp/test_coach_options.cpp (32 episodes, 25 sims, 8 arena games); prints one JSON line
// with the per-iteration report, the validation keys included (doubles with 17 significant digits: they read back exactly).
// tests/test_evaluate_gpu.py compares it and the files written under <dir> with the Python host's run of the same configuration.
#include <cstdio>
#include <cstdlib>

#include "az_host.hpp"

using namespace az_host;

static void print_list(const char* key, const std::vector<double>& v) {
    std::printf(", \"%s\": [", key);
    for (size_t i = 0; i < v.size(); ++i) std::printf("%s%.17g", i ? ", " : "", v[i]);
    std::printf("]");
}

int main(int argc, char** argv) {
    if (argc != 8) { std::fprintf(stderr, "usage: test_coach_validation <dir> <channels> <seed> <epochs> <validation_share> <keep_best> <patience>\n"); return 2; }
    const std::string dir = argv[1];
    const int channels = std::atoi(argv[2]);
    const uint64_t seed = std::strtoull(argv[3], nullptr, 10);
    try {
        Engine e(0, 256, channels);
        e.check(az_net_init_random(e.raw(), 0, 3));
        e.check(az_set_option(e.raw(), "train_epochs", std::atoi(argv[4])));
        Coach coach = Coach::setup(e, dir, 1000000, 0.55f, 15, 3, 100000, 1, 64, 8, 1, 32, 25, 1, 1000, 1);
        coach.validation_share = std::atof(argv[5]);
        coach.keep_best = std::atoi(argv[6]) != 0;
        coach.patience = (size_t)std::atoi(argv[7]);
        const auto rep = coach.learn(false, seed);
        std::printf("[");
        for (size_t i = 0; i < rep.size(); ++i) {
            const auto& r = rep[i];
            std::printf("%s{\"iteration\": %zu, \"samples\": %zu, \"samples_raw\": %zu, \"nwins\": %zu, \"pwins\": %zu, \"draws\": %zu, \"accepted\": %s, \"model_id\": %zu",
                        i ? ", " : "", r.iteration, r.samples, r.samples_raw, r.nwins, r.pwins, r.draws, r.accepted ? "true" : "false", r.model_id);
            std::printf(", \"epochs\": %zu, \"val_n\": %zu, \"best_epoch\": %d", r.losses.size() / 2, r.val_n, (int)r.best_epoch);
            print_list("val_loss_pi", r.val_loss_pi);
            print_list("val_loss_v", r.val_loss_v);
            print_list("val_top1", r.val_top1);
            std::printf("}");
        }
        std::printf("]\n");
        return 0;
    } catch (const std::exception& ex) {
        std::fprintf(stderr, "panic: %s\n", ex.what());
        return 1;
    }
}
