// C++ host with Coach::selfplay_class (include/az_host.hpp).  Usage: test_coach_class <dir> <channels> <seed> <class: -1 | 0 | 1 | absent>
// The configuration of tests/cpp/test_coach.cpp; "absent" never touches the knob.  Prints one JSON line with the per-iteration report;
// tests/test_net_class_gpu.py compares it and the files written under <dir> with the Python host's run of the same configuration.
#include <cstdio>
#include <cstdlib>

#include "az_host.hpp"

using namespace az_host;

int main(int argc, char** argv) {
    if (argc < 5) { std::fprintf(stderr, "usage: test_coach_class <dir> <channels> <seed> <class>\n"); return 2; }
    const std::string dir = argv[1];
    const int channels = std::atoi(argv[2]);
    const uint64_t seed = std::strtoull(argv[3], nullptr, 10);
    const std::string cls = argv[4];
    try {
        Engine e(0, 256, channels);
        e.check(az_net_init_random(e.raw(), 0, 3));
        e.check(az_set_option(e.raw(), "train_epochs", 2));
        Coach coach = Coach::setup(e, dir, 1000000, 0.55f, 15, 3, 100000, 1, 64, 16, 2, 48, 25, 1, 1000, 1);
        if (cls != "absent") coach.selfplay_class = (az_net_class)std::atoi(cls.c_str());
        const auto rep = coach.learn(false, seed);
        std::printf("[");
        for (size_t i = 0; i < rep.size(); ++i) {
            const auto& r = rep[i];
            std::printf("%s{\"iteration\": %zu, \"samples\": %zu, \"nwins\": %zu, \"pwins\": %zu, \"draws\": %zu, \"accepted\": %s, "
                        "\"model_id\": %zu, \"losses\": [", i ? ", " : "", r.iteration, r.samples, r.nwins, r.pwins, r.draws,
                        r.accepted ? "true" : "false", r.model_id);
            for (size_t k = 0; k < r.losses.size(); ++k) std::printf("%s%.9g", k ? ", " : "", r.losses[k]);
            std::printf("]}");
        }
        const auto live = e.net_class(coach.model_id);
        std::printf("]\n{\"live_class\": [%d, %d]}\n", (int)live.first, (int)live.second);
        return 0;
    } catch (const std::exception& ex) {
        std::fprintf(stderr, "panic: %s\n", ex.what());
        return 1;
    }
}
