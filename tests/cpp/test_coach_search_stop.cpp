// C++ host with Coach::search_stop (include/az_host.hpp; include/az_search_stop.h).  Usage: test_coach_search_stop <dir> <channels> <seed>
// <search_stop 0|1|-1> <num_eps> <num_sims>; -1 never touches the field.  One iteration of a small configuration (8 arena games, 1 epoch);
// prints one JSON line with the per-iteration report and one with the four counters.  tests/test_search_stop_gpu.py compares it and the
// files written under <dir> with the Python host's run of the same configuration.
#include <cstdio>
#include <cstdlib>

#include "az_host.hpp"

using namespace az_host;

int main(int argc, char** argv) {
    if (argc < 7) { std::fprintf(stderr, "usage: test_coach_search_stop <dir> <channels> <seed> <search_stop> <num_eps> <num_sims>\n"); return 2; }
    const std::string dir = argv[1];
    const int channels = std::atoi(argv[2]), stop = std::atoi(argv[4]);
    const uint64_t seed = std::strtoull(argv[3], nullptr, 10);
    try {
        Engine e(0, 256, channels);
        e.check(az_net_init_random(e.raw(), 0, 3));
        e.check(az_set_option(e.raw(), "train_epochs", 1));
        Coach coach = Coach::setup(e, dir, 1000000, 0.55f, 15, 3, 100000, 1, 64, 8, 1, std::strtoull(argv[5], nullptr, 10),
                                   std::strtoull(argv[6], nullptr, 10), 1, 1000, 1);
        if (stop >= 0) coach.search_stop = stop != 0;
        const auto rep = coach.learn(false, seed);
        std::printf("[");
        for (size_t i = 0; i < rep.size(); ++i) {
            const auto& r = rep[i];
            std::printf("%s{\"iteration\": %zu, \"samples\": %zu, \"nwins\": %zu, \"pwins\": %zu, \"draws\": %zu, \"accepted\": %s, \"model_id\": %zu}",
                        i ? ", " : "", r.iteration, r.samples, r.nwins, r.pwins, r.draws, r.accepted ? "true" : "false", r.model_id);
        }
        std::printf("]\n");
        const SearchStopStats s = search_stop_stats(e);
        std::printf("{\"eligible_moves\": %llu, \"stopped_moves\": %llu, \"budgeted_sims\": %llu, \"skipped_sims\": %llu}\n", (unsigned long long)s.eligible_moves,
                    (unsigned long long)s.stopped_moves, (unsigned long long)s.budgeted_sims, (unsigned long long)s.skipped_sims);
        return 0;
    } catch (const std::exception& ex) {
        std::fprintf(stderr, "panic: %s\n", ex.what());
        return 1;
    }
}
