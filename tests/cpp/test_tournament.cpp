// The hash-net case of tests/test_tournament_gpu.py through include/az_host.hpp: az_host::tournament and az_host::rating_fit, one JSON line.
// argv: games_per_pair num_sims opening_plies seed salt0 salt1 salt2 ...   (model ids 60, 61, ...)
#include <cstdio>
#include <cstdlib>

#include "az_host.hpp"

int main(int argc, char** argv) {
    if (argc < 7) return 64;
    try {
        az_host::Engine e(0, 256, 128);
        az_host::TournamentParams p;
        p.games_per_pair = std::atoi(argv[1]);
        p.num_sims = std::atoi(argv[2]);
        e.set_arena_openings(std::atoll(argv[3]));
        p.seed = std::strtoull(argv[4], nullptr, 10);
        for (int i = 5; i < argc; ++i) {
            const int32_t id = 60 + (i - 5);
            e.check(az_net_set_kind(e.raw(), id, AZ_NET_HASH, std::strtoull(argv[i], nullptr, 10)));
            p.model_ids.push_back(id);
        }
        const az_host::TournamentResult r = az_host::tournament(e, p);
        const az_host::Ratings fit = az_host::rating_fit(r.wld, r.K);
        std::printf("{\"wld\": [");
        for (size_t i = 0; i < r.wld.size(); ++i) std::printf("%s%llu", i ? ", " : "", (unsigned long long)r.wld[i]);
        std::printf("], \"results\": [");
        for (size_t i = 0; i < r.results.size(); ++i) std::printf("%s%d", i ? ", " : "", (int)r.results[i]);
        std::printf("], \"game_len\": [");
        for (size_t i = 0; i < r.game_len.size(); ++i) std::printf("%s%d", i ? ", " : "", (int)r.game_len[i]);
        std::printf("], \"moves\": [");
        for (size_t i = 0; i < r.moves.size(); ++i) std::printf("%s%d", i ? ", " : "", (int)r.moves[i]);
        std::printf("], \"sweeps\": %d, \"elo\": [", fit.sweeps);
        for (size_t i = 0; i < fit.elo.size(); ++i) std::printf("%s%.17g", i ? ", " : "", fit.elo[i]);
        std::printf("], \"elo_se\": [");
        for (size_t i = 0; i < fit.elo_se.size(); ++i) std::printf("%s%.17g", i ? ", " : "", fit.elo_se[i]);
        std::printf("]}\n");
    } catch (const az_host::Panic& ex) {
        std::fprintf(stderr, "panic: %s\n", ex.what());
        return 1;
    }
    return 0;
}
