// az_rating.h compiled alone by g++ (no HIP, no engine), built with -fsanitize=address,undefined by tests/test_tournament_cpu.py and run as a
// program.  argv = K prior c0 c1 ... (the K*K*3 counts of wld): fits them and prints one JSON line.
// With no arguments it runs a built-in sweep of shapes (every K, the refusals, a model that wins everything) and prints "ok".
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../../alphazero-rs_amd/csrc/az_rating.h"

static int self_check() {
    uint64_t rng = 0x9E3779B97F4A7C15ull;
    auto next = [&]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; };
    for (int K = 2; K <= az::RATING_MAX_MODELS; ++K) {
        std::vector<uint64_t> wld((size_t)K * K * 3, 0);
        for (int i = 0; i < K; ++i)
            for (int j = i + 1; j < K; ++j) {
                const uint64_t w = next() % 40, l = next() % 40, d = next() % 10;
                uint64_t* a = &wld[((size_t)i * K + j) * 3];
                uint64_t* b = &wld[((size_t)j * K + i) * 3];
                a[0] = w; a[1] = l; a[2] = d; b[0] = l; b[1] = w; b[2] = d;
            }
        std::vector<double> elo(K), se(K);
        int32_t sweeps = 0;
        if (!az::rating_fit(wld.data(), K, 2.0, elo.data(), se.data(), &sweeps)) return 1;
        double sum = 0;
        for (int i = 0; i < K; ++i) { sum += elo[i]; if (!(se[i] > 0)) return 2; }
        if (sum > 1e-9 || sum < -1e-9 || sweeps < 1) return 3;
        if (!az::rating_fit(wld.data(), K, 2.0, elo.data(), nullptr, nullptr)) return 4;     // the optional outputs
    }
    {   // every higher-listed model wins all 100 games, K = 4
        const int K = 4;
        std::vector<uint64_t> wld((size_t)K * K * 3, 0);
        for (int i = 0; i < K; ++i)
            for (int j = 0; j < K; ++j)
                if (i != j) wld[((size_t)i * K + j) * 3 + (i < j ? 0 : 1)] = 100;
        double elo[4], se[4];
        int32_t sweeps = 0;
        if (!az::rating_fit(wld.data(), K, 2.0, elo, se, &sweeps)) return 5;
        if (!(elo[0] > elo[1] && elo[1] > elo[2] && elo[2] > elo[3]) || sweeps >= az::RATING_MAX_SWEEPS) return 6;
    }
    {   // the refusals write nothing
        uint64_t wld[2 * 2 * 3] = {0, 0, 0, 3, 1, 0, 1, 3, 0, 0, 0, 0};
        double elo[2] = {7.0, 7.0}, se[2] = {7.0, 7.0};
        int32_t sweeps = 7;
        const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
        bool any = az::rating_fit(wld, 1, 2.0, elo, se, &sweeps) || az::rating_fit(wld, 17, 2.0, elo, se, &sweeps) ||
                   az::rating_fit(wld, 2, -1.0, elo, se, &sweeps) || az::rating_fit(wld, 2, inf, elo, se, &sweeps) ||
                   az::rating_fit(wld, 2, nan, elo, se, &sweeps) || az::rating_fit(nullptr, 2, 2.0, elo, se, &sweeps) ||
                   az::rating_fit(wld, 2, 2.0, nullptr, se, &sweeps);
        if (any || elo[0] != 7.0 || elo[1] != 7.0 || se[0] != 7.0 || se[1] != 7.0 || sweeps != 7) return 7;
    }
    std::printf("ok\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 3) return self_check();
    const int K = std::atoi(argv[1]);
    const double prior = std::atof(argv[2]);
    if (K < 1 || K > 64 || argc != 3 + K * K * 3) return 64;
    std::vector<uint64_t> wld((size_t)K * K * 3);
    for (size_t i = 0; i < wld.size(); ++i) wld[i] = std::strtoull(argv[3 + i], nullptr, 10);
    std::vector<double> elo((size_t)K, 0.0), se((size_t)K, 0.0);
    int32_t sweeps = 0;
    if (!az::rating_fit(wld.data(), K, prior, elo.data(), se.data(), &sweeps)) { std::printf("{\"refused\": true}\n"); return 0; }
    std::printf("{\"sweeps\": %d, \"elo\": [", sweeps);
    for (int i = 0; i < K; ++i) std::printf("%s%.17g", i ? ", " : "", elo[i]);
    std::printf("], \"elo_se\": [");
    for (int i = 0; i < K; ++i) std::printf("%s%.17g", i ? ", " : "", se[i]);
    std::printf("]}\n");
    return 0;
}
