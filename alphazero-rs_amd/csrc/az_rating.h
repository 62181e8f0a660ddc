// az_rating.h -- ratings from a round robin's result matrix (az_rating_fit, include/az_engine.h).
//
// Host-only, no HIP, no engine: g++ compiles this header alone (tests/cpp/rating_fit.cpp), and the Python twin tests/rating_twin.py repeats
// the same operations in the same order.
//
// Bradley-Terry with a draw counted as half a win, fitted by Hunter's MM iteration (Hunter 2004, "MM algorithms for generalized
// Bradley-Terry models").  wld [K][K][3]: wld[i][j] = {W, L, D} of model i against model j; the diagonal is ignored.  Every sum runs in
// ascending j, in double.
//   1. for i != j: s_ij = W + D/2 + prior/2, n_ij = W + L + D + prior; S_i = sum_j s_ij; gamma = 1
//   2. a sweep: gamma'_i = S_i / sum_{j != i} n_ij / (gamma_i + gamma_j) from the OLD gamma, then gamma' scaled so that sum gamma' = K
//   3. stop after the sweep whose max_i |gamma'_i - gamma_i| / gamma_i is below 1e-13, or after 100 000 sweeps
//   4. elo_i = 400 log10(gamma_i) minus the mean over the models
//   5. elo_se_i = (400 / ln 10) / sqrt(sum_j n_ij gamma_i gamma_j / (gamma_i + gamma_j)^2): the DIAGONAL of the Fisher information only, an
//      approximation that ignores the covariance between the models (and the constraint that fixes the mean)
// prior = 0 with a model that has no games, or only wins or only losses, diverges (its gamma runs to 0 or infinity until the sweep limit):
// prior = 2 (one virtual draw's worth of games against every other model) is the recommended value.
#pragma once
#include <cmath>
#include <cstdint>

namespace az {

constexpr int RATING_MAX_MODELS = 16;
constexpr int RATING_MAX_SWEEPS = 100000;
constexpr double RATING_TOL = 1e-13;

inline bool rating_args_ok(const uint64_t* wld, int K, double prior_games, const double* elo) {
    return wld && elo && K >= 2 && K <= RATING_MAX_MODELS && std::isfinite(prior_games) && prior_games >= 0.0;
}

// Returns false (nothing written) on a refused argument.  elo_se and sweeps may be nullptr.
inline bool rating_fit(const uint64_t* wld, int K, double prior_games, double* elo, double* elo_se, int32_t* sweeps) {
    if (!rating_args_ok(wld, K, prior_games, elo)) return false;
    double n[RATING_MAX_MODELS][RATING_MAX_MODELS], S[RATING_MAX_MODELS], g[RATING_MAX_MODELS], g2[RATING_MAX_MODELS];
    for (int i = 0; i < K; ++i) {
        S[i] = 0.0;
        for (int j = 0; j < K; ++j) {
            n[i][j] = 0.0;
            if (i == j) continue;
            const uint64_t* c = wld + ((size_t)i * K + j) * 3;
            const double W = (double)c[0], L = (double)c[1], D = (double)c[2];
            const double s = W + D / 2.0 + prior_games / 2.0;
            n[i][j] = W + L + D + prior_games;
            S[i] += s;
        }
        g[i] = 1.0;
    }
    int done = 0;
    for (int it = 0; it < RATING_MAX_SWEEPS; ++it) {
        double total = 0.0;
        for (int i = 0; i < K; ++i) {
            double den = 0.0;
            for (int j = 0; j < K; ++j)
                if (j != i) den += n[i][j] / (g[i] + g[j]);
            g2[i] = S[i] / den;
            total += g2[i];
        }
        const double scale = (double)K / total;
        double delta = 0.0;
        for (int i = 0; i < K; ++i) {
            g2[i] = g2[i] * scale;
            const double d = std::fabs(g2[i] - g[i]) / g[i];
            if (d > delta) delta = d;
        }
        for (int i = 0; i < K; ++i) g[i] = g2[i];
        done = it + 1;
        if (delta < RATING_TOL) break;
    }
    double mean = 0.0;
    for (int i = 0; i < K; ++i) { elo[i] = 400.0 * std::log10(g[i]); mean += elo[i]; }
    mean /= (double)K;
    for (int i = 0; i < K; ++i) elo[i] -= mean;
    if (elo_se) {
        const double unit = 400.0 / std::log(10.0);
        for (int i = 0; i < K; ++i) {
            double info = 0.0;
            for (int j = 0; j < K; ++j)
                if (j != i) info += n[i][j] * g[i] * g[j] / ((g[i] + g[j]) * (g[i] + g[j]));
            elo_se[i] = unit / std::sqrt(info);
        }
    }
    if (sweeps) *sweeps = done;
    return true;
}

}  // namespace az
