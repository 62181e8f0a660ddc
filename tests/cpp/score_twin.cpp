// The g++ build of csrc/az_score.h behind a C interface (tests/score_twin.py): the per-tuple score with its integer sums, the hold-out rule
// and the best / stop decision -- what the kernels of az_score.hip and the engine's per-epoch validation must equal bit for bit.
// TEST INFRASTRUCTURE ONLY.  Build: g++ -std=c++17 -O2 -ffp-contract=off -shared -fPIC -I alphazero-rs_amd/csrc
#include <cstdint>

#include "az_score.h"

extern "C" {

// p [n][7] and v [n] the net's output, pis [n][7] and zs [n] the targets, states [n][2], weights [n] or null; sums [5] = S_ce, S_kl, S_se,
// S_hit, W; ce, se, kl [n] and hit [n] (each may be null)
void twin_score(int64_t n, const float* p, const float* v, const float* pis, const float* zs, const uint64_t* states, const uint32_t* weights,
                uint64_t* sums, float* ce, float* se, float* kl, uint8_t* hit) {
    for (int j = 0; j < az::SCORE_SUMS; ++j) sums[j] = 0;
    for (int64_t i = 0; i < n; ++i) {
        const float c = az::score_ce(pis + i * 7, p + i * 7), k = az::target_kl(pis + i * 7, p + i * 7), s = az::score_se(v[i], zs[i]);
        const uint32_t h = az::score_hit(pis + i * 7, p + i * 7, states[2 * i], states[2 * i + 1]);
        const uint64_t w = weights ? weights[i] : 1;
        sums[0] += w * az::score_fixed(c);
        sums[1] += w * az::score_fixed(k);
        sums[2] += w * az::score_fixed(s);
        sums[3] += w * h;
        sums[4] += w;
        if (ce) ce[i] = c;
        if (se) se[i] = s;
        if (kl) kl[i] = k;
        if (hit) hit[i] = (uint8_t)h;
    }
}

void twin_holdout(int64_t n, const uint64_t* states, int64_t share_e6, uint64_t seed, uint8_t* held, uint64_t* keys) {
    const uint64_t t = az::score_thresh24((uint64_t)share_e6);
    for (int64_t i = 0; i < n; ++i) {
        const uint64_t k = az::score_holdout_key(states[2 * i], states[2 * i + 1]);
        if (keys) keys[i] = k;
        held[i] = az::score_held(seed, k, t) ? 1 : 0;
    }
}

// hist [n][4] = (loss_pi, loss_v, kl, top1) per epoch; returns stop, *best = the best epoch
int32_t twin_best_stop(const double* hist, int32_t n, int32_t patience, int32_t* best) {
    int b = 0;
    const bool stop = az::score_best_stop(hist, 4, n, patience, &b);
    *best = b;
    return stop ? 1 : 0;
}

}  // extern "C"
