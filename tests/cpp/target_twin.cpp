// The g++ build of csrc/az_target.h behind a C interface (tests/target_twin.py): the root value, the z/q blend, the KL pass with its
// integer sum and the copies, tuple by tuple -- what the kernels of az_target.hip and k_selfplay_record must equal bit for bit.
// TEST INFRASTRUCTURE ONLY.  Build: g++ -std=c++17 -O2 -ffp-contract=off -shared -fPIC -I alphazero-rs_amd/csrc
#include <cstdint>

#include "az_target.h"

extern "C" {

// R [n] from counts [n][7] and q [n][7]
void twin_root_value(int64_t n, const uint32_t* counts, const float* q, float* out) {
    for (int64_t i = 0; i < n; ++i) out[i] = az::target_root_value(counts + i * 7, q + i * 7);
}

void twin_blend(int64_t n, const float* zs, const float* root_q, int64_t lambda_e6, float* out) {
    for (int64_t i = 0; i < n; ++i) out[i] = az::target_blend(lambda_e6, zs[i], root_q[i]);
}

// kl [n], K [n] (either may be null); returns SK
uint64_t twin_kl(int64_t n, const float* pis, const float* priors, float* kl, uint64_t* K) {
    uint64_t sk = 0;
    for (int64_t i = 0; i < n; ++i) {
        const float v = az::target_kl(pis + i * 7, priors + i * 7);
        const uint64_t k = az::target_kl_fixed(v);
        if (kl) kl[i] = v;
        if (K) K[i] = k;
        sk += k;
    }
    return sk;
}

// counts [n] and kl [n] of az_samples_surprise; w [n] (may be null) the weights in double; returns sum of the counts
uint64_t twin_surprise(int64_t n, const float* pis, const float* priors, int64_t share_e6, uint64_t seed, uint32_t* counts, float* kl, double* w) {
    const uint64_t sk = twin_kl(n, pis, priors, kl, nullptr);
    uint64_t total = 0;
    for (int64_t i = 0; i < n; ++i) {
        const uint64_t k = az::target_kl_fixed(az::target_kl(pis + i * 7, priors + i * 7));
        const double wi = az::target_weight(share_e6, n, k, sk);
        if (w) w[i] = wi;
        counts[i] = az::target_copies(wi, seed, (uint64_t)i);
        total += counts[i];
    }
    return total;
}

uint64_t twin_rng_surprise() { return az::TARGET_RNG_SURPRISE; }

}  // extern "C"
