// az_forced.h -- forced playouts at the root and policy target pruning ("forced_playouts_k_e6" / "policy_prune", include/az_engine.h;
// KataGo, Wu 2019, section 3.2).  HIP-free apart from the host/device qualifier (AZF_HD, as az_playout.h has AZP_HD):
// the tree kernels and the g++ twin of the tests (tests/cpp/selfplay_twin.cpp) compile this text, and both give the same bits.  Integer
// operations and correctly rounded f32 * / + sqrt only: explicit *_rn intrinsics on the device, plain operators under g++ -O2
// -ffp-contract=off.  The square root is __builtin_sqrtf on both sides, NOT __fsqrt_rn (the comment above puct_sqrt_parent in az_common.h).
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#define AZF_HD __host__ __device__ __forceinline__
#else
#define AZF_HD inline
#endif

namespace az {

constexpr int64_t FORCED_K_E6_MAX = 16000000;

#if defined(__HIP_DEVICE_COMPILE__)
AZF_HD float azf_add(float a, float b) { return __fadd_rn(a, b); }
AZF_HD float azf_mul(float a, float b) { return __fmul_rn(a, b); }
AZF_HD float azf_div(float a, float b) { return __fdiv_rn(a, b); }
#else
AZF_HD float azf_add(float a, float b) { return a + b; }
AZF_HD float azf_mul(float a, float b) { return a * b; }
AZF_HD float azf_div(float a, float b) { return a / b; }
#endif

// k of the option value: the division in double, rounded once to f32 (as eps of "root_noise_eps_e6")
inline float forced_k_of(int64_t k_e6) { return (float)((double)k_e6 / 1e6); }

// nf = sqrt((k * p) * S): the visits a root child with prior p is owed when the root's children hold S visits together
AZF_HD float forced_nf(float k, float p, uint32_t S) { return __builtin_sqrtf(azf_mul(azf_mul(k, p), (float)S)); }
// FORCED SELECTION: a root child that has been visited (n > 0) and is still short of nf wins the root's arg-max (its u becomes +inf)
AZF_HD bool forced_child(float k, float p, uint32_t S, uint32_t n) { return n > 0u && (float)n < forced_nf(k, p, S); }

// sqrt(N_parent + 1e-6) and the PUCT term of az_common.h (src/node.rs:352-356), restated so that this header stands alone
AZF_HD float forced_sqrt_parent(uint32_t parent_n) { return __builtin_sqrtf(azf_add((float)parent_n, 1e-6f)); }
AZF_HD float forced_puct(float q, uint32_t n, float p, float sq, float cpuct_f) {
    return azf_add(q, azf_div(azf_mul(azf_mul(cpuct_f, p), sq), (float)((n + 1u) & 0xFFFFu)));
}
// PRUNED TARGET of one root child j != b (b = the most visited child, u_star = its PUCT value) with n > 0 visits, value q and prior p:
// take back at most f = (uint32_t)nf of its visits, one at a time, while the child -- with one visit fewer and its Q held fixed -- would
// still score below the best child; a child reduced to a single playout is pruned outright.
AZF_HD uint32_t forced_prune_loop(float k, float p, uint32_t S, uint32_t n, float q, float sq, float cpuct_f, float u_star) {
    const uint32_t f = (uint32_t)forced_nf(k, p, S);
    const uint32_t lo = n > f ? n - f : 0u;
    const float c = azf_mul(azf_mul(cpuct_f, p), sq);
    uint32_t m = n;
    while (m > lo && azf_add(q, azf_div(c, (float)m)) < u_star) --m;
    return m;
}
AZF_HD uint32_t forced_prune(float k, float p, uint32_t S, uint32_t n, float q, float sq, float cpuct_f, float u_star) {
    const uint32_t m = forced_prune_loop(k, p, S, n, q, sq, cpuct_f, u_star);
    return (m != n && m == 1u) ? 0u : m;          // the single-playout rule
}

}  // namespace az
