// az_target.h -- per-tuple search statistics as training targets (az_selfplay_get_search, az_samples_blend_z, az_samples_surprise,
// include/az_engine.h).  The RULE is HIP-free apart from the host/device qualifier (AZT_HD, as az_draw.h has AZW_HD):
// the kernels of az_target.hip and az_tree.hip and the g++ twin of the tests (tests/cpp/target_twin.cpp, g++ -O2 -ffp-contract=off) compile
// this text.  Every formula is stated operation by operation -- f32 through az_noise.h's azn_* (the *_rn intrinsics on the device), f64
// through azt_d* below -- so every side gives the same bits.
//
//   root value   R of a move, from the root children's RAW counts n[a] and RAW q[a] (what az_tree_get_action_prob returns as counts and q;
//                they stay raw under forced playouts, pruning and Gumbel):
//                  acc = 0.0f, N = 0;  for a ascending with n[a] > 0:  acc = acc + (float)n[a] * q[a],  N += n[a]
//                  R = N ? acc / (float)N : 0.0f, clamped to [-1, 1]   (a child that wins at once carries q = 1.01; a z must stay in [-1, 1])
//                A child's q is in the perspective of the side to move at the root, the sign of the tuple's z.
//   blend        b = (float)lambda_e6 / 1e6f, a = 1.0f - b, z' = a * z + b * R;  lambda_e6 = 0 returns z and 1000000 returns R, bit for bit
//   surprise     KL_i = KL(pi_i || prior_i):  t = 0.0f;  for a ascending with pi[a] >= 2^-126:
//                  t = t + pi[a] * (log2(pi[a]) - log2(max(prior[a], 2^-126)))            (noise_log2 of az_noise.h)
//                KL = t * 0x3F317218 (ln 2), clamped to [0, 64];  K_i = llrint((double)KL * 2^32) as u64;  SK = sum of the K_i in u64 -- an
//                integer sum, so it does not depend on the order the additions arrive in; with n <= 2^24 it stays below 2^62
//   copies       s = (double)share_e6 / 1e6;  w_i = SK ? (1.0 - s) + s * (((double)n * (double)K_i) / (double)SK) : 1
//                U_i = (double)(rng_draw(seed, i, 0, RNG_SURPRISE) >> 11) * 2^-53;  c_i = floor(w_i) + (U_i < w_i - floor(w_i))
//                The weights average 1 over the window: a share 1 - s spread uniformly, a share s in proportion to KL.
#pragma once
#include <math.h>
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define AZT_HD __host__ __device__ __forceinline__
#else
#define AZT_HD inline
#endif

#include "az_noise.h"
#include "az_samples.h"

namespace az {

constexpr int TARGET_ACTIONS = 7;
constexpr int64_t TARGET_MAX_TUPLES = 1ll << 24;         // keeps SK below 2^62 (K_i <= 64 * 2^32)
constexpr int64_t TARGET_E6 = 1000000;
constexpr uint64_t TARGET_RNG_SURPRISE = 10;             // RNG_SURPRISE of az_common.h, restated (az_target.hip asserts that they agree)
constexpr float TARGET_MIN_NORMAL = 1.17549435e-38f;     // 2^-126
constexpr float TARGET_KL_MAX = 64.0f;

#if defined(__HIP_DEVICE_COMPILE__)
AZT_HD double azt_dadd(double a, double b) { return __dadd_rn(a, b); }
AZT_HD double azt_dsub(double a, double b) { return __dsub_rn(a, b); }
AZT_HD double azt_dmul(double a, double b) { return __dmul_rn(a, b); }
AZT_HD double azt_ddiv(double a, double b) { return __ddiv_rn(a, b); }
AZT_HD long long azt_llrint(double a) { return __double2ll_rn(a); }
#else
AZT_HD double azt_dadd(double a, double b) { return a + b; }
AZT_HD double azt_dsub(double a, double b) { return a - b; }
AZT_HD double azt_dmul(double a, double b) { return a * b; }
AZT_HD double azt_ddiv(double a, double b) { return a / b; }
AZT_HD long long azt_llrint(double a) { return llrint(a); }       // round to nearest even: the default rounding mode, which nothing here changes
#endif

AZT_HD uint64_t target_mix64(uint64_t x) {            // mix64 of az_common.h
    x += 0x9E3779B97F4A7C15ull;
    uint64_t z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
AZT_HD uint64_t target_rng(uint64_t seed, uint64_t i, uint64_t j, uint64_t purpose) {      // rng_draw of az_common.h
    return target_mix64(target_mix64(target_mix64(target_mix64(seed) ^ i) ^ j) ^ purpose);
}

AZT_HD float target_clamp1(float x) { return x > 1.0f ? 1.0f : (x < -1.0f ? -1.0f : x); }
// one term of the root value's sum: acc and N go on by child a's raw count and raw q
AZT_HD void target_root_term(float& acc, uint32_t& N, uint32_t n, float q) {
    if (n == 0u) return;
    acc = azn_add(acc, azn_mul((float)n, q));
    N += n;
}
AZT_HD float target_root_finish(float acc, uint32_t N) { return N ? target_clamp1(azn_div(acc, (float)N)) : 0.0f; }
// R from the counts and q of the root's children by action
AZT_HD float target_root_value(const uint32_t* n, const float* q) {
    float acc = 0.0f;
    uint32_t N = 0u;
    for (int a = 0; a < TARGET_ACTIONS; ++a) target_root_term(acc, N, n[a], q[a]);
    return target_root_finish(acc, N);
}

AZT_HD float target_blend(int64_t lambda_e6, float z, float R) {
    if (lambda_e6 == 0) return z;
    if (lambda_e6 == TARGET_E6) return R;
    const float b = azn_div((float)lambda_e6, 1e6f), a = azn_sub(1.0f, b);
    return azn_add(azn_mul(a, z), azn_mul(b, R));
}

AZT_HD float target_kl(const float* pi, const float* prior) {
    float t = 0.0f;
    for (int a = 0; a < TARGET_ACTIONS; ++a) {
        if (!(pi[a] >= TARGET_MIN_NORMAL)) continue;
        const float p = prior[a] > TARGET_MIN_NORMAL ? prior[a] : TARGET_MIN_NORMAL;
        t = azn_add(t, azn_mul(pi[a], azn_sub(noise_log2(pi[a]), noise_log2(p))));
    }
    const float kl = azn_mul(t, 0.693147182f);          // 0x3F317218
    return !(kl >= 0.0f) ? 0.0f : (kl > TARGET_KL_MAX ? TARGET_KL_MAX : kl);
}
AZT_HD uint64_t target_kl_fixed(float kl) { return (uint64_t)azt_llrint(azt_dmul((double)kl, 4294967296.0)); }

AZT_HD double target_weight(int64_t share_e6, int64_t n, uint64_t K, uint64_t SK) {
    if (SK == 0ull) return 1.0;
    const double s = azt_ddiv((double)share_e6, 1e6);
    return azt_dadd(azt_dsub(1.0, s), azt_dmul(s, azt_ddiv(azt_dmul((double)n, (double)K), (double)SK)));
}
AZT_HD uint32_t target_copies(double w, uint64_t seed, uint64_t i) {
    const double u = azt_dmul((double)(target_rng(seed, i, 0ull, TARGET_RNG_SURPRISE) >> 11), 1.1102230246251565e-16);      // 2^-53
    const double f = floor(w);
    return (uint32_t)(long long)f + (u < azt_dsub(w, f) ? 1u : 0u);
}

#if defined(__HIPCC__)
// ---- device side (az_target.hip) -----------------------------------------------------------------------------------------------------
// out[i] = target_blend(lambda_e6, zs[i], root_q[i]); *bad |= SAMPLE_BAD_VALUE where either input is NaN or outside [-1, 1]
void launch_target_blend(const float* zs, const float* root_q, int64_t n, int64_t lambda_e6, float* out, uint32_t* bad, hipStream_t s);
// pass 1: kl[i], K[i]; *SK += the K of every tuple (one 64-bit integer atomic per workgroup); *bad |= the verdict bits (sample_check of
// az_samples.h, and a prior outside [0, 1])
void launch_target_kl(const SampleWindow& w, const float* priors, int64_t n, float* kl, uint64_t* K, uint64_t* SK, uint32_t* bad, hipStream_t s);
// pass 2: counts[i] = c_i
void launch_target_copies(const uint64_t* K, const uint64_t* SK, int64_t n, int64_t share_e6, uint64_t seed, uint32_t* counts, hipStream_t s);
// pass 4 (behind launch_draw_scan of az_draw.h): output row r is tuple min{ i : Q[i] > r }; every copy bit for bit.  Any output may be nullptr
void launch_target_gather(const uint64_t* Q, int64_t n, int64_t total, uint32_t* idx /* [total] workspace */, const ulonglong2* states, const float* boards,
                          const float* pis, const float* zs, ulonglong2* o_states, float* o_boards, float* o_pis, float* o_zs, hipStream_t s);
#endif

}  // namespace az
