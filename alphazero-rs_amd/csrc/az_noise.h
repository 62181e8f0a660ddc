// az_noise.h -- the sampler of the opt-in Dirichlet root noise (include/az_engine.h "root_noise_eps_e6").
// Plain C++ with no HIP in it: hipcc compiles it for the device (az_tree.hip), g++ -O2 -ffp-contract=off for the host (the twin of
// tests/cpp/selfplay_twin.cpp), and both produce the same bits.  It uses integer operations and correctly rounded f32
// + - * / sqrt only -- explicit *_rn intrinsics on the device, where the compiler would otherwise contract a * b + c and where a bare
// v_sqrt_f32 is 1 ulp off (az_common.h) -- and carries its own log2 / exp2: no call into libm or the device math library.
//
// THE SCHEME (everything a second implementation needs to reproduce eta bit for bit; all arithmetic is IEEE f32, round to nearest even,
// in exactly the operation order written below):
//   stream    draw j of action a of the root (seed, game_id, ply) = rng_draw(seed, game_id, ply, 5 + 256 * a + 65536 * j)
//             (rng_draw / mix64: az_common.h; purpose RNG_NOISE = 5).  An action's variate has a sub-stream of its own, so one action's
//             rejection count never shifts another's draws.
//   uniform   U(r) = ((float)(r >> 40) + 0.5f) * 2^-24.  The sum is rounded (to even) for r >> 40 >= 2^23, so U lies in (0, 1].
//   gamma     g ~ Gamma(alpha) by Marsaglia-Tsang with polar normals:  A = alpha < 1 ? alpha + 1 : alpha;  d = A - 1/3 (0x3EAAAAAB);
//             c = 1 / sqrt(9 * d).  Round r = 0 .. 31 uses draws j = 3r, 3r + 1, 3r + 2:
//               v1 = 2 * U(3r) - 1;  v2 = 2 * U(3r + 1) - 1;  s = v1 * v1 + v2 * v2;      rejected unless 0 < s < 1
//               x = v1 * sqrt((-2 * ln(s)) / s);  v = 1 + c * x;                            rejected unless v > 0
//               v = (v * v) * v;                                                            rejected if v < 2^-126
//               accepted iff ln(U(3r + 2)) < (0.5 * (x * x) + (d - d * v)) + d * ln(v);  then g = d * v
//             After 32 rejected rounds g = A (never seen: a round is rejected with probability < 0.27).
//             alpha < 1:  g = g * exp2(log2(U(96)) / alpha)            (the u^(1/alpha) boost; draw j = 96)
//   eta       eta[a] = g[a] / sum, sum = the g of the valid actions added in ascending action order starting from 0.0f;
//             sum == 0 (every variate underflowed): eta[a] = 1 / (float)k over the k valid actions.  Invalid actions: 0.
//   mixing    prior <- (1 - eps) * prior + eps * eta[a]                (three roundings: 1 - eps, the two products, the sum)
//   ln(x) = log2(x) * 0x3F317218 (ln 2);  log2 and exp2 are the polynomials below.
// Measured against math.log2 / 2**x in float64 (tests/test_root_noise_cpu.py): the relative error of noise_log2 over [2^-126, 2^24] is at
// most 2.7e-7, that of noise_exp2 over (-125, 0] at most 1.0e-7; the sampler needs 1e-5.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define AZN_HD __host__ __device__ __forceinline__
#else
#define AZN_HD inline
#endif

namespace az {

constexpr uint64_t NOISE_PURPOSE = 5;        // == RNG_NOISE (az_common.h)
constexpr int NOISE_ROUNDS = 32;             // rejection rounds per variate: every loop of the sampler is bounded
constexpr uint64_t NOISE_BOOST_DRAW = 96;    // draw index of the alpha < 1 boost (3 * NOISE_ROUNDS)

#if defined(__HIP_DEVICE_COMPILE__)
AZN_HD float azn_add(float a, float b) { return __fadd_rn(a, b); }
AZN_HD float azn_sub(float a, float b) { return __fsub_rn(a, b); }
AZN_HD float azn_mul(float a, float b) { return __fmul_rn(a, b); }
AZN_HD float azn_div(float a, float b) { return __fdiv_rn(a, b); }
#else
AZN_HD float azn_add(float a, float b) { return a + b; }
AZN_HD float azn_sub(float a, float b) { return a - b; }
AZN_HD float azn_mul(float a, float b) { return a * b; }
AZN_HD float azn_div(float a, float b) { return a / b; }
#endif
AZN_HD float azn_sqrt(float a) { return __builtin_sqrtf(a); }       // correctly rounded on both sides (never of a negative number here)
AZN_HD uint32_t azn_bits(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }
AZN_HD float azn_float(uint32_t u) { float f; __builtin_memcpy(&f, &u, 4); return f; }

// same function as mix64 of az_common.h (restated: this header includes nothing of the engine)
AZN_HD uint64_t noise_mix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    uint64_t z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// the part of rng_draw(seed, game_id, ply, .) the draws of one root share
AZN_HD uint64_t noise_stream(uint64_t seed, uint64_t game_id, uint64_t ply) { return noise_mix64(noise_mix64(noise_mix64(seed) ^ game_id) ^ ply); }
AZN_HD uint64_t noise_draw(uint64_t stream, uint32_t a, uint64_t j) { return noise_mix64(stream ^ (NOISE_PURPOSE + 256ull * a + 65536ull * j)); }
AZN_HD float noise_uniform(uint64_t r) { return azn_mul(azn_add((float)(uint32_t)(r >> 40), 0.5f), 5.9604644775390625e-8f); }

// log2 of a normal positive x: x = m * 2^e with m in [sqrt(1/2), sqrt(2)); ln(m) = 2 * atanh(s), s = (m - 1) / (m + 1), by its odd series
// up to s^9 (|s| < 0.1716: the first dropped term is below 2e-9 of the result) -- relative accuracy holds through x = 1
AZN_HD float noise_log2(float x) {
    const uint32_t u = azn_bits(x);
    int e = (int)(u >> 23) - 127;
    uint32_t mb = (u & 0x007FFFFFu) | 0x3F800000u;
    if (mb >= 0x3FB504F3u) { mb -= 0x00800000u; e += 1; }
    const float m = azn_float(mb);
    const float s = azn_div(azn_sub(m, 1.0f), azn_add(m, 1.0f));
    const float z = azn_mul(s, s);
    float p = 0.111111111f;
    p = azn_add(azn_mul(p, z), 0.142857143f);
    p = azn_add(azn_mul(p, z), 0.2f);
    p = azn_add(azn_mul(p, z), 0.333333333f);
    p = azn_add(azn_mul(p, z), 1.0f);
    const float ln_m = azn_mul(azn_mul(2.0f, s), p);
    return azn_add((float)e, azn_mul(ln_m, 1.44269504f));
}
AZN_HD float noise_ln(float x) { return azn_mul(noise_log2(x), 0.693147182f); }

// 2^x for x <= 0 (larger x is taken as 0); 0 below -125 (no subnormal results).  x = n + r, |r| <= 1/2; 2^r = e^(r ln 2) by its series
// up to t^7 (|t| < 0.3466: the first dropped term is below 6e-9); the exponent is added to the bits
AZN_HD float noise_exp2(float x) {
    if (!(x > -125.0f)) return 0.0f;
    if (x > 0.0f) x = 0.0f;
    const int n = (int)azn_sub(x, 0.5f);
    const float t = azn_mul(azn_sub(x, (float)n), 0.693147182f);
    float p = 1.98412698e-4f;
    p = azn_add(azn_mul(p, t), 1.38888889e-3f);
    p = azn_add(azn_mul(p, t), 8.33333333e-3f);
    p = azn_add(azn_mul(p, t), 4.16666667e-2f);
    p = azn_add(azn_mul(p, t), 0.166666667f);
    p = azn_add(azn_mul(p, t), 0.5f);
    p = azn_add(azn_mul(p, t), 1.0f);
    p = azn_add(azn_mul(p, t), 1.0f);
    return azn_float(azn_bits(p) + ((uint32_t)n << 23));
}

// the Gamma(alpha) variate of action a of the root whose stream is `stream` (noise_stream)
AZN_HD float noise_gamma(uint64_t stream, uint32_t a, float alpha) {
    const bool boost = alpha < 1.0f;
    const float A = boost ? azn_add(alpha, 1.0f) : alpha;
    const float d = azn_sub(A, 0.333333343f);
    const float c = azn_div(1.0f, azn_sqrt(azn_mul(9.0f, d)));
    float g = A;
    for (int r = 0; r < NOISE_ROUNDS; ++r) {
        const float v1 = azn_sub(azn_mul(2.0f, noise_uniform(noise_draw(stream, a, 3ull * r))), 1.0f);
        const float v2 = azn_sub(azn_mul(2.0f, noise_uniform(noise_draw(stream, a, 3ull * r + 1))), 1.0f);
        const float s = azn_add(azn_mul(v1, v1), azn_mul(v2, v2));
        if (!(s > 0.0f && s < 1.0f)) continue;
        const float x = azn_mul(v1, azn_sqrt(azn_div(azn_mul(-2.0f, noise_ln(s)), s)));
        float v = azn_add(1.0f, azn_mul(c, x));
        if (!(v > 0.0f)) continue;
        v = azn_mul(azn_mul(v, v), v);
        if (v < 1.17549435e-38f) continue;
        const float lhs = noise_ln(noise_uniform(noise_draw(stream, a, 3ull * r + 2)));
        const float rhs = azn_add(azn_add(azn_mul(0.5f, azn_mul(x, x)), azn_sub(d, azn_mul(d, v))), azn_mul(d, noise_ln(v)));
        if (lhs < rhs) { g = azn_mul(d, v); break; }
    }
    if (boost) g = azn_mul(g, noise_exp2(azn_div(noise_log2(noise_uniform(noise_draw(stream, a, NOISE_BOOST_DRAW))), alpha)));
    return g;
}

// eta[a] of one variate, given the sum over the root's valid actions and their number
AZN_HD float noise_normalise(float g, float sum, uint32_t n_valid) { return sum > 0.0f ? azn_div(g, sum) : azn_div(1.0f, (float)n_valid); }
AZN_HD float noise_mix(float eps, float prior, float eta) { return azn_add(azn_mul(azn_sub(1.0f, eps), prior), azn_mul(eps, eta)); }

// eta[0 .. n_actions) of the root (seed, game_id, ply) with the given valid-move mask (bit a = action a is valid); n_actions <= 8
inline void noise_eta(uint64_t seed, uint64_t game_id, uint64_t ply, float alpha, uint32_t valid_mask, int n_actions, float* eta) {
    const uint64_t stream = noise_stream(seed, game_id, ply);
    float g[8];
    float sum = 0.0f;
    uint32_t k = 0;
    for (int a = 0; a < n_actions; ++a) {
        g[a] = 0.0f;
        if (!((valid_mask >> a) & 1u)) continue;
        g[a] = noise_gamma(stream, (uint32_t)a, alpha);
        sum = azn_add(sum, g[a]);
        ++k;
    }
    for (int a = 0; a < n_actions; ++a) eta[a] = ((valid_mask >> a) & 1u) ? noise_normalise(g[a], sum, k) : 0.0f;
}

}  // namespace az
