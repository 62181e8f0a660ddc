// az_gumbel.h -- Gumbel root search with sequential halving ("gumbel_m" / "gumbel_c_visit_e6" / "gumbel_c_scale_e6", include/az_engine.h;
// Danihelka et al., ICLR 2022, "Policy improvement by planning with Gumbel").  HIP-free apart from the host/device
// qualifier (AZG_HD, as az_forced.h has AZF_HD): the tree kernels and the g++ twin of the tests (tests/cpp/gumbel_twin.cpp) compile this
// text, and both give the same bits.  Integer operations and correctly rounded f32 + - * / only -- the azn_* wrappers of az_noise.h:
// explicit *_rn intrinsics on the device, plain operators under g++ -O2 -ffp-contract=off -- plus noise_ln / noise_exp2 of az_noise.h.
//
// THE SCHEME (everything a second implementation needs to reproduce a Gumbel move bit for bit; all arithmetic is IEEE f32, round to
// nearest even, in exactly the operation order written below).  A root has nchild <= 7 child SLOTS j in ascending action order; slot j
// has the action a_j, the stored prior p_j (with the root noise mixed in when that is on), the resolved visit count n_j and q_j, the q
// of PUCT ((W - vloss) / n, 0 when n == 0).
//   baseline   once per move, after the root has its prior and before the move's first selection: base_j = n_j (u16).  d_j = (n_j - base_j)
//              mod 2^16 is the slot's visits in THIS move, and t = sum_j d_j the index of the current simulation within the move.
//              One repair keeps that true: a slot that is still a placeholder (n_j = 0) and whose first visit finds its state in the
//              tree already -- a node an earlier move built -- becomes a link to that node; base_j is then set to that node's visit count
//              before the visit.  (Only the root's arg-max routes a simulation into a root child: a root child has one stone more than
//              the root, every other node below the root at least two.)
//   variate    r = rng_draw(seed, game_id, ply, 8 + 256 * a_j)    (rng_draw / mix64: az_common.h; purpose RNG_GUMBEL = 8)
//              U = ((float)(r >> 41) + 0.5f) * 2^-23              exact: a 23-bit integer plus one half, strictly inside (0, 1)
//              g_j = -ln(-ln(U))                                  ln = noise_ln; both negations are exact
//              g_j = 0 for every slot when the move's temperature is 0.
//   logit      l_j = ln(max(p_j, 2^-126))
//   considered m_eff = min(m, nchild); n = the move's budget; c(t) = gumbel_considered_visit(m_eff, n, t): entry t of the sequence of
//              considered visit counts of sequential halving -- integer arithmetic only, the loop is written out below.
//   value      v_mix = (sum_{n_b > 0} p_b * q_b) / (sum_{n_b > 0} p_b), both sums from 0.0f in ascending slot order; 0 when the
//              denominator is not > 0 (no slot visited).  qh_j = n_j > 0 ? q_j : v_mix.
//              sigma_j = ((c_visit + (float)max_b n_b) * c_scale) * qh_j
//   selection  at the first level of a simulation: s_j = (g_j + l_j) + sigma_j for the slots with d_j == c(t), -inf for every other;
//              arg-max with the fold of best_child (the later slot wins unless the earlier one is strictly greater).
//   result     selected = the arg-max of s_j over the slots with d_j == max_b d_b, same fold.
//              x_j = l_j + sigma_j;  e_j = exp2((x_j - max_b x_b) * 0x3FB8AA3B (log2 e));  pi[a_j] = e_j / sum_b e_b, the sum from 0.0f
//              in ascending slot order.  Actions without a slot get 0.  The temperature does not enter.
// Measured against -log(-log(U)) in float64 (tests/test_gumbel_cpu.py) on the 4096 smallest and the 4096 largest values of U, the 8192
// around U = 1/e (where the inner logarithm crosses 1 and g crosses 0) and 2^20 random ones: |g - exact| <= 3.3e-7 * max(1, |exact|), g in
// [-2.82, 16.64].  The test asserts 6.6e-7: the inner logarithm's relative error e <= 3.3e-7 (az_noise.h: 2.7e-7 for noise_log2, plus the
// rounding of the ln 2 product) is an absolute error of the outer one, which adds e * |g| of its own.
#pragma once
#include <stdint.h>
#include "az_noise.h"

#if defined(__HIPCC__)
#define AZG_HD __host__ __device__ __forceinline__
#else
#define AZG_HD inline
#endif

namespace az {

constexpr uint64_t GUMBEL_PURPOSE = 8;           // RNG_GUMBEL: purposes 1 .. 7 are taken (az_common.h, az_noise.h, az_playout.h, az_opening.h)
constexpr int GUMBEL_M_MIN = 2, GUMBEL_M_MAX = 7;
constexpr int64_t GUMBEL_C_VISIT_E6_MAX = 1000000000, GUMBEL_C_VISIT_E6_DEFAULT = 50000000;
constexpr int64_t GUMBEL_C_SCALE_E6_MIN = 1, GUMBEL_C_SCALE_E6_MAX = 100000000, GUMBEL_C_SCALE_E6_DEFAULT = 1000000;

// c_visit / c_scale of the option value: the division in double, rounded once to f32 (as eps of "root_noise_eps_e6")
inline float gumbel_of_e6(int64_t v_e6) { return (float)((double)v_e6 / 1e6); }

AZG_HD float gumbel_uniform(uint64_t r) { return azn_mul(azn_add((float)(uint32_t)(r >> 41), 0.5f), 1.1920928955078125e-7f); }
// g of a uniform: -ln(-ln(U))
AZG_HD float gumbel_of_uniform(float u) { return -noise_ln(-noise_ln(u)); }
// the variate of the slot with action a of the root (seed, game_id, ply)
AZG_HD float gumbel_variate(uint64_t seed, uint64_t game_id, uint64_t ply, uint32_t a, bool temp_is_zero) {
    if (temp_is_zero) return 0.0f;
    const uint64_t r = noise_mix64(noise_stream(seed, game_id, ply) ^ (GUMBEL_PURPOSE + 256ull * a));      // == rng_draw(seed, game_id, ply, 8 + 256 * a)
    return gumbel_of_uniform(gumbel_uniform(r));
}
AZG_HD float gumbel_logit(float p) { return noise_ln(p > 1.17549435e-38f ? p : 1.17549435e-38f); }

// entry t of the sequence of considered visit counts for m_eff considered actions and a budget of n simulations
AZG_HD uint32_t gumbel_considered_visit(uint32_t m_eff, uint32_t n, uint32_t t) {
    if (m_eff <= 1u) return t;
    uint32_t L = 0u;
    while ((1u << L) < m_eff) ++L;                       // ceil(log2 m_eff), 1 .. 3
    uint32_t k = m_eff, v = 0u;
    for (;;) {
        const uint32_t e0 = n / (L * k);
        const uint32_t extra = e0 > 1u ? e0 : 1u;
        const uint32_t block = extra * k;
        if (t < block) return v + t / k;
        t -= block;
        v += extra;
        k = k / 2u > 2u ? k / 2u : 2u;
    }
}

// v_mix: add the slots in ascending order, then take the quotient
struct GumbelMix { float num, den; };
AZG_HD void gumbel_mix_add(GumbelMix& mx, float p, float q, uint32_t n) {
    if (n > 0u) { mx.num = azn_add(mx.num, azn_mul(p, q)); mx.den = azn_add(mx.den, p); }
}
AZG_HD float gumbel_vmix(const GumbelMix& mx) { return mx.den > 0.0f ? azn_div(mx.num, mx.den) : 0.0f; }
AZG_HD float gumbel_sigma(float c_visit, float c_scale, uint32_t max_n, uint32_t n, float q, float v_mix) {
    return azn_mul(azn_mul(azn_add(c_visit, (float)max_n), c_scale), n > 0u ? q : v_mix);
}
AZG_HD float gumbel_score(float g, float l, float sigma) { return azn_add(azn_add(g, l), sigma); }
AZG_HD float gumbel_x(float l, float sigma) { return azn_add(l, sigma); }
AZG_HD float gumbel_softmax_term(float x, float max_x) { return noise_exp2(azn_mul(azn_sub(x, max_x), 1.44269504f)); }

// ---- the whole rule over the slots of one root, as plain loops (the twin and the tests; the kernels hold one slot per lane and fold with
// shuffles, calling the same pieces in the same order) ----
constexpr int GUMBEL_SLOTS = 7;
struct GumbelRoot {
    uint32_t nchild;
    float p[GUMBEL_SLOTS], q[GUMBEL_SLOTS], g[GUMBEL_SLOTS];
    uint32_t n[GUMBEL_SLOTS], base[GUMBEL_SLOTS];
};
inline uint32_t gumbel_d(const GumbelRoot& r, uint32_t j) { return (r.n[j] - r.base[j]) & 0xFFFFu; }
inline void gumbel_sigmas(const GumbelRoot& r, float c_visit, float c_scale, float* sigma) {
    GumbelMix mx{0.0f, 0.0f};
    uint32_t max_n = 0u;
    for (uint32_t j = 0; j < r.nchild; ++j) { gumbel_mix_add(mx, r.p[j], r.q[j], r.n[j]); if (r.n[j] > max_n) max_n = r.n[j]; }
    const float v_mix = gumbel_vmix(mx);
    for (uint32_t j = 0; j < r.nchild; ++j) sigma[j] = gumbel_sigma(c_visit, c_scale, max_n, r.n[j], r.q[j], v_mix);
}
// the arg-max of s_j over the slots with d_j == want; *found = whether any slot had it (else the last slot is returned, as the fold does)
inline uint32_t gumbel_argmax(const GumbelRoot& r, float c_visit, float c_scale, uint32_t want, bool* found) {
    float sigma[GUMBEL_SLOTS];
    gumbel_sigmas(r, c_visit, c_scale, sigma);
    uint32_t best = 0u;
    float bu = 0.0f;
    bool any = false;
    for (uint32_t j = 0; j < r.nchild; ++j) {
        const bool ok = gumbel_d(r, j) == want;
        const float u = ok ? gumbel_score(r.g[j], gumbel_logit(r.p[j]), sigma[j]) : -__builtin_inff();
        any = any || ok;
        if (j == 0u || !(bu > u)) { best = j; bu = u; }
    }
    if (found) *found = any;
    return best;
}
// the slot a simulation of the move goes to (m, n: "gumbel_m" and the move's budget)
inline uint32_t gumbel_select(const GumbelRoot& r, uint32_t m, uint32_t n, float c_visit, float c_scale, bool* found) {
    uint32_t t = 0u;
    for (uint32_t j = 0; j < r.nchild; ++j) t += gumbel_d(r, j);
    const uint32_t m_eff = m < r.nchild ? m : r.nchild;
    return gumbel_argmax(r, c_visit, c_scale, gumbel_considered_visit(m_eff, n, t), found);
}
// the move's result: the selected slot and pi by slot
inline uint32_t gumbel_result(const GumbelRoot& r, float c_visit, float c_scale, float* pi_slot) {
    uint32_t max_d = 0u;
    for (uint32_t j = 0; j < r.nchild; ++j) if (gumbel_d(r, j) > max_d) max_d = gumbel_d(r, j);
    float sigma[GUMBEL_SLOTS], x[GUMBEL_SLOTS], e[GUMBEL_SLOTS];
    gumbel_sigmas(r, c_visit, c_scale, sigma);
    float max_x = 0.0f;
    for (uint32_t j = 0; j < r.nchild; ++j) {
        x[j] = gumbel_x(gumbel_logit(r.p[j]), sigma[j]);
        if (j == 0u || x[j] > max_x) max_x = x[j];
    }
    float sum = 0.0f;
    for (uint32_t j = 0; j < r.nchild; ++j) { e[j] = gumbel_softmax_term(x[j], max_x); sum = azn_add(sum, e[j]); }
    for (uint32_t j = 0; j < r.nchild; ++j) pi_slot[j] = azn_div(e[j], sum);
    return gumbel_argmax(r, c_visit, c_scale, max_d, nullptr);
}

}  // namespace az
