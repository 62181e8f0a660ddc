// az_score.h -- held-out loss of a net as self-play runs it (az_net_evaluate), the hold-out rule (az_samples_holdout) and the best-epoch /
// patience decision of NNet::train's per-epoch validation (include/az_engine.h; DESIGN.md sections 4.1l and 8.3).  The RULE is HIP-free
// apart from the host/device qualifier (AZS_HD, as az_target.h has AZT_HD): the kernels of az_score.hip and the g++ twin of the tests
// (tests/cpp/score_twin.cpp, g++ -O2 -ffp-contract=off) compile this text.  f32 through az_noise.h's azn_*, f64 through az_target.h's azt_d*.
//
//   per tuple    from the net's output (p[0..6], v) for the state, the target (pi[0..6], z) and the state (mine, theirs):
//     ce         t = 0.0f;  for a ascending with pi[a] >= 2^-126:  t = t + pi[a] * noise_log2(p[a] > 2^-126 ? p[a] : 2^-126)
//                ce = -(t * 0x3F317218), clamped to [0, 128]: a NaN gives 128, anything not above 0 gives +0
//     kl         target_kl(pi, p) of az_target.h, unchanged
//     se         d = v - z, se = d * d; a NaN or anything above 4 (no net with a tanh value head gives one) counts as 4
//     hit        t* = the lowest a that maximises pi[a]; m* = the lowest LEGAL a that maximises p[a] (a column is legal while its top cell
//                is empty; a NaN p[a] never is the maximum); hit = (t* == m*)
//   fixed point  K(x) = (uint64_t)llrint((double)x * 2^30)
//   sums         S_ce = sum w_i K(ce_i), S_kl, S_se likewise, S_hit = sum w_i hit_i, W = sum w_i in u64: integer sums, so no result depends
//                on the order of the additions.  1 <= n <= 2^24 and 1 <= W <= 2^24 keep every sum below 2^62 (K <= 128 * 2^30)
//   results      loss_pi = S_ce / 2^30 / W, kl = S_kl / 2^30 / W, loss_v = S_se / 2^30 / W, top1 = S_hit / W: doubles from the integers
//   hold-out     held = (mix64(mix64(seed) ^ k) >> 40) < thresh24, k = the pack word of the tuple's mirror-canonical state (the key of
//                az_samples_merge under AZ_MERGE_CANONICAL: a position and its mirror image share it), thresh24 = share_e6 * 2^24 / 1000000
//   best / stop  over a history of (loss_pi + loss_v) per epoch: best = the first epoch of the lowest sum; with patience P > 0 training
//                stops behind the first epoch that ends P consecutive epochs without a new best
#pragma once
#include "az_target.h"      // first: under hipcc it brings the runtime header az_mirror.h's qualifiers need
#include "az_mirror.h"

#if defined(__HIPCC__)
#define AZS_HD __host__ __device__ __forceinline__
#else
#define AZS_HD inline
#endif

namespace az {

constexpr int64_t SCORE_MAX_TUPLES = 1ll << 24;
constexpr uint64_t SCORE_MAX_WEIGHT = 1ull << 24;
constexpr float SCORE_CE_MAX = 128.0f, SCORE_SE_MAX = 4.0f;
constexpr int SCORE_SUMS = 5;                 // S_ce, S_kl, S_se, S_hit, W
constexpr int SCORE_MAX_PATIENCE = 1000;

AZS_HD float score_ce(const float* pi, const float* p) {
    float t = 0.0f;
    for (int a = 0; a < TARGET_ACTIONS; ++a) {
        if (!(pi[a] >= TARGET_MIN_NORMAL)) continue;
        const float q = p[a] > TARGET_MIN_NORMAL ? p[a] : TARGET_MIN_NORMAL;
        t = azn_add(t, azn_mul(pi[a], noise_log2(q)));
    }
    const float ce = -azn_mul(t, 0.693147182f);          // 0x3F317218
    if (ce != ce) return SCORE_CE_MAX;
    if (!(ce > 0.0f)) return 0.0f;
    return ce > SCORE_CE_MAX ? SCORE_CE_MAX : ce;
}
AZS_HD float score_se(float v, float z) {
    const float d = azn_sub(v, z);
    const float se = azn_mul(d, d);
    return !(se <= SCORE_SE_MAX) ? SCORE_SE_MAX : se;
}
// a column is legal while its top cell (bit c * 7 + 5, az_game.h) is empty
AZS_HD bool score_legal(uint64_t mine, uint64_t theirs, int a) { return ((mine | theirs) & (1ull << (a * 7 + 5))) == 0ull; }
AZS_HD uint32_t score_hit(const float* pi, const float* p, uint64_t mine, uint64_t theirs) {
    int ts = 0, ms = -1;
    float best = 0.0f;
    for (int a = 1; a < TARGET_ACTIONS; ++a)
        if (pi[a] > pi[ts]) ts = a;
    for (int a = 0; a < TARGET_ACTIONS; ++a) {
        if (!score_legal(mine, theirs, a) || p[a] != p[a]) continue;
        if (ms < 0 || p[a] > best) { ms = a; best = p[a]; }
    }
    return ts == ms ? 1u : 0u;
}
AZS_HD uint64_t score_fixed(float x) { return (uint64_t)azt_llrint(azt_dmul((double)x, 1073741824.0)); }      // 2^30

// the hold-out rule
AZS_HD uint64_t score_thresh24(uint64_t share_e6) { return (share_e6 << 24) / 1000000ull; }
AZS_HD uint64_t score_holdout_key(uint64_t mine, uint64_t theirs) {
    const MirrorCanon c = mirror_canonical(mine, theirs);
    return mirror_key(c.mine, c.theirs);
}
AZS_HD bool score_held(uint64_t seed, uint64_t key, uint64_t thresh24) { return (target_mix64(target_mix64(seed) ^ key) >> 40) < thresh24; }

// The best / stop decision behind epoch n (1-based count of epochs run so far): hist[2 * k] + hist[2 * k + 1] (one double addition) is epoch
// k's loss_pi + loss_v, hist having `stride` doubles per epoch.  *best = the first epoch of the lowest sum (a NaN sum never is a new best;
// with nothing but NaN, epoch 0).  Returns true when patience > 0 and the last `patience` epochs brought no new best.
inline bool score_best_stop(const double* hist, int stride, int n, int patience, int* best) {
    int b = 0;
    bool have = false;
    double lo = 0.0;
    for (int k = 0; k < n; ++k) {
        const double s = hist[(size_t)k * stride] + hist[(size_t)k * stride + 1];
        if (s != s) continue;
        if (!have || s < lo) { have = true; lo = s; b = k; }
    }
    *best = b;
    return patience > 0 && n - 1 - b >= patience;
}

#if defined(__HIPCC__)
// ---- device side (az_score.hip) --------------------------------------------------------------------------------------------------------
// one thread per tuple: sample_check of az_samples.h (strict = its strict_pi); out[i] = the state, or the empty board where the tuple is
// refused (nothing invalid ever reaches a forward); *bad |= the verdict bits
void launch_score_states(const SampleWindow& w, int strict, int64_t n, ulonglong2* out, uint32_t* bad, hipStream_t s);
// one thread per row of a chunk: tuple first + r scores net_pi[r * 8 .. + 7) and net_v[r] (an EvalBatch's rows, read in place) against its
// target; sums[0 .. 5) += the workgroup's integers (one 64-bit atomic per workgroup and sum); ce / se / kl [n] may be nullptr
void launch_score(const float* net_pi, const float* net_v, const ulonglong2* states, const float* pis, const float* zs, const uint32_t* weights,
                  int64_t first, int rows, uint64_t* sums, float* ce, float* se, float* kl, hipStream_t s);
// held[i] = score_held(seed, score_holdout_key(states[i]), thresh24)
void launch_score_holdout(const ulonglong2* states, int64_t n, uint64_t seed, uint64_t thresh24, uint8_t* held, hipStream_t s);
#endif

}  // namespace az
