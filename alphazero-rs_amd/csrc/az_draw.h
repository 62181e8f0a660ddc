// az_draw.h -- multiplicity-weighted batch draws of NNet::train (az_net_train_samples / az_net_train_draw, include/az_engine.h; DESIGN.md
// section 8.2).  The RULE is HIP-free apart from the host/device qualifier (AZW_HD, as az_forced.h has AZF_HD): the draw kernel of
// az_draw.hip, the engine's host code and the g++ twin of the tests (tests/cpp/train_draw_twin.cpp) compile this text.  Integer operations
// only, so every side gives the same bits.
//
// n tuples with u32 weights w (NULL = all ones; a weight of 0 is legal).  Q[i] = w[0] + .. + w[i] in u64, W = Q[n-1] > 0.
//   row j of global step t   r = rng_draw(train_seed, t, j, RNG_BATCH) -- az_net_train's own draw -- then u = (r * W) >> 64 (the 128-bit
//                            product), and the row is tuple i = min{ i : Q[i] > u }: tuple i is drawn with probability w[i] / W, a tuple of
//                            weight 0 never.  With every weight 1, Q[i] = i + 1 and i = u = az_net_train's row
//   mirrored                 iff the top bit of rng_draw(train_seed, t, j, RNG_TRAIN_MIRROR) is set (AZ_TRAIN_MIRROR only)
//   steps of an epoch        max(1, S / train_batch), S = n, or W under AZ_TRAIN_EPOCH_BY_WEIGHT
// The launchers at the end (HIP only) are the device side: the u64 prefix sum Q and the draw kernel.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define AZW_HD __host__ __device__ __forceinline__
#else
#define AZW_HD inline
#endif

namespace az {

constexpr int64_t DRAW_MAX_TUPLES = 2147483647ll;      // 2^31 - 1
// the purpose words of az_common.h, restated so that this header stands alone (az_draw.hip asserts that they agree)
constexpr uint64_t DRAW_RNG_BATCH = 4, DRAW_RNG_TRAIN_MIRROR = 9;
constexpr int32_t DRAW_EPOCH_BY_WEIGHT = 1, DRAW_MIRROR = 2;       // AZ_TRAIN_EPOCH_BY_WEIGHT, AZ_TRAIN_MIRROR

AZW_HD uint64_t draw_mix64(uint64_t x) {            // mix64 of az_common.h
    x += 0x9E3779B97F4A7C15ull;
    uint64_t z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
AZW_HD uint64_t draw_rng(uint64_t seed, uint64_t t, uint64_t j, uint64_t purpose) {      // rng_draw of az_common.h
    return draw_mix64(draw_mix64(draw_mix64(draw_mix64(seed) ^ t) ^ j) ^ purpose);
}
AZW_HD uint64_t draw_mulhi(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * (unsigned __int128)b) >> 64);
#endif
}
// u of row j of global step t: uniform on 0 .. W-1
AZW_HD uint64_t draw_u(uint64_t seed, uint64_t t, uint64_t j, uint64_t W) { return draw_mulhi(draw_rng(seed, t, j, DRAW_RNG_BATCH), W); }
// min{ i : Q[i] > u } over the non-decreasing Q[0 .. n); u < Q[n-1] is the caller's (u < W)
AZW_HD int64_t draw_search(const uint64_t* Q, int64_t n, uint64_t u) {
    int64_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (Q[mid] > u) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}
// the row's tuple; Q == NULL: all weights 1 (W = n)
AZW_HD int64_t draw_row(const uint64_t* Q, int64_t n, uint64_t W, uint64_t seed, uint64_t t, uint64_t j) {
    const uint64_t u = draw_u(seed, t, j, W);
    return Q ? draw_search(Q, n, u) : (int64_t)u;
}
AZW_HD bool draw_mirrored(uint64_t seed, uint64_t t, uint64_t j) { return (draw_rng(seed, t, j, DRAW_RNG_TRAIN_MIRROR) >> 63) != 0; }
// steps of an epoch over S tuples (or S units of weight) at batch b
AZW_HD int64_t draw_epoch_steps(uint64_t S, int64_t b) {
    const uint64_t s = S / (uint64_t)b;
    return s < 1 ? 1 : (int64_t)s;
}
// inclusive u64 prefix sum on the host (the twin's, and what the device scan must equal); returns W
inline uint64_t draw_prefix(const uint32_t* w, int64_t n, uint64_t* Q) {
    uint64_t acc = 0;
    for (int64_t i = 0; i < n; ++i) {
        acc += w ? (uint64_t)w[i] : 1ull;
        Q[i] = acc;
    }
    return acc;
}

#if defined(__HIPCC__)
// ---- device side (az_draw.hip) -------------------------------------------------------------------------------------------------------
constexpr uint32_t DRAW_SCAN_THREADS = 256, DRAW_SCAN_ITEMS = 8;
constexpr uint32_t DRAW_SCAN_BLOCK = DRAW_SCAN_THREADS * DRAW_SCAN_ITEMS;     // B: weights per workgroup of the first and third pass
constexpr uint32_t DRAW_SCAN_GROUP = 1024;                                   // G: block sums the one workgroup of the second pass takes per round
inline size_t draw_scan_blocks(int64_t n) { return ((size_t)n + DRAW_SCAN_BLOCK - 1) / DRAW_SCAN_BLOCK; }
// Q[0 .. n) = the inclusive prefix sum of w (device, [n]); bsum: draw_scan_blocks(n) u64 of workspace; *total = W.  n in 1 .. 2^31 - 1
void launch_draw_scan(const uint32_t* w, int64_t n, uint64_t* Q, uint64_t* bsum, uint64_t* total, hipStream_t s);
// rows k = 0 .. steps*b of global steps t0 .. t0 + steps: idx[k] = the tuple of row k % b of step t0 + k / b, mir[k] = 1 iff mirrored (0
// throughout unless `mirror`).  Q == NULL: all weights 1 and W = n
void launch_draw_rows(const uint64_t* Q, int64_t n, uint64_t W, uint64_t seed, uint64_t t0, int64_t steps, int b, bool mirror, int64_t* idx,
                      uint8_t* mir, hipStream_t s);
// *bad |= sample_state_bits of az_samples.h: a state with overlapping stones or bits outside the 7 x 6 board
void launch_draw_check_states(const ulonglong2* states, int64_t n, uint32_t* bad, hipStream_t s);
#endif

}  // namespace az
