// az_fp8.h -- the quantiser of the "net_fp8" numerics class (include/az_engine.h): OCP e4m3fn codes,
// the power-of-two scale rules and the index math of the packed fp8 weight copies.  Plain C++ with no HIP in it, so the host side
// of az_net.hip and a g++ unit test (tests/cpp/test_fp8_cpu.cpp) compile the same code.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

namespace az {

constexpr float FP8_MAX = 448.0f;            // largest finite e4m3fn value (code 0x7E); 0x7F / 0xFF are NaN, there is no infinity

// f32 -> e4m3fn, round to nearest even, SATURATING: |x| > 448 (infinities included) gives +-448; NaN gives the NaN code.
inline uint8_t fp8_e4m3_from_f32(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    const uint8_t sign = (uint8_t)((u >> 24) & 0x80u);
    u &= 0x7FFFFFFFu;
    if (u > 0x7F800000u) return (uint8_t)(sign | 0x7Fu);
    if (u >= 0x43E00000u) return (uint8_t)(sign | 0x7Eu);                  // >= 448: saturate (464, the first value that would round up, too)
    if (u < 0x3C800000u) {                                                   // < 2^-6: the subnormal codes, steps of 2^-9
        float a;
        std::memcpy(&a, &u, 4);
        const float r = std::nearbyint(a * 512.0f);                          // exact product; ties to even (default rounding mode)
        return (uint8_t)(sign | (uint8_t)r);                                 // r == 8 is the code of 2^-6, the first normal
    }
    const uint32_t r = u + 0x7FFFFu + ((u >> 20) & 1u);                      // keep 3 mantissa bits, ties to even; a carry moves the exponent
    const uint32_t e = (r >> 23) - 120u, m = (r >> 20) & 7u;                 // bias 127 -> 7
    return (uint8_t)(sign | (e << 3) | m);                                   // at most 0x7E: inputs below 448 round to at most 448
}

inline float fp8_e4m3_to_f32(uint8_t c) {
    const int e = (c >> 3) & 15, m = c & 7;
    float a;
    if (e == 15 && m == 7) a = NAN;
    else if (e == 0) a = std::ldexp((float)m, -9);
    else a = std::ldexp((float)(8 + m), e - 10);
    return (c & 0x80u) ? -a : a;
}

// 2^floor(log2(448 / amax)): the largest power of two s with amax * s <= 448; 1 for amax == 0 (or not finite).  Exact: from the
// binary exponent of amax, no division and no logarithm.
inline float fp8_pow2_scale(float amax) {
    if (!(amax > 0.0f) || std::isinf(amax)) return 1.0f;
    int e;
    const float m = std::frexp(amax, &e);                                    // amax = m * 2^e, m in [0.5, 1); 448 = 0.875 * 2^9
    int k = m <= 0.875f ? 9 - e : 8 - e;
    k = k < -126 ? -126 : k > 126 ? 126 : k;
    return std::ldexp(1.0f, k);
}
inline float fp8_weight_scale(float amax_row) { return fp8_pow2_scale(amax_row); }                  // sw[n], per output channel
constexpr float FP8_ACT_HEADROOM = 4.0f;
inline float fp8_act_scale(float amax_calib) { return fp8_pow2_scale(FP8_ACT_HEADROOM * amax_calib); }   // sa2 / sa3, per tensor

// ---- the packed weight copy of a 3x3 conv layer (ConvNet::w8): the LDS-DMA ring's stage images --------------------------------------
// [N / 128 column tiles][K-steps][128 rows][128 B]; one K-step = one filter tap x 128 input channels, walked channel block outer, tap
// inner; inside a row the 16-byte chunk c sits at slot c ^ (row & 7) (the ring's LDS swizzle, applied here because a stage is copied
// as it is), channels in natural order inside a chunk.  A lane of the 16x16x128 MFMA reads chunks q and 4 + q (q = lane >> 4) of its
// activation row and of its weight row, so both operands pair the same channels whatever the instruction's k order is.
constexpr int FP8_KSTEP = 128;
inline int64_t fp8_ring_steps(int C) { return (int64_t)(C / FP8_KSTEP) * 9; }
inline int64_t fp8_ring_offset(int C, int n, int tap, int c) {              // byte offset of weight (output channel n, tap, input channel c)
    const int nt = n >> 7, r = n & 127, cb = c / FP8_KSTEP, cc = c % FP8_KSTEP;
    const int64_t step = (int64_t)cb * 9 + tap;
    return ((nt * fp8_ring_steps(C) + step) * 128 + r) * 128 + (((cc >> 4) ^ (r & 7)) << 4) + (cc & 15);
}

// ---- the calibration set: a constant of the library ----------------------------------------------------------------------------------
constexpr int FP8_CALIB_POSITIONS = 1024;
constexpr uint64_t FP8_CALIB_SEED = 0xF8CA11B8ull;

}  // namespace az
