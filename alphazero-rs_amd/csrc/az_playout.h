// az_playout.h -- playout cap randomization ("playout_cap_sims" / "playout_cap_full_e6", include/az_engine.h): which moves of a self-play
// episode get the full simulation budget.  HIP-free apart from the host/device qualifier (AZP_HD, as az_noise.h has AZN_HD): the tree kernels, the engine's host code and the g++
// twin of the tests (tests/cpp/selfplay_twin.cpp) compile this text.
#pragma once
#include <cstdint>
#if defined(__HIPCC__)
#define AZP_HD __host__ __device__ __forceinline__
#else
#define AZP_HD inline
#endif

namespace az {

constexpr uint64_t RNG_PLAYOUT_CAP = 6;      // the purpose word of the mode draw (az_common.h: 1 .. 5 are taken)
constexpr int64_t PLAYOUT_CAP_MAX_SIMS = 65535, PLAYOUT_CAP_E6 = 1000000;

AZP_HD uint64_t playout_mix64(uint64_t x) {   // mix64 of az_common.h, restated so that this header stands alone
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
// thresh24 = (P * 2^24) / 1000000, unsigned 64-bit: P = 1000000 gives 2^24 (every 24-bit draw is below it), P = 0 gives 0 (none is)
AZP_HD uint32_t playout_cap_thresh24(uint64_t full_e6) { return (uint32_t)((full_e6 << 24) / 1000000ull); }
// the move of episode game_id at ply (stones on the board) is a FULL move: rng_draw(seed, game_id, ply, RNG_PLAYOUT_CAP) >> 40 < thresh24
AZP_HD bool playout_cap_full(uint64_t seed, uint64_t game_id, uint64_t ply, uint32_t thresh24) {
    const uint64_t r = playout_mix64(playout_mix64(playout_mix64(playout_mix64(seed) ^ game_id) ^ ply) ^ RNG_PLAYOUT_CAP);
    return (uint32_t)(r >> 40) < thresh24;
}
// A slot's word for its current move: the budget in the low 31 bits, bit 31 = the move is full.
constexpr uint32_t PLAYOUT_FULL_BIT = 0x80000000u;
AZP_HD uint32_t playout_cap_word(uint64_t seed, uint64_t game_id, uint64_t ply, uint32_t thresh24, uint32_t num_sims, uint32_t cap_sims) {
    return playout_cap_full(seed, game_id, ply, thresh24) ? (num_sims | PLAYOUT_FULL_BIT) : cap_sims;
}

}  // namespace az
