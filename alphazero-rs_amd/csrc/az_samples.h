// az_samples.h -- what every entry that takes a window of training tuples (an az_samples: states or boards, pis, zs) refuses in a tuple,
// and the sentences it refuses with: az_samples_merge, az_samples_surprise, az_net_evaluate, az_samples_holdout,
// az_net_train_set_validation and the states of az_net_train_samples (include/az_engine.h; DESIGN.md section 4.1g, "the window check").
// The RULE is HIP-free apart from the host/device qualifier (AZV_HD, as az_target.h has AZT_HD): k_merge_keys, k_target_kl, k_score_states
// and k_draw_check_states and the g++ twin of the tests (tests/cpp/samples_twin.cpp) compile this text.
//
//   state      given as (mine, theirs), or rebuilt from the two feature planes (the inverse of Game::feature: plane 0 = the side to move,
//              row 0 = top, cell (r, c) = bit c * 7 + (5 - r)); a feature that is not 0 or 1, or a cell set in both planes: SAMPLE_BAD_FEATURE
//              stones of both sides on one cell, or a bit outside the 7 x 6 board: SAMPLE_BAD_STATE
//   values     every pi[a] in [-1, 1], or in [0, 1] where the entry scores the pi as a distribution (strict_pi); z in [-1, 1]; a NaN fails
//              every range test: SAMPLE_BAD_VALUE
//   priors     SAMPLE_BAD_PRIOR is az_samples_surprise's alone (k_target_kl tests them next to the pi it loads them with)
#pragma once
#include <stddef.h>
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define AZV_HD __host__ __device__ __forceinline__
#else
#define AZV_HD inline
#endif

namespace az {

constexpr uint32_t SAMPLE_BAD_VALUE = 1u, SAMPLE_BAD_STATE = 2u, SAMPLE_BAD_FEATURE = 4u, SAMPLE_BAD_PRIOR = 8u;      // verdict bits
// the 42 cells of the board: C4_FULL of az_game.h, restated so that this header stands alone (az_merge.hip asserts that they agree)
constexpr uint64_t SAMPLE_BOARD = 0x3Full | (0x3Full << 7) | (0x3Full << 14) | (0x3Full << 21) | (0x3Full << 28) | (0x3Full << 35) | (0x3Full << 42);

#if defined(__HIPCC__)
typedef ulonglong2 SampleState;
#else
struct SampleState { uint64_t x, y; };      // the caller's [n][2] uint64, which promises no more than 8-byte alignment
#endif

// a window of n tuples: states [n], or (states == nullptr) boards [n][84]; pis [n][7]; zs [n]
struct SampleWindow { const SampleState* states; const float* boards; const float* pis; const float* zs; };

// a NaN fails both comparisons
AZV_HD bool sample_in_unit(float x) { return x >= -1.0f && x <= 1.0f; }
AZV_HD bool sample_is_prior(float x) { return x >= 0.0f && x <= 1.0f; }

AZV_HD uint32_t sample_state_bits(uint64_t mine, uint64_t theirs) {
    return ((mine & theirs) || ((mine | theirs) & ~SAMPLE_BOARD)) ? SAMPLE_BAD_STATE : 0u;
}
// the state of 84 feature cells; returns the feature verdict (the state holds the cells that are exactly 1 either way)
AZV_HD uint32_t sample_state_from_planes(const float* f, uint64_t* mine, uint64_t* theirs) {
    uint32_t bad = 0u;
    uint64_t m = 0, t = 0;
    for (int r = 0; r < 6; ++r)
        for (int c = 0; c < 7; ++c) {
            const float a = f[r * 7 + c], o = f[42 + r * 7 + c];
            const bool a1 = a == 1.0f, o1 = o == 1.0f;
            if (!((a1 || a == 0.0f) && (o1 || o == 0.0f)) || (a1 && o1)) bad = SAMPLE_BAD_FEATURE;
            const uint64_t bit = 1ull << (c * 7 + (5 - r));
            if (a1) m |= bit;
            if (o1) t |= bit;
        }
    *mine = m;
    *theirs = t;
    return bad;
}
// the verdict bits of tuple i of a window, and its state
AZV_HD uint32_t sample_check(const SampleWindow& w, int64_t i, bool strict_pi, uint64_t* mine, uint64_t* theirs) {
    uint32_t bad = 0u;
    if (w.states) {
        const SampleState s = w.states[i];
        *mine = s.x;
        *theirs = s.y;
    } else {
        bad = sample_state_from_planes(w.boards + (size_t)i * 84, mine, theirs);
    }
    bad |= sample_state_bits(*mine, *theirs);
    for (int a = 0; a < 7; ++a) {
        const float x = w.pis[(size_t)i * 7 + a];
        if (!(strict_pi ? sample_is_prior(x) : sample_in_unit(x))) bad |= SAMPLE_BAD_VALUE;
    }
    if (!sample_in_unit(w.zs[i])) bad |= SAMPLE_BAD_VALUE;
    return bad;
}

// ---- host only --------------------------------------------------------------------------------------------------------------------------
// the sentence a refusal ends with (the entry puts its own name in front); nullptr: no bit set
inline const char* sample_bad_text(uint32_t bits, bool strict_pi) {
    if (bits & SAMPLE_BAD_FEATURE) return "a boards feature that is not 0 or 1, or a cell set in both planes";
    if (bits & SAMPLE_BAD_STATE) return "a state with overlapping stones or bits outside the 7x6 board";
    if (bits & SAMPLE_BAD_VALUE)
        return strict_pi ? "a pi that is NaN or outside [0, 1], or a z that is NaN or outside [-1, 1]" : "a pi or z that is NaN or outside [-1, 1]";
    if (bits & SAMPLE_BAD_PRIOR) return "a prior that is NaN or outside [0, 1]";
    return nullptr;
}

// one workspace, carved: need(bytes) is the offset of the next part, every part padded to 256 bytes; total = the bytes asked for so far
struct Carve {
    size_t total = 0;
    size_t need(size_t bytes) {
        const size_t off = total;
        total += (bytes + 255) / 256 * 256;
        return off;
    }
};

// true where an output array overlaps an input array (a null or empty array overlaps nothing)
struct SampleSpan { const void* p; size_t bytes; };
template <size_t A, size_t B>
inline bool sample_arrays_overlap(const SampleSpan (&in)[A], const SampleSpan (&out)[B]) {
    for (const SampleSpan& a : in)
        for (const SampleSpan& b : out) {
            if (!a.p || !b.p || !a.bytes || !b.bytes) continue;
            const uintptr_t a0 = (uintptr_t)a.p, b0 = (uintptr_t)b.p;
            if (a0 < b0 + b.bytes && b0 < a0 + a.bytes) return true;
        }
    return false;
}

}  // namespace az
