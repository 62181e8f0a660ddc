// az_reanalyse.h -- what az_reanalyse (include/az_reanalyse.h) refuses in a stored position beyond what every sample
// window refuses (az_samples.h), and the host-side rule of the two Coaches: which history entries a learn() iteration re-searches and on which
// game ids.  HIP-free apart from the host/device qualifier (AZR_HD, as az_samples.h has AZV_HD): k_reanalyse_check and the g++ twin of the
// tests (tests/cpp/reanalyse_twin.cpp) compile this text.
//
// A position az_reanalyse searches is one a game of Connect Four can stand in with a move still to make:
//   gravity    no stone above an empty cell: REANALYSE_FLOATING
//   turn       the side to move (`mine`) has as many stones as the other side or one fewer: theirs - mine in {0, 1}; else REANALYSE_COUNTS
//   open       neither side has four in a row and a cell is free (a search of a finished game is the reference's panic,
//              src/async_mcts.rs:85): REANALYSE_DECIDED
// The three are tested on a state that passed sample_state_bits (no overlap, nothing outside the 7 x 6 board); a state that did not carries
// that verdict alone.
#pragma once
#include "az_samples.h"

#if defined(__HIPCC__)
#define AZR_HD __host__ __device__ __forceinline__
#else
#define AZR_HD inline
#endif

namespace az {

constexpr uint32_t REANALYSE_FLOATING = 16u, REANALYSE_COUNTS = 32u, REANALYSE_DECIDED = 64u;      // verdict bits, next to SAMPLE_BAD_*
constexpr int64_t REANALYSE_MAX_POSITIONS = (int64_t)1 << 24;
constexpr int32_t REANALYSE_DEFAULT_CONCURRENT = 8192;

AZR_HD uint32_t reanalyse_popcount(uint64_t x) {
    uint32_t n = 0;
    for (; x; x &= x - 1) ++n;
    return n;
}
// az_game.h's c4_has_four, restated so that this header stands alone (az_tree.hip asserts nothing about it: the GPU tests hold the two together,
// a decided position that slipped through would be the search's own AZ_ERR_TERMINAL_ROOT)
AZR_HD bool reanalyse_has_four(uint64_t b) {
    uint64_t m;
    m = b & (b >> 1); if (m & (m >> 2)) return true;
    m = b & (b >> 7); if (m & (m >> 14)) return true;
    m = b & (b >> 6); if (m & (m >> 12)) return true;
    m = b & (b >> 8); if (m & (m >> 16)) return true;
    return false;
}
// the verdict bits of one position given as (mine, theirs)
AZR_HD uint32_t reanalyse_position_bits(uint64_t mine, uint64_t theirs) {
    if (const uint32_t b = sample_state_bits(mine, theirs)) return b;
    uint32_t bad = 0u;
    const uint64_t occ = mine | theirs;
    for (int c = 0; c < 7; ++c) {
        const uint32_t col = (uint32_t)(occ >> (c * 7)) & 0x3Fu;        // a column without a gap is 2^height - 1
        if (col & (col + 1u)) bad |= REANALYSE_FLOATING;
    }
    const uint32_t nm = reanalyse_popcount(mine), nt = reanalyse_popcount(theirs);
    if (!(nt == nm || nt == nm + 1u)) bad |= REANALYSE_COUNTS;
    if (reanalyse_has_four(mine) || reanalyse_has_four(theirs) || occ == SAMPLE_BOARD) bad |= REANALYSE_DECIDED;
    return bad;
}
// position i of a window given as states [n] or (states == nullptr) boards [n][84]: its verdict bits and its state
AZR_HD uint32_t reanalyse_check(const SampleState* states, const float* boards, int64_t i, uint64_t* mine, uint64_t* theirs) {
    uint32_t bad = 0u;
    if (states) {
        const SampleState s = states[i];
        *mine = s.x;
        *theirs = s.y;
    } else {
        bad = sample_state_from_planes(boards + (size_t)i * 84, mine, theirs);
    }
    return bad ? bad : reanalyse_position_bits(*mine, *theirs);
}

// ---- host only --------------------------------------------------------------------------------------------------------------------------
// the sentence a refusal ends with; nullptr: no bit set
inline const char* reanalyse_bad_text(uint32_t bits) {
    if (const char* why = sample_bad_text(bits & (SAMPLE_BAD_FEATURE | SAMPLE_BAD_STATE), false)) return why;
    if (bits & REANALYSE_FLOATING) return "a stone above an empty cell";
    if (bits & REANALYSE_COUNTS) return "stone counts that no game reaches (theirs - mine must be 0 or 1)";
    if (bits & REANALYSE_DECIDED) return "a position that is already decided or full";
    return nullptr;
}

// ---- the Coaches' rule (Coach.reanalyse_sims; alphazero-rs_amd/coach.py and include/az_host.hpp state it once each, tests/test_reanalyse_cpu.py
// holds the two to this text) --------------------------------------------------------------------------------------------------------------
// In iteration `it`, once the new window is appended and the oldest dropped, the history holds `len` entries; the last one is the window this
// iteration's net just played.  Every OLDER entry h in [0, len - 1) is re-searched, tuple j of it on game id
//     reanalyse_first_game_id(it, h) + j,      with seed + it as the call's seed.
// The ids of one (iteration, entry) pair are a block of 2^32 of their own, far above every self-play id a Coach hands out.
constexpr uint64_t REANALYSE_ID_BASE = 1ull << 62;
inline uint64_t reanalyse_first_game_id(uint64_t iteration, uint64_t history_index) {
    return REANALYSE_ID_BASE + (iteration << 40) + (history_index << 32);
}
inline int reanalyse_entries(int history_len) { return history_len > 1 ? history_len - 1 : 0; }

}  // namespace az
