// az_opening.h -- paired arena openings ("arena_opening_plies" / az_arena_set_opening_book, include/az_engine.h):
// the position arena game g and its seat-swapped twin g + total/2 start from.  HIP-free apart from the host/device qualifier (AZO_HD, as
// az_playout.h has AZP_HD): the arena's opening kernel (az_tree.hip), the engine's host code and the g++ twin of the tests
// (tests/cpp/opening_twin.cpp) compile this text.  Integer-only, templated on the Game policy of az_game.h: it uses G::State (16 bytes,
// .x = the mover's stones, .y = the other side's), G::ACTIONS, G::valid_mask, G::play and G::ended_code, nothing else.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#define AZO_HD __host__ __device__ __forceinline__
#else
#define AZO_HD inline
#endif

namespace az {

constexpr uint64_t RNG_OPENING = 7;           // the purpose word of the opening draws (az_common.h and az_playout.h: 1 .. 6 are taken)
constexpr int OPENING_MAX_PLIES = 12;         // "arena_opening_plies": 0 (off) or an even value up to this
constexpr int OPENING_MAX_BOOK = 65536;       // entries of an opening book
constexpr uint32_t OPENING_E_NONE = 0, OPENING_E_PLUS1 = 1;    // E_NONE / E_PLUS1 of az_common.h, restated so that this header stands alone

AZO_HD uint64_t opening_mix64(uint64_t x) {   // mix64 of az_common.h
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
// rng_choose(rng_draw(seed, pair, j, RNG_OPENING), k) of az_common.h
AZO_HD uint32_t opening_choose(uint64_t seed, uint64_t pair, uint64_t j, uint32_t k) {
    const uint64_t r = opening_mix64(opening_mix64(opening_mix64(opening_mix64(seed) ^ pair) ^ j) ^ RNG_OPENING);
    return (uint32_t)(((r >> 32) * (uint64_t)k) >> 32);
}

// C1 of canonical state s: bit a set <=> a is legal and the game goes on behind it
template <class G>
AZO_HD uint32_t opening_c1(typename G::State s) {
    const uint32_t vm = G::valid_mask(s);
    uint32_t c = 0;
    for (int a = 0; a < G::ACTIONS; ++a)
        if (((vm >> a) & 1u) && G::ended_code(G::play(s, a)) == OPENING_E_NONE) c |= 1u << a;
    return c;
}
// the mover of canonical state s wins with one move (ended_code of the successor is E_PLUS1: the player who moved in has won)
template <class G>
AZO_HD bool opening_win_in_one(typename G::State s) {
    const uint32_t vm = G::valid_mask(s);
    for (int b = 0; b < G::ACTIONS; ++b)
        if (((vm >> b) & 1u) && G::ended_code(G::play(s, b)) == OPENING_E_PLUS1) return true;
    return false;
}
// C2: those of C1 after which the next mover has no immediately winning reply -- the QUIET plies
template <class G>
AZO_HD uint32_t opening_c2(typename G::State s, uint32_t c1) {
    uint32_t c = 0;
    for (int a = 0; a < G::ACTIONS; ++a)
        if (((c1 >> a) & 1u) && !opening_win_in_one<G>(G::play(s, a))) c |= 1u << a;
    return c;
}

// The opening of pair `pair` with n plies (n even, at most OPENING_MAX_PLIES) grown from `base` (canonical, first seat to move).  Ply j picks
// C[opening_choose(seed, pair, j, |C|)] of the ascending candidates C = C2, or C1 where no ply is quiet, and stops where C is empty.  The
// opening used is the longest EVEN prefix of what was played (an odd last ply is dropped), so the first seat is to move again and *out is
// {first seat's stones, second seat's stones}: a start_board.  Returns the plies used and writes them to moves[0 .. len); *fallbacks
// (may be null) counts the used plies that were drawn from C1 because C2 was empty.
template <class G>
AZO_HD int opening_grow(typename G::State base, uint64_t seed, uint64_t pair, int n, typename G::State* out, uint8_t* moves, int* fallbacks = nullptr) {
    typename G::State s = base, even = base;
    int len = 0, played = 0, fb = 0, fb_even = 0;
    for (int j = 0; j < n; ++j, ++played) {
        const uint32_t c1 = opening_c1<G>(s);
        const uint32_t c2 = opening_c2<G>(s, c1);
        const uint32_t c = c2 ? c2 : c1;
        if (!c) break;
        if (!c2) ++fb;
        uint32_t k = opening_choose(seed, pair, (uint64_t)j, (uint32_t)__builtin_popcount(c));
        int a = 0;
        for (;; ++a)
            if ((c >> a) & 1u) { if (k == 0u) break; --k; }
        moves[j] = (uint8_t)a;
        s = G::play(s, a);
        if (j & 1) { even = s; len = j + 1; fb_even = fb; }
    }
    if (played > len) moves[len] = 0;             // the dropped odd ply leaves no trace
    *out = even;
    if (fallbacks) *fallbacks = fb_even;
    return len;
}

// Base position of pair p: book[p % nb] while a book is set, else the call's start position.
AZO_HD uint64_t opening_book_index(uint64_t pair, uint32_t nb) { return pair % nb; }

}  // namespace az
