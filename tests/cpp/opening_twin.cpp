// opening_twin.cpp -- the g++ build of csrc/az_opening.h (paired arena openings: "arena_opening_plies" / az_arena_set_opening_book,
// include/az_engine.h).  TEST INFRASTRUCTURE ONLY.
//
// The header is templated on a Game policy; the engine instantiates it with the device policies of csrc/az_game.h, this twin with a policy
// made of the ORACLE's rules (oracle/az_oracle_games.hpp: CBits<4> = Connect Four, CBits<3> = Connect Three), so the text the kernel
// compiles is run here over an independent statement of the games.  Built by the tests with g++ -O2 into a shared library driven through
// ctypes (tests/opening_twin.py).
#include "az_oracle_games.hpp"
#include "az_opening.h"

namespace {

using namespace azo;

template <int WIN>
struct OracleGame {
    struct State { uint64_t x, y; };            // canonical: x = the mover's stones
    static constexpr int ACTIONS = C4_W;
    static uint32_t valid_mask(State s) {
        const std::vector<uint8_t> v = CBits<WIN>{s.x, s.y}.get_valid_moves(1);
        uint32_t m = 0;
        for (int c = 0; c < ACTIONS; ++c) m |= v[c] ? (1u << c) : 0u;
        return m;
    }
    static State play(State s, int a) {
        const auto nx = CBits<WIN>{s.x, s.y}.get_next_state(1, (uint8_t)a);
        const CBits<WIN> c = nx.first.get_canonical_form(nx.second);
        return State{c.p1, c.m1};
    }
    // e = -get_game_ended(1) of the canonical state, as the engine's ecode: 0 none, 1 = +1 (the player who moved in has won), 2 = -1, 3 draw
    static uint32_t ended_code(State s) {
        const float r = CBits<WIN>{s.x, s.y}.get_game_ended(1);
        return r == 0.0f ? 0u : (r == -1.0f ? 1u : (r == 1.0f ? 2u : 3u));
    }
};

template <class G>
void grow_all(uint64_t seed, int64_t items, const uint64_t* pairs, const uint64_t* bases, int n, uint64_t* boards, int32_t* len, uint8_t* moves,
              int32_t* fallbacks) {
    for (int64_t i = 0; i < items; ++i) {
        typename G::State out;
        uint8_t mv[az::OPENING_MAX_PLIES] = {0};
        int fb = 0;
        len[i] = az::opening_grow<G>(typename G::State{bases[2 * i], bases[2 * i + 1]}, seed, pairs[i], n, &out, mv, &fb);
        boards[2 * i] = out.x;
        boards[2 * i + 1] = out.y;
        std::memcpy(moves + i * az::OPENING_MAX_PLIES, mv, sizeof mv);
        if (fallbacks) fallbacks[i] = fb;
    }
}

}  // namespace

extern "C" {

int32_t twin_opening_rng_word() { return (int32_t)az::RNG_OPENING; }
int32_t twin_opening_max_plies() { return az::OPENING_MAX_PLIES; }

// item i: the opening of pair pairs[i] with n plies grown from bases[i] under game 0 (Connect Four) or 1 (Connect Three):
// boards [items,2], len [items], moves [items,12] (zero behind len), fallbacks [items] (may be null)
int32_t twin_opening_grow(int32_t game, uint64_t seed, int64_t items, const uint64_t* pairs, const uint64_t* bases, int32_t n, uint64_t* boards,
                          int32_t* len, uint8_t* moves, int32_t* fallbacks) {
    if (n < 0 || n > az::OPENING_MAX_PLIES || (n & 1)) return -1;
    if (game == 0) grow_all<OracleGame<4>>(seed, items, pairs, bases, n, boards, len, moves, fallbacks);
    else if (game == 1) grow_all<OracleGame<3>>(seed, items, pairs, bases, n, boards, len, moves, fallbacks);
    else return -1;
    return 0;
}

}  // extern "C"
