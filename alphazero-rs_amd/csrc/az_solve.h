// az_solve.h -- the exact endgame search of az_solve / az_move_quality (include/az_engine.h).
//
// Host and device compile this same text (the kernels in az_solve.hip, the g++ twin in tests/cpp/solve_twin.cpp), so a value, a node
// count and an UNKNOWN verdict are the same on both, item for item.  The header includes nothing of the engine: it is a template over a
// Game policy G (az_game.h) of which it uses State (two words {x = the mover's stones, y = the other side's}), play, valid_mask,
// ended_code, pack and stones, and no rule is named here -- ConnectFour and ConnectThree both instantiate it.
//
// An ITEM is one (position s, root action a) pair; its result is the outcome for the side to move at s after it plays a, an exact value
// in {-1, 0, +1}, or AZ_SOLVE_ILLEGAL / AZ_SOLVE_UNKNOWN.
//
// THE SEARCH RULE (frozen: node counts and the UNKNOWN set are part of the result)
//   item      ended_code(s) != none, or a not in valid_mask(s)        -> ILLEGAL, 0 nodes
//             stones(s) < min_stones                                  -> UNKNOWN, 0 nodes
//             c = play(s, a) ends the game                            -> +1 / 0 / -1 from ended_code(c), 0 nodes
//             otherwise                                               -> -node(c, -1, +1)
//   node(s, alpha, beta), negamax, fail-soft, on an explicit stack of at most MAX_PLIES frames:
//     0. budget: a node is COUNTED when it is entered.  Entering a node when `nodes == max_nodes` ends the item: UNKNOWN, nodes = max_nodes
//     1. a legal move whose child has ended_code E_PLUS1 (the mover wins at once)        -> return +1
//     2. T = the legal moves a with ended_code(play({s.y, s.x}, a)) == E_PLUS1: the squares where the opponent would win at once.
//        |T| >= 2 -> return -1;  |T| == 1 -> the node's move list is T;  |T| == 0 -> it is valid_mask(s)
//     3. table probe (tt_log2 > 0): an entry of this item for pack(s) with bounds [lo, hi]:
//        lo == hi or lo >= beta -> return lo;  hi <= alpha -> return hi.  The window is not narrowed otherwise
//     4. the move list in the order 3, 2, 4, 1, 5, 0, 6; for each move c = play(s, a): a child that ends the game is a draw (value 0: a win
//        was excluded in 1) and is not a node; any other child is node(c, -beta, -alpha) negated.  best = max, alpha = max(alpha, best),
//        stop when alpha >= beta
//     5. table store (always replace): best <= the alpha the node was entered with -> [-1, best];  best >= beta -> [best, +1];
//        else [best, best].  Nodes answered in 1 - 3 are not stored.  return best
//   Everything is a function of (s, a, max_nodes, min_stones, tt_log2, G): an item never sees a table entry of another item.
//
// TABLE ENTRY, one 64-bit word (one load or store is consistent):
//   bits 0-48 pack(s) (49 bits: both games' keys)   | 49-50 lo + 1 | 51-52 hi + 1 | 53-63 generation (1 .. 2047; 0 = never written)
//   The slice of 1 << tt_log2 entries belongs to the LANE that runs the item (the host twin: to the caller); its generation counter moves on
//   by one per item that enters a node, and an entry of another generation is an empty slot.  When the counter would pass 2047 the lane
//   zeroes its slice and starts again at 1.  slot = (mix(pack) >> 32) & (size - 1).
//
// The search is a state machine (solve_begin, then solve_step until it returns true) so that a kernel can interleave "take the next item"
// with "advance the search by one child" in ONE loop: the lanes of a wave then never wait for each other's items.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define AZS_HD __host__ __device__ __forceinline__
#else
#define AZS_HD inline
#endif

namespace az {

constexpr int SOLVE_ILLEGAL = -128, SOLVE_UNKNOWN = 127;            // == AZ_SOLVE_ILLEGAL / AZ_SOLVE_UNKNOWN
constexpr uint32_t SOLVE_E_NONE = 0, SOLVE_E_PLUS1 = 1, SOLVE_E_MINUS1 = 2, SOLVE_E_DRAW = 3;      // == E_* of az_common.h
constexpr int SOLVE_KEY_BITS = 49;
constexpr uint64_t SOLVE_KEY_MASK = (1ull << SOLVE_KEY_BITS) - 1ull;
constexpr uint32_t SOLVE_GEN_MAX = 2047;
// classes of az_move_quality == AZ_MQ_*
constexpr int MQ_SKIPPED = 0, MQ_KEPT = 1, MQ_WIN_TO_DRAW = 2, MQ_WIN_TO_LOSS = 3, MQ_DRAW_TO_LOSS = 4, MQ_UNKNOWN = 5;

AZS_HD uint64_t solve_mix(uint64_t x) {                             // == mix64 of az_common.h
    x += 0x9E3779B97F4A7C15ull;
    uint64_t z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
AZS_HD int solve_value_of_ecode(uint32_t ec) { return ec == SOLVE_E_PLUS1 ? 1 : (ec == SOLVE_E_MINUS1 ? -1 : 0); }
// centre-first: the i-th move tried is (SOLVE_ORDER >> 4 i) & 15
constexpr uint32_t SOLVE_ORDER = 0x6051423u;
AZS_HD int solve_next_move(uint32_t todo) {
    int a = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 6; i >= 0; --i) {
        const int m = (int)((SOLVE_ORDER >> (4 * i)) & 15u);
        if ((todo >> m) & 1u) a = m;
    }
    return a;
}

template <class G>
struct SolveFrame {
    typename G::State s;
    int8_t alpha0, alpha, beta, best;
    uint8_t todo;                      // moves of the node's list not tried yet
};

// One item's search.  `tt` is the lane's slice (nullptr when tt_log2 == 0), `gen` its generation counter, kept by the caller across items.
template <class G>
struct SolveSearch {
    SolveFrame<G> f[G::MAX_PLIES];
    int sp;                            // top frame, -1 = none
    int ret;                           // value a finished child handed up (from the child's side to move)
    bool have_ret;
    uint32_t nodes, max_nodes;
    uint64_t* tt;
    uint32_t tt_mask, gen;
    int result;                        // the item's result once solve_step returned true (or solve_begin did)

    AZS_HD static typename G::State swapped(typename G::State s) {
        typename G::State o = s;
        o.x = s.y;
        o.y = s.x;
        return o;
    }
    AZS_HD uint32_t slot_of(uint64_t key) const { return (uint32_t)(solve_mix(key) >> 32) & tt_mask; }

    // rule steps 1 - 3 for a node that has just been counted: true = answered (*value), false = a frame was pushed
    AZS_HD bool enter(typename G::State s, int alpha, int beta, int* value) {
        const uint32_t vm = G::valid_mask(s);
        const typename G::State o = swapped(s);
        uint32_t threats = 0;
        bool win = false;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int a = 0; a < G::ACTIONS; ++a) {
            if (!((vm >> a) & 1u)) continue;
            if (G::ended_code(G::play(s, a)) == SOLVE_E_PLUS1) win = true;
            if (G::ended_code(G::play(o, a)) == SOLVE_E_PLUS1) threats |= 1u << a;
        }
        if (win) { *value = 1; return true; }
        if (threats & (threats - 1u)) { *value = -1; return true; }
        if (tt) {
            const uint64_t key = (uint64_t)G::pack(s);
            const uint64_t e = tt[slot_of(key)];
            if ((e & SOLVE_KEY_MASK) == key && (uint32_t)(e >> 53) == gen) {
                const int lo = (int)((e >> 49) & 3u) - 1, hi = (int)((e >> 51) & 3u) - 1;
                if (lo == hi || lo >= beta) { *value = lo; return true; }
                if (hi <= alpha) { *value = hi; return true; }
            }
        }
        SolveFrame<G>& t = f[++sp];
        t.s = s;
        t.alpha0 = (int8_t)alpha;
        t.alpha = (int8_t)alpha;
        t.beta = (int8_t)beta;
        t.best = -1;
        t.todo = (uint8_t)(threats ? threats : vm);
        return false;
    }

    // true = the item is decided at once (result, nodes are final)
    AZS_HD bool begin(typename G::State s, int a, uint32_t max_nodes_, int32_t min_stones, uint64_t* tt_, uint32_t tt_log2, uint32_t* gen_io) {
        sp = -1;
        have_ret = false;
        ret = 0;
        nodes = 0;
        max_nodes = max_nodes_;
        tt = tt_log2 ? tt_ : nullptr;
        tt_mask = tt_log2 ? (1u << tt_log2) - 1u : 0u;
        gen = *gen_io;
        if (G::ended_code(s) != SOLVE_E_NONE || !((G::valid_mask(s) >> a) & 1u)) { result = SOLVE_ILLEGAL; return true; }
        if ((int32_t)G::stones(s) < min_stones) { result = SOLVE_UNKNOWN; return true; }
        const typename G::State c = G::play(s, a);
        const uint32_t ec = G::ended_code(c);
        if (ec != SOLVE_E_NONE) { result = solve_value_of_ecode(ec); return true; }
        if (tt) {                              // a fresh generation for this item's entries
            if (gen >= SOLVE_GEN_MAX) {
                for (uint32_t i = 0; i <= tt_mask; ++i) tt[i] = 0ull;
                gen = 0;
            }
            *gen_io = ++gen;
        }
        nodes = 1;                             // max_nodes >= 1
        int v;
        if (enter(c, -1, 1, &v)) { result = -v; return true; }
        return false;
    }

    // advances the search by at most one child; true = finished
    AZS_HD bool step() {
        SolveFrame<G>& t = f[sp];
        if (have_ret) {
            have_ret = false;
            const int v = -ret;
            if (v > t.best) t.best = (int8_t)v;
            if (v > t.alpha) t.alpha = (int8_t)v;
            if (t.alpha >= t.beta) t.todo = 0;
        }
        if (t.todo == 0) {                     // the node is done: store, hand its value up
            const int best = t.best;
            if (tt) {
                const int lo = best <= t.alpha0 ? -1 : best, hi = best <= t.alpha0 ? best : (best >= t.beta ? 1 : best);
                const uint64_t key = (uint64_t)G::pack(t.s);
                tt[slot_of(key)] = (key & SOLVE_KEY_MASK) | ((uint64_t)(lo + 1) << 49) | ((uint64_t)(hi + 1) << 51) | ((uint64_t)gen << 53);
            }
            --sp;
            if (sp < 0) { result = -best; return true; }
            ret = best;
            have_ret = true;
            return false;
        }
        const int a = solve_next_move(t.todo);
        t.todo = (uint8_t)(t.todo & ~(1u << a));
        const typename G::State c = G::play(t.s, a);
        if (G::ended_code(c) != SOLVE_E_NONE) {        // the board is full: a draw (a win was excluded when the node was entered)
            ret = 0;
            have_ret = true;
            return false;
        }
        if (nodes == max_nodes) { result = SOLVE_UNKNOWN; return true; }
        ++nodes;
        int v;
        if (enter(c, -t.beta, -t.alpha, &v)) {
            ret = v;
            have_ret = true;
        }
        return false;
    }
};

// values[i] of az_solve from the seven move values of a position that is not finished: +1 if any action is +1, else UNKNOWN if any legal
// action is UNKNOWN, else the maximum over the legal actions
AZS_HD int solve_combine(const int8_t* mv, int actions) {
    int best = -2;
    bool unknown = false;
    for (int a = 0; a < actions; ++a) {
        const int v = mv[a];
        if (v == SOLVE_ILLEGAL) continue;
        if (v == SOLVE_UNKNOWN) { unknown = true; continue; }
        if (v > best) best = v;
    }
    if (best == 1) return 1;
    if (unknown || best == -2) return SOLVE_UNKNOWN;
    return best;
}

// class of the move `a` played at a position with move values mv (az_move_quality): a move of value +1 is KEPT whatever its siblings are
AZS_HD int solve_classify(const int8_t* mv, int actions, int a) {
    const int pv = mv[a];
    if (pv == 1) return MQ_KEPT;
    const int V = solve_combine(mv, actions);
    if (V == SOLVE_UNKNOWN || pv == SOLVE_UNKNOWN) return MQ_UNKNOWN;
    if (pv == V) return MQ_KEPT;
    if (V == 1) return pv == 0 ? MQ_WIN_TO_DRAW : MQ_WIN_TO_LOSS;
    return MQ_DRAW_TO_LOSS;
}

}  // namespace az

// ---- the kernels' side (az_solve.hip); not seen by a host-only build -----------------------------------------------------------------------
#if defined(__HIPCC__)
namespace az {

constexpr uint32_t SOLVE_BAD_STATE = 1u, SOLVE_BAD_RECORD = 2u;        // verdict bits of the validating passes

struct SolveBufs {
    const ulonglong2* states;       // [n] canonical {mine, theirs}
    const uint8_t* active;          // [n] or nullptr: 0 = not a position (every action ILLEGAL, 0 nodes)
    uint32_t n;
    uint32_t max_nodes;
    int32_t min_stones;
    uint32_t tt_log2;
    unsigned long long* tt;         // [lanes << tt_log2]
    uint32_t* gens;                 // [lanes] generation counter of each lane's slice, kept across calls
    uint32_t* counter;              // the next item
    int8_t* mv;                     // [n][7]
    uint32_t* nodes;                // [n][7]
    int8_t* values;                 // [n]
};

struct MoveQualityBufs {
    const ulonglong2* start;        // [n] or nullptr = the initial board
    const int32_t* game_len;        // [n]
    const uint8_t* moves;           // [n][MAX_PLIES]
    uint32_t n;
    int32_t min_stones;
    ulonglong2* states;             // [n][MAX_PLIES] the position before ply p
    uint8_t* active;                // [n][MAX_PLIES] 1 = ply p was played
    uint32_t* verdict;
    const int8_t* mv;               // [n][MAX_PLIES][7] the solver's output for `states`
    uint8_t* ply_class;             // [n][MAX_PLIES]
    int8_t* ply_value;              // [n][MAX_PLIES]
};

int solve_device_lanes(int game);                                       // CUs x resident waves x 64 of the search kernel on the current device
void launch_solve_validate(const ulonglong2* states, uint32_t n, uint32_t* verdict, hipStream_t s);
void launch_solve(int game, const SolveBufs& b, uint32_t lanes, hipStream_t s);
void launch_move_quality_replay(int game, const MoveQualityBufs& b, hipStream_t s);
void launch_move_quality_classify(int game, const MoveQualityBufs& b, hipStream_t s);

}  // namespace az
#endif
