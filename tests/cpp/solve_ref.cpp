// solve_ref.cpp -- an independent reference for az_solve: a memoised FULL minimax (no pruning, no move ordering, no shortcuts) over
// std::unordered_map, with its own Connect Four / Connect Three rules written on a cell array, not on bitboards.  It shares nothing with
// csrc/az_solve.h.  TEST INFRASTRUCTURE ONLY (tests/solve_twin.py drives it).
//
// Usage: solve_ref <in> <out>      in: as solve_twin's (max_nodes, min_stones and tt_log2 are ignored);  out: int8 move_values [n][7], int8 values [n]
#include <cstdint>
#include <cstdio>
#include <unordered_map>
#include <vector>

namespace {

constexpr int COLS = 7, ROWS = 6;
int K = 4;                                   // stones in a row that win

struct Board {
    int8_t cell[COLS][ROWS];                 // 0 empty, 1 / 2 the stones of player 1 / player 2 (absolute colours: nothing is flipped)
    int height[COLS];
    int mover;                               // 1 or 2
    uint64_t occ[3];                         // occ[p]: the cells of player p as a bit set -- the memo's key only, no rule reads it
};

bool line_through(const Board& b, int c, int r, int who) {
    const int dc[4] = {1, 0, 1, 1}, dr[4] = {0, 1, 1, -1};
    for (int d = 0; d < 4; ++d) {
        int run = 1;
        for (int sgn = -1; sgn <= 1; sgn += 2)
            for (int k = 1; k < K; ++k) {
                const int cc = c + sgn * k * dc[d], rr = r + sgn * k * dr[d];
                if (cc < 0 || cc >= COLS || rr < 0 || rr >= ROWS || b.cell[cc][rr] != who) break;
                ++run;
            }
        if (run >= K) return true;
    }
    return false;
}
bool any_line(const Board& b, int who) {
    for (int c = 0; c < COLS; ++c)
        for (int r = 0; r < ROWS; ++r)
            if (b.cell[c][r] == who && line_through(b, c, r, who)) return true;
    return false;
}
bool full(const Board& b) {
    for (int c = 0; c < COLS; ++c) if (b.height[c] < ROWS) return false;
    return true;
}
struct Key {
    uint64_t a, b;                           // the mover's cells, the other side's cells
    bool operator==(const Key& o) const { return a == o.a && b == o.b; }
};
struct KeyHash {
    size_t operator()(const Key& k) const {
        uint64_t x = k.a * 0x9E3779B97F4A7C15ull ^ (k.b + 0x7F4A7C15ull) * 0xC2B2AE3D27D4EB4Full;
        return (size_t)(x ^ (x >> 29));
    }
};
std::unordered_map<Key, int8_t, KeyHash> memo;

int value_of(Board& b);
// value of dropping a stone into column c for the side to move at b; b is restored
int value_of_move(Board& b, int c) {
    const int who = b.mover, r = b.height[c];
    b.cell[c][r] = (int8_t)who;
    ++b.height[c];
    b.occ[who] |= 1ull << (c * ROWS + r);
    b.mover = 3 - who;
    int v;
    if (line_through(b, c, r, who)) v = 1;
    else if (full(b)) v = 0;
    else v = -value_of(b);
    b.mover = who;
    b.occ[who] &= ~(1ull << (c * ROWS + r));
    --b.height[c];
    b.cell[c][r] = 0;
    return v;
}
// value of b (not finished) for its side to move: the best of ALL its moves
int value_of(Board& b) {
    const Key k{b.occ[b.mover], b.occ[3 - b.mover]};
    auto it = memo.find(k);
    if (it != memo.end()) return it->second;
    int best = -2;
    for (int c = 0; c < COLS; ++c) {
        if (b.height[c] >= ROWS) continue;
        const int v = value_of_move(b, c);
        if (v > best) best = v;
    }
    memo.emplace(k, (int8_t)best);
    return best;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: solve_ref <in> <out>\n"); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hdr[5];
    if (std::fread(hdr, 4, 5, f) != 5) return 2;
    K = hdr[0] == 1 ? 3 : 4;
    memo.reserve((size_t)1 << 22);
    const int n = hdr[1];
    std::vector<uint64_t> st((size_t)n * 2);
    if (n && std::fread(st.data(), 8, st.size(), f) != st.size()) return 2;
    std::fclose(f);
    std::vector<int8_t> mv((size_t)n * 7), values((size_t)n);
    for (int i = 0; i < n; ++i) {
        Board b;
        b.mover = 1;
        b.occ[0] = b.occ[1] = b.occ[2] = 0;
        for (int c = 0; c < COLS; ++c) {
            b.height[c] = 0;
            for (int r = 0; r < ROWS; ++r) {
                const uint64_t bit = 1ull << (c * 7 + r);
                b.cell[c][r] = (st[2 * i] & bit) ? 1 : ((st[2 * i + 1] & bit) ? 2 : 0);
                if (b.cell[c][r]) { b.height[c] = r + 1; b.occ[b.cell[c][r]] |= 1ull << (c * ROWS + r); }
            }
        }
        int8_t* m = &mv[(size_t)i * 7];
        if (any_line(b, 1) || any_line(b, 2) || full(b)) {          // finished: no action, the value as the tree sees it (to the side that moved in)
            for (int c = 0; c < COLS; ++c) m[c] = -128;
            values[i] = (int8_t)(any_line(b, 1) ? -1 : (any_line(b, 2) ? 1 : 0));
            continue;
        }
        int best = -2;
        for (int c = 0; c < COLS; ++c) {
            if (b.height[c] >= ROWS) { m[c] = -128; continue; }
            m[c] = (int8_t)value_of_move(b, c);
            if (m[c] > best) best = m[c];
        }
        values[i] = (int8_t)best;
    }
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    std::fwrite(mv.data(), 1, mv.size(), o);
    std::fwrite(values.data(), 1, values.size(), o);
    std::fclose(o);
    return 0;
}
