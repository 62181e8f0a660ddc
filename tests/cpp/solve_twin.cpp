// solve_twin.cpp -- csrc/az_solve.h compiled for the host: the text the kernels of az_solve.hip compile, so values, node counts and UNKNOWN
// verdicts can be compared item for item (tests/solve_twin.py drives it).  TEST INFRASTRUCTURE ONLY.
// The Game policies below restate the five members of az_game.h the search uses, on the same canonical bitboards; az_game.h itself needs the
// HIP headers.  The GPU tests hold the engine to this program bit for bit, which pins the two statements of the rules to each other.
//
// Usage: solve_twin <in> <out>
//   in : int32 game (0 = Connect Four, 1 = Connect Three), int32 n, uint32 max_nodes, int32 min_stones, int32 tt_log2, then n x {mine, theirs} u64
//   out: int8 move_values [n][7], int8 values [n], uint32 nodes [n][7]
// One table slice serves all items in turn, as a lane's does.
//
// Usage: solve_twin classify <in> <out>      the header's solve_classify / solve_combine alone
//   in : int32 n, int8 move_values [n][7], uint8 action [n]        out: uint8 class [n], int8 combined value [n]
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "az_solve.h"

namespace {

constexpr uint64_t FULL = 0x3Full | (0x3Full << 7) | (0x3Full << 14) | (0x3Full << 21) | (0x3Full << 28) | (0x3Full << 35) | (0x3Full << 42);
constexpr uint64_t BOTTOM = 1ull | (1ull << 7) | (1ull << 14) | (1ull << 21) | (1ull << 28) | (1ull << 35) | (1ull << 42);

template <int K>
bool has_line(uint64_t b) {
    const int dirs[4] = {1, 7, 6, 8};
    for (int d : dirs) {
        uint64_t m = b;
        for (int k = 1; k < K; ++k) m &= b >> (d * k);
        if (m) return true;
    }
    return false;
}

template <int K>
struct HostGame {
    static constexpr int ACTIONS = 7, MAX_PLIES = 42;
    struct State { uint64_t x, y; };
    using Packed = uint64_t;
    static State play(State s, int a) {
        const uint64_t mask = s.x | s.y;
        const uint64_t nb = (mask + (1ull << (a * 7))) & (0x3Full << (a * 7));
        return State{s.y, s.x | nb};
    }
    static uint32_t valid_mask(State s) {
        uint32_t v = 0;
        for (int c = 0; c < 7; ++c) v |= ((s.x | s.y) & (1ull << (c * 7 + 5))) ? 0u : (1u << c);
        return v;
    }
    static uint32_t ended_code(State s) {
        if (has_line<K>(s.x)) return az::SOLVE_E_MINUS1;
        if (has_line<K>(s.y)) return az::SOLVE_E_PLUS1;
        if ((s.x | s.y) == FULL) return az::SOLVE_E_DRAW;
        return az::SOLVE_E_NONE;
    }
    static Packed pack(State s) { return s.x + (s.x | s.y) + BOTTOM; }
    static uint32_t stones(State s) { return (uint32_t)__builtin_popcountll(s.x | s.y); }
};

template <class G>
void run(const std::vector<uint64_t>& st, int n, uint32_t max_nodes, int32_t min_stones, int32_t tt_log2, std::vector<int8_t>& mv,
         std::vector<int8_t>& values, std::vector<uint32_t>& nodes) {
    std::vector<uint64_t> table(tt_log2 ? (size_t)1 << tt_log2 : 1, 0ull);
    uint32_t gen = 0;
    auto* S = new az::SolveSearch<G>();
    for (int i = 0; i < n; ++i) {
        const typename G::State s{st[2 * i], st[2 * i + 1]};
        for (int a = 0; a < G::ACTIONS; ++a) {
            bool fin = S->begin(s, a, max_nodes, min_stones, table.data(), (uint32_t)tt_log2, &gen);
            while (!fin) fin = S->step();
            mv[(size_t)i * 7 + a] = (int8_t)S->result;
            nodes[(size_t)i * 7 + a] = S->nodes;
        }
        const uint32_t ec = G::ended_code(s);
        values[i] = (int8_t)(ec != az::SOLVE_E_NONE ? az::solve_value_of_ecode(ec) : az::solve_combine(&mv[(size_t)i * 7], G::ACTIONS));
    }
    delete S;
}

}  // namespace

int classify_main(const char* in, const char* out) {
    FILE* f = std::fopen(in, "rb");
    if (!f) return 2;
    int32_t n = 0;
    if (std::fread(&n, 4, 1, f) != 1 || n < 0) return 2;
    std::vector<int8_t> mv((size_t)n * 7), val((size_t)n);
    std::vector<uint8_t> act((size_t)n), cls((size_t)n);
    if (n && (std::fread(mv.data(), 1, mv.size(), f) != mv.size() || std::fread(act.data(), 1, act.size(), f) != act.size())) return 2;
    std::fclose(f);
    for (int i = 0; i < n; ++i) {
        cls[i] = (uint8_t)az::solve_classify(&mv[(size_t)i * 7], 7, act[i]);
        val[i] = (int8_t)az::solve_combine(&mv[(size_t)i * 7], 7);
    }
    FILE* o = std::fopen(out, "wb");
    if (!o) return 2;
    std::fwrite(cls.data(), 1, cls.size(), o);
    std::fwrite(val.data(), 1, val.size(), o);
    std::fclose(o);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 4 && std::string(argv[1]) == "classify") return classify_main(argv[2], argv[3]);
    if (argc < 3) { std::fprintf(stderr, "usage: solve_twin <in> <out>\n"); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hdr[5];
    if (std::fread(hdr, 4, 5, f) != 5) return 2;
    const int game = hdr[0], n = hdr[1];
    const uint32_t max_nodes = (uint32_t)hdr[2];
    std::vector<uint64_t> st((size_t)n * 2);
    if (n && std::fread(st.data(), 8, st.size(), f) != st.size()) return 2;
    std::fclose(f);
    std::vector<int8_t> mv((size_t)n * 7), values((size_t)n);
    std::vector<uint32_t> nodes((size_t)n * 7);
    if (game == 1) run<HostGame<3>>(st, n, max_nodes, hdr[3], hdr[4], mv, values, nodes);
    else run<HostGame<4>>(st, n, max_nodes, hdr[3], hdr[4], mv, values, nodes);
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    std::fwrite(mv.data(), 1, mv.size(), o);
    std::fwrite(values.data(), 1, values.size(), o);
    std::fwrite(nodes.data(), 4, nodes.size(), o);
    std::fclose(o);
    return 0;
}
