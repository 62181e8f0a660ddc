// az_solve.hip -- the kernels of az_solve and az_move_quality (csrc/az_solve.h holds the search and its frozen rule).
// Templates over the Game policy of az_game.h.  The one thing restated here and not taken from the policy is what a REACHABLE stacking is
// (solve_state_ok): both games play on the same 7 x 6 board with gravity.
#include "az_solve.h"

#include <algorithm>

#include "az_game.h"

namespace az {
namespace {

constexpr uint32_t SOLVE_WAVE = 64;         // one wave per workgroup: a wave leaves on its own
constexpr uint32_t AUX_BLOCK = 256;

__device__ __forceinline__ bool solve_state_ok(uint64_t mine, uint64_t theirs) {
    if ((mine & theirs) || ((mine | theirs) & ~C4_FULL)) return false;
    const uint64_t mask = mine | theirs;
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 7; ++c) {
        const uint32_t col = (uint32_t)(mask >> (c * 7)) & 0x3Fu;
        ok = ok && ((col & (col + 1u)) == 0u);      // stones stacked from the bottom: 2^h - 1
    }
    return ok;
}

__global__ __launch_bounds__(AUX_BLOCK) void k_solve_validate(const ulonglong2* states, uint32_t n, uint32_t* verdict) {
    const uint32_t i = blockIdx.x * AUX_BLOCK + threadIdx.x;
    if (i >= n) return;
    const ulonglong2 s = states[i];
    if (!solve_state_ok(s.x, s.y)) atomicOr(verdict, SOLVE_BAD_STATE);
}

// The persistent search grid.  Every lane runs ONE loop in which it either takes its next item or advances its search by one child, so no
// lane waits for a neighbour's item.  The lanes of a wave that need an item in the same pass share one atomic on the counter.  A wave
// leaves when every lane of it has been refused an item.
template <class G>
__global__ __launch_bounds__(SOLVE_WAVE) void k_solve(SolveBufs b) {
    const uint32_t lane = blockIdx.x * SOLVE_WAVE + threadIdx.x;
    unsigned long long* tt = b.tt_log2 ? b.tt + ((size_t)lane << b.tt_log2) : nullptr;
    uint32_t gen = b.gens[lane];
    const uint32_t n_items = b.n * (uint32_t)G::ACTIONS;
    SolveSearch<G> S;
    uint32_t item = 0;
    bool busy = false, done = false;
    for (;;) {
        const bool need = !busy && !done;
        const unsigned long long mask = __ballot(need);
        if (mask != 0ull) {
            const int leader = __ffsll((long long)mask) - 1;
            uint32_t base = 0;
            if ((int)threadIdx.x == leader) base = atomicAdd(b.counter, (uint32_t)__popcll(mask));
            base = (uint32_t)__shfl((int)base, leader);
            if (need) {
                item = base + (uint32_t)__popcll(mask & ((1ull << threadIdx.x) - 1ull));
                if (item >= n_items) done = true;
            }
        }
        bool finished = false;
        if (need && !done) {
            const uint32_t i = item / (uint32_t)G::ACTIONS, a = item % (uint32_t)G::ACTIONS;
            if (b.active && !b.active[i]) {
                S.result = SOLVE_ILLEGAL;
                S.nodes = 0;
                finished = true;
            } else {
                finished = S.begin(b.states[i], (int)a, b.max_nodes, b.min_stones, (uint64_t*)tt, b.tt_log2, &gen);
                busy = !finished;
            }
        } else if (busy) {
            finished = S.step();
            busy = !finished;
        }
        if (finished) {
            b.mv[item] = (int8_t)S.result;
            b.nodes[item] = S.nodes;
        }
        if (__all(done ? 1 : 0)) break;
    }
    b.gens[lane] = gen;
}

// values[i]: the combination rule of az_solve.h; a finished position carries the value of its ended_code as the tree sees it
template <class G>
__global__ __launch_bounds__(AUX_BLOCK) void k_solve_values(SolveBufs b) {
    const uint32_t i = blockIdx.x * AUX_BLOCK + threadIdx.x;
    if (i >= b.n) return;
    int v;
    if (b.active && !b.active[i]) v = SOLVE_UNKNOWN;
    else {
        const uint32_t ec = G::ended_code(b.states[i]);
        v = ec != E_NONE ? solve_value_of_ecode(ec) : solve_combine(b.mv + (size_t)i * G::ACTIONS, G::ACTIONS);
    }
    b.values[i] = (int8_t)v;
}

// one lane per game: the position before every ply that was played, or a verdict
template <class G>
__global__ __launch_bounds__(AUX_BLOCK) void k_mq_replay(MoveQualityBufs b) {
    const uint32_t g = blockIdx.x * AUX_BLOCK + threadIdx.x;
    if (g >= b.n) return;
    typename G::State s = b.start ? b.start[g] : G::init();
    uint32_t bad = 0;
    if (!solve_state_ok(s.x, s.y)) { bad |= SOLVE_BAD_STATE; s = G::init(); }
    const int32_t len = b.game_len[g];
    if (len < 0 || len > G::MAX_PLIES) bad |= SOLVE_BAD_RECORD;
    for (int p = 0; p < G::MAX_PLIES; ++p) {
        const size_t slot = (size_t)g * G::MAX_PLIES + p;
        bool on = p < len && !bad;
        uint32_t a = 0;
        if (on) {
            a = b.moves[slot];
            if (G::ended_code(s) != E_NONE || a >= (uint32_t)G::ACTIONS || !((G::valid_mask(s) >> a) & 1u)) {
                bad |= SOLVE_BAD_RECORD;
                on = false;
            }
        }
        b.states[slot] = on ? s : G::init();
        b.active[slot] = on ? 1 : 0;
        if (on) s = G::play(s, (int)a);
    }
    if (bad) atomicOr(b.verdict, bad);
}

template <class G>
__global__ __launch_bounds__(AUX_BLOCK) void k_mq_classify(MoveQualityBufs b) {
    const size_t slot = (size_t)blockIdx.x * AUX_BLOCK + threadIdx.x;
    if (slot >= (size_t)b.n * G::MAX_PLIES) return;
    int cls = MQ_SKIPPED, val = SOLVE_UNKNOWN;
    if (b.active[slot] && (int32_t)G::stones(b.states[slot]) >= b.min_stones) {
        const int8_t* mv = b.mv + slot * G::ACTIONS;
        cls = solve_classify(mv, G::ACTIONS, (int)b.moves[slot]);
        val = solve_combine(mv, G::ACTIONS);
    }
    b.ply_class[slot] = (uint8_t)cls;
    b.ply_value[slot] = (int8_t)val;
}

inline unsigned aux_blocks(size_t items) { return (unsigned)((items + AUX_BLOCK - 1) / AUX_BLOCK); }

}  // namespace

int solve_device_lanes(int game) {
    int dev = 0, cus = 0, per_cu = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
    const hipError_t st = game == 1 ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_solve<ConnectThree>, (int)SOLVE_WAVE, 0)
                                    : hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_solve<ConnectFour>, (int)SOLVE_WAVE, 0);
    if (st != hipSuccess || cus <= 0 || per_cu <= 0) return 0;
    return cus * std::min(per_cu, 32) * (int)SOLVE_WAVE;
}
void launch_solve_validate(const ulonglong2* states, uint32_t n, uint32_t* verdict, hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_solve_validate, dim3(aux_blocks(n)), dim3(AUX_BLOCK), 0, s, states, n, verdict);
}
void launch_solve(int game, const SolveBufs& b, uint32_t lanes, hipStream_t s) {
    if (b.n == 0) return;
    const dim3 grid(lanes / SOLVE_WAVE), block(SOLVE_WAVE);
    if (game == 1) hipLaunchKernelGGL(k_solve<ConnectThree>, grid, block, 0, s, b);
    else hipLaunchKernelGGL(k_solve<ConnectFour>, grid, block, 0, s, b);
    if (game == 1) hipLaunchKernelGGL(k_solve_values<ConnectThree>, dim3(aux_blocks(b.n)), dim3(AUX_BLOCK), 0, s, b);
    else hipLaunchKernelGGL(k_solve_values<ConnectFour>, dim3(aux_blocks(b.n)), dim3(AUX_BLOCK), 0, s, b);
}
void launch_move_quality_replay(int game, const MoveQualityBufs& b, hipStream_t s) {
    if (b.n == 0) return;
    if (game == 1) hipLaunchKernelGGL(k_mq_replay<ConnectThree>, dim3(aux_blocks(b.n)), dim3(AUX_BLOCK), 0, s, b);
    else hipLaunchKernelGGL(k_mq_replay<ConnectFour>, dim3(aux_blocks(b.n)), dim3(AUX_BLOCK), 0, s, b);
}
void launch_move_quality_classify(int game, const MoveQualityBufs& b, hipStream_t s) {
    if (b.n == 0) return;
    const unsigned nb = aux_blocks((size_t)b.n * ConnectFour::MAX_PLIES);
    if (game == 1) hipLaunchKernelGGL(k_mq_classify<ConnectThree>, dim3(nb), dim3(AUX_BLOCK), 0, s, b);
    else hipLaunchKernelGGL(k_mq_classify<ConnectFour>, dim3(nb), dim3(AUX_BLOCK), 0, s, b);
}

}  // namespace az
