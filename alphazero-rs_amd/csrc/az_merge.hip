// az_merge.hip -- the kernels of az_samples_merge (position averaging; csrc/az_merge.h).
// Templates over the Game policy of az_game.h, as the tree kernels are: they use G::State, G::pack, G::canonical and G::feature.  The one
// thing that is not taken from the policy is the inverse of G::feature (a state from its two feature planes), which the window check of
// az_samples.h holds; both games play on the same 7 x 6 board with the same planes (connect_four_game.rs:219-237), as k_canonicalise of
// az_engine.hip relies on too.
#include "az_merge.h"

#include <algorithm>

#include "az_game.h"

namespace az {

static_assert(SAMPLE_BOARD == C4_FULL && ConnectFour::ACTIONS == 7 && ConnectFour::FEATURES == 84, "az_samples.h restates az_game.h's board, actions and feature cells");

namespace {

constexpr uint32_t MERGE_BLOCK = 256;
constexpr uint32_t ACC_SLOTS = 512;             // LDS table of the accumulate pass: emptied when over a quarter full, so never over three quarters
constexpr uint32_t ACC_EMPTY = 0xFFFFFFFFu;     // no rank (ranks stay below 2^24)

// ---- keys: validate, canonicalise, insert ---------------------------------------------------------------------------------------------
template <class G>
__global__ __launch_bounds__(MERGE_BLOCK) void k_merge_keys(MergeBufs b, int canonical) {
    const uint32_t i = blockIdx.x * MERGE_BLOCK + threadIdx.x;
    if (i >= b.n) return;
    uint64_t mine, theirs;
    const uint32_t bad = sample_check(b.in, i, false, &mine, &theirs);
    if (bad) {                                   // the call is refused: nothing behind this pass runs
        atomicOr(&b.hdr[0], bad);
        return;
    }
    typename G::State s = make_ulonglong2(mine, theirs);
    uint32_t mirrored = 0;
    if (canonical) s = G::canonical(s, &mirrored);
    const unsigned long long key = (unsigned long long)G::pack(s);         // never 0
    uint32_t pos = (uint32_t)(mix64(key) >> 24) & b.tmask;
    for (;;) {                                   // the table is at most half full: an empty slot or the key itself comes up
        unsigned long long cur = b.tkey[pos];
        if (cur == 0ull) cur = atomicCAS(&b.tkey[pos], 0ull, key);
        if (cur == 0ull || cur == key) break;
        pos = (pos + 1u) & b.tmask;
    }
    // The slot's lowest input index.  n copies of one position would be n atomics on one address, which the memory side serves one after
    // the other: where every live lane of the wave sits on one slot only the first (the lowest index) goes on, and nobody sends an index that
    // is not below what the slot already holds (the value only falls, so an old reading can cost an atomic, never lose one).
    const unsigned long long live = __ballot(1);
    const int leader = __ffsll((long long)live) - 1;
    const bool one_slot = __ballot(pos == (uint32_t)__shfl((int)pos, leader)) == live;
    if ((!one_slot || (int)(threadIdx.x & 63u) == leader) && __hip_atomic_load(&b.tmin[pos], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > i)
        atomicMin(&b.tmin[pos], i);
    b.slot[i] = pos | (mirrored ? MERGE_MIRRORED : 0u);
    b.cst[i] = s;
}

// ---- scan: output rank = number of first occurrences before this one ------------------------------------------------------------------
__device__ __forceinline__ bool merge_is_first(const MergeBufs& b, uint32_t i, uint32_t* pos) {
    if (i >= b.n) return false;
    *pos = b.slot[i] & ~MERGE_MIRRORED;
    return b.tmin[*pos] == i;
}
__global__ __launch_bounds__(MERGE_BLOCK) void k_merge_scan_count(MergeBufs b) {
    uint32_t pos = 0;
    const int c = __syncthreads_count(merge_is_first(b, blockIdx.x * MERGE_BLOCK + threadIdx.x, &pos) ? 1 : 0);
    if (threadIdx.x == 0) b.bsum[blockIdx.x] = (uint32_t)c;
}
// one workgroup of 1024: bsum[0 .. nb) becomes its exclusive scan, hdr[1] the total m
__global__ __launch_bounds__(1024) void k_merge_scan_blocks(MergeBufs b, uint32_t nb) {
    __shared__ uint32_t s_w[16];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < nb; base += 1024u) {
        const uint32_t idx = base + tid;
        const uint32_t v = idx < nb ? b.bsum[idx] : 0u;
        uint32_t x = v;
        for (uint32_t off = 1; off < 64u; off <<= 1) {
            const uint32_t y = __shfl_up(x, off);
            if (lane >= off) x += y;
        }
        if (lane == 63u) s_w[wave] = x;
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (uint32_t w = 0; w < 16u; ++w) {
            const uint32_t t = s_w[w];
            if (w < wave) before += t;
            total += t;
        }
        if (idx < nb) b.bsum[idx] = carry + before + x - v;
        carry += total;
        __syncthreads();
    }
    if (tid == 0) b.hdr[1] = carry;
}
__global__ __launch_bounds__(MERGE_BLOCK) void k_merge_scan_rank(MergeBufs b) {
    __shared__ uint32_t s_w[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t i = blockIdx.x * MERGE_BLOCK + tid;
    uint32_t pos = 0;
    const bool first = merge_is_first(b, i, &pos);
    const unsigned long long bal = __ballot(first);
    if (lane == 0) s_w[wave] = (uint32_t)__popcll(bal);
    __syncthreads();
    if (!first) return;
    uint32_t rank = b.bsum[blockIdx.x] + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
    for (uint32_t w = 0; w < wave; ++w) rank += s_w[w];
    b.trank[pos] = rank;
    b.first[rank] = i;
}

// ---- accumulate: eight fixed-point values and a count per tuple, combined in the wave and in LDS before they reach memory ---------------
// A workgroup keeps ONE LDS table over all its rounds of 256 tuples and empties it into memory only when it is more than a quarter full
// (so a round's 256 tuples always find room: at most 128 + 256 of 512 slots) and at the end: a group that every round hits -- the empty
// board, the first openings -- costs a workgroup nine global atomics per flush, not nine per round.  Atomics on one address are served
// one after the other by the memory side.
__global__ __launch_bounds__(MERGE_BLOCK) void k_merge_accumulate(MergeBufs b) {
    __shared__ uint32_t s_key[ACC_SLOTS];
    __shared__ unsigned long long s_sum[ACC_SLOTS][9];        // [8] = the count
    __shared__ uint32_t s_used;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t rounds = (b.n + MERGE_BLOCK - 1u) / MERGE_BLOCK;
    auto flush = [&]() {                         // every slot to memory and back to empty; the caller puts barriers around it
        for (uint32_t k = tid; k < ACC_SLOTS; k += MERGE_BLOCK) {
            const uint32_t key = s_key[k];
            if (key == ACC_EMPTY) continue;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if (s_sum[k][j]) atomicAdd(&b.sums[(size_t)key * 8 + j], s_sum[k][j]);
                s_sum[k][j] = 0ull;
            }
            atomicAdd(&b.cnt[key], (uint32_t)s_sum[k][8]);
            s_sum[k][8] = 0ull;
            s_key[k] = ACC_EMPTY;
        }
    };
    for (uint32_t k = tid; k < ACC_SLOTS; k += MERGE_BLOCK) {
        s_key[k] = ACC_EMPTY;
#pragma unroll
        for (int j = 0; j < 9; ++j) s_sum[k][j] = 0ull;
    }
    if (tid == 0) s_used = 0u;
    __syncthreads();
    for (uint32_t round = blockIdx.x; round < rounds; round += gridDim.x) {
        const uint32_t used = s_used;            // the same value in every thread: nobody inserts before the barrier below
        __syncthreads();
        if (used > ACC_SLOTS / 4u) {
            flush();
            if (tid == 0) s_used = 0u;
            __syncthreads();
        }
        const uint32_t i = round * MERGE_BLOCK + tid;
        const bool valid = i < b.n;
        uint32_t rank = 0;
        long long q[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (valid) {
            const uint32_t sl = b.slot[i];
            rank = b.trank[sl & ~MERGE_MIRRORED];
            const bool mir = (sl & MERGE_MIRRORED) != 0u;
#pragma unroll
            for (int a = 0; a < 7; ++a) q[mir ? 6 - a : a] = llrint((double)b.in.pis[(size_t)i * 7 + a] * 0x1p38);
            q[7] = llrint((double)b.in.zs[i] * 0x1p38);
        }
        // a whole wave on one group: sum across the wave, one lane goes on
        unsigned long long copies = 1ull;
        bool add = valid;
        if (__all(valid && rank == (uint32_t)__shfl((int)rank, 0))) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                long long v = q[j];
                for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
                q[j] = v;
            }
            copies = 64ull;
            add = lane == 0u;
        }
        if (add) {
            uint32_t h = (rank * 0x9E3779B1u) >> 23;          // 9 bits
            for (;;) {
                const uint32_t prev = atomicCAS(&s_key[h], ACC_EMPTY, rank);
                if (prev == ACC_EMPTY) atomicAdd(&s_used, 1u);
                if (prev == ACC_EMPTY || prev == rank) break;
                h = (h + 1u) & (ACC_SLOTS - 1u);
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) atomicAdd(&s_sum[h][j], (unsigned long long)q[j]);
            atomicAdd(&s_sum[h][8], copies);
        }
        __syncthreads();
    }
    flush();
}

// ---- finalise --------------------------------------------------------------------------------------------------------------------------
// a group of one copies its tuple's bits (no arithmetic touches them); a larger one divides its sums in double and rounds once to f32
__global__ __launch_bounds__(MERGE_BLOCK) void k_merge_finalise(MergeBufs b, uint32_t m) {
    const uint32_t j = blockIdx.x * MERGE_BLOCK + threadIdx.x;
    if (j >= m) return;
    const uint32_t i = b.first[j];
    const uint32_t k = b.cnt[j];
    b.o_states[j] = b.cst[i];
    if (k == 1u) {                               // verbatim: no arithmetic touches the values
        const bool mir = (b.slot[i] & MERGE_MIRRORED) != 0u;
        for (int a = 0; a < 7; ++a) b.o_pis[(size_t)j * 7 + (mir ? 6 - a : a)] = b.in.pis[(size_t)i * 7 + a];
        b.o_zs[j] = b.in.zs[i];
        return;
    }
    const double div = (double)((long long)k << MERGE_FRAC_BITS);          // k * 2^38 <= 2^62: exact
    for (int a = 0; a < 7; ++a) b.o_pis[(size_t)j * 7 + a] = (float)((double)(long long)b.sums[(size_t)j * 8 + a] / div);
    b.o_zs[j] = (float)((double)(long long)b.sums[(size_t)j * 8 + 7] / div);
}
template <class G>
__global__ __launch_bounds__(MERGE_BLOCK) void k_merge_boards(MergeBufs b, uint32_t m) {
    const size_t idx = (size_t)blockIdx.x * MERGE_BLOCK + threadIdx.x;
    if (idx >= (size_t)m * G::FEATURES) return;
    const uint32_t j = (uint32_t)(idx / G::FEATURES);
    b.o_boards[idx] = G::feature(b.o_states[j], (int)(idx % G::FEATURES));
}

inline unsigned merge_blocks(size_t items) { return (unsigned)((items + MERGE_BLOCK - 1) / MERGE_BLOCK); }

}  // namespace

void launch_merge_keys(int game, const MergeBufs& b, int canonical, hipStream_t s) {
    if (b.n == 0) return;
    if (game == 1) hipLaunchKernelGGL(k_merge_keys<ConnectThree>, dim3(merge_blocks(b.n)), dim3(MERGE_BLOCK), 0, s, b, canonical);
    else hipLaunchKernelGGL(k_merge_keys<ConnectFour>, dim3(merge_blocks(b.n)), dim3(MERGE_BLOCK), 0, s, b, canonical);
}
void launch_merge_scan(const MergeBufs& b, hipStream_t s) {
    if (b.n == 0) return;
    const unsigned nb = merge_blocks(b.n);
    hipLaunchKernelGGL(k_merge_scan_count, dim3(nb), dim3(MERGE_BLOCK), 0, s, b);
    hipLaunchKernelGGL(k_merge_scan_blocks, dim3(1), dim3(1024), 0, s, b, (uint32_t)nb);
    hipLaunchKernelGGL(k_merge_scan_rank, dim3(nb), dim3(MERGE_BLOCK), 0, s, b);
}
void launch_merge_accumulate(const MergeBufs& b, hipStream_t s) {
    if (b.n == 0) return;
    hipLaunchKernelGGL(k_merge_accumulate, dim3(std::min(merge_blocks(b.n), 2048u)), dim3(MERGE_BLOCK), 0, s, b);
}
void launch_merge_finalise(int game, const MergeBufs& b, uint32_t m, hipStream_t s) {
    if (m == 0) return;
    hipLaunchKernelGGL(k_merge_finalise, dim3(merge_blocks(m)), dim3(MERGE_BLOCK), 0, s, b, m);
    if (!b.o_boards) return;
    const unsigned nb = merge_blocks((size_t)m * ConnectFour::FEATURES);
    if (game == 1) hipLaunchKernelGGL(k_merge_boards<ConnectThree>, dim3(nb), dim3(MERGE_BLOCK), 0, s, b, m);
    else hipLaunchKernelGGL(k_merge_boards<ConnectFour>, dim3(nb), dim3(MERGE_BLOCK), 0, s, b, m);
}

}  // namespace az
