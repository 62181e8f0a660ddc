// az_draw.hip -- the device side of the weighted batch draws (csrc/az_draw.h): the u64 prefix sum of the u32
// weights (block reduce, scan of the block sums, block scan -- k_merge_scan_* of az_merge.hip is the precedent), the draw kernel that fills
// an epoch's index table and mirror bits, and the state check of az_net_train_samples.  Integer sums: no result depends on the schedule.
#include "az_draw.h"

#include <algorithm>

#include "az_game.h"
#include "az_samples.h"

namespace az {

static_assert(DRAW_RNG_BATCH == RNG_BATCH && DRAW_RNG_TRAIN_MIRROR == RNG_TRAIN_MIRROR, "az_draw.h restates az_common.h's purpose words");

namespace {

using u64 = unsigned long long;

// this thread's DRAW_SCAN_ITEMS consecutive weights of the block (0 behind the end), and their sum
__device__ __forceinline__ u64 draw_load(const uint32_t* __restrict__ w, int64_t n, uint32_t v[DRAW_SCAN_ITEMS]) {
    const int64_t base = (int64_t)blockIdx.x * DRAW_SCAN_BLOCK + (int64_t)threadIdx.x * DRAW_SCAN_ITEMS;
    u64 sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < DRAW_SCAN_ITEMS; ++k) {
        v[k] = base + k < n ? w[base + k] : 0u;
        sum += v[k];
    }
    return sum;
}

// pass 1: bsum[block] = the sum of the block's weights
__global__ __launch_bounds__(DRAW_SCAN_THREADS) void k_draw_scan_reduce(const uint32_t* __restrict__ w, int64_t n, u64* __restrict__ bsum) {
    __shared__ u64 s_w[DRAW_SCAN_THREADS / 64];
    uint32_t v[DRAW_SCAN_ITEMS];
    u64 x = draw_load(w, n, v);
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
    if ((threadIdx.x & 63u) == 0u) s_w[threadIdx.x >> 6] = x;
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 t = 0;
        for (uint32_t k = 0; k < DRAW_SCAN_THREADS / 64; ++k) t += s_w[k];
        bsum[blockIdx.x] = t;
    }
}

// pass 2, one workgroup of DRAW_SCAN_GROUP: bsum[0 .. nb) becomes its exclusive scan, *total the sum of all.  More block sums than the
// workgroup holds are taken in rounds of DRAW_SCAN_GROUP with a running carry.
__global__ __launch_bounds__(DRAW_SCAN_GROUP) void k_draw_scan_blocks(u64* __restrict__ bsum, uint64_t nb, u64* __restrict__ total) {
    __shared__ u64 s_w[DRAW_SCAN_GROUP / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    u64 carry = 0;
    for (uint64_t base = 0; base < nb; base += DRAW_SCAN_GROUP) {
        const uint64_t idx = base + tid;
        const u64 v = idx < nb ? bsum[idx] : 0ull;
        u64 x = v;
        for (uint32_t off = 1; off < 64u; off <<= 1) {
            const u64 y = __shfl_up(x, off);
            if (lane >= off) x += y;
        }
        if (lane == 63u) s_w[wave] = x;
        __syncthreads();
        u64 before = 0, sum = 0;
        for (uint32_t k = 0; k < DRAW_SCAN_GROUP / 64; ++k) {
            const u64 t = s_w[k];
            if (k < wave) before += t;
            sum += t;
        }
        if (idx < nb) bsum[idx] = carry + before + x - v;
        carry += sum;
        __syncthreads();
    }
    if (tid == 0) *total = carry;
}

// pass 3: Q[i] = bsum[block] + the inclusive scan inside the block
__global__ __launch_bounds__(DRAW_SCAN_THREADS) void k_draw_scan_apply(const uint32_t* __restrict__ w, int64_t n, const u64* __restrict__ bsum,
                                                                       u64* __restrict__ Q) {
    __shared__ u64 s_w[DRAW_SCAN_THREADS / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t v[DRAW_SCAN_ITEMS];
    const u64 mine = draw_load(w, n, v);
    u64 x = mine;
    for (uint32_t off = 1; off < 64u; off <<= 1) {
        const u64 y = __shfl_up(x, off);
        if (lane >= off) x += y;
    }
    if (lane == 63u) s_w[wave] = x;
    __syncthreads();
    u64 acc = bsum[blockIdx.x] + x - mine;
    for (uint32_t k = 0; k < wave; ++k) acc += s_w[k];
    const int64_t base = (int64_t)blockIdx.x * DRAW_SCAN_BLOCK + (int64_t)tid * DRAW_SCAN_ITEMS;
#pragma unroll
    for (uint32_t k = 0; k < DRAW_SCAN_ITEMS; ++k) {
        acc += v[k];
        if (base + k < n) Q[base + k] = acc;
    }
}

// one thread per (step, j): the multiply-high, the binary search over Q, the mirror bit
__global__ __launch_bounds__(256) void k_draw_rows(const uint64_t* __restrict__ Q, int64_t n, uint64_t W, uint64_t seed, uint64_t t0, int64_t rows,
                                                   int b, int mirror, int64_t* __restrict__ idx, uint8_t* __restrict__ mir) {
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < rows; k += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t t = t0 + (uint64_t)(k / b), j = (uint64_t)(k % b);
        idx[k] = draw_row(Q, n, W, seed, t, j);
        if (mir) mir[k] = (mirror && draw_mirrored(seed, t, j)) ? 1 : 0;
    }
}

__global__ __launch_bounds__(256) void k_draw_check_states(const ulonglong2* __restrict__ states, int64_t n, uint32_t* __restrict__ bad) {
    uint32_t mine_bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const ulonglong2 s = states[i];
        mine_bad |= sample_state_bits(s.x, s.y);
    }
    if (mine_bad) atomicOr(bad, mine_bad);
}

inline unsigned draw_grid(int64_t items) { return (unsigned)std::min<int64_t>((items + 255) / 256, 65536); }

}  // namespace

void launch_draw_scan(const uint32_t* w, int64_t n, uint64_t* Q, uint64_t* bsum, uint64_t* total, hipStream_t s) {
    if (n <= 0) return;
    const size_t nb = draw_scan_blocks(n);
    hipLaunchKernelGGL(k_draw_scan_reduce, dim3((unsigned)nb), dim3(DRAW_SCAN_THREADS), 0, s, w, n, (u64*)bsum);
    hipLaunchKernelGGL(k_draw_scan_blocks, dim3(1), dim3(DRAW_SCAN_GROUP), 0, s, (u64*)bsum, (uint64_t)nb, (u64*)total);
    hipLaunchKernelGGL(k_draw_scan_apply, dim3((unsigned)nb), dim3(DRAW_SCAN_THREADS), 0, s, w, n, (const u64*)bsum, (u64*)Q);
}

void launch_draw_rows(const uint64_t* Q, int64_t n, uint64_t W, uint64_t seed, uint64_t t0, int64_t steps, int b, bool mirror, int64_t* idx,
                      uint8_t* mir, hipStream_t s) {
    const int64_t rows = steps * b;
    if (rows <= 0) return;
    hipLaunchKernelGGL(k_draw_rows, dim3(draw_grid(rows)), dim3(256), 0, s, Q, n, W, seed, t0, rows, b, mirror ? 1 : 0, idx, mir);
}

void launch_draw_check_states(const ulonglong2* states, int64_t n, uint32_t* bad, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_draw_check_states, dim3(draw_grid(n)), dim3(256), 0, s, states, n, bad);
}

}  // namespace az
