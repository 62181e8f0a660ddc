// az_target.hip -- the device side of az_samples_blend_z and az_samples_surprise (csrc/az_target.h): the blend, the
// KL pass with its per-workgroup integer sum, the copies, and the gather that writes tuple i c_i times.  The prefix sum between the last two
// is launch_draw_scan of az_draw.h.  Integer sums only where lanes meet: no result depends on the schedule.
#include "az_target.h"

#include <algorithm>

#include "az_draw.h"
#include "az_game.h"

namespace az {

static_assert(TARGET_RNG_SURPRISE == RNG_SURPRISE, "az_target.h restates az_common.h's purpose word");
static_assert(TARGET_ACTIONS == ConnectFour::ACTIONS && ConnectFour::FEATURES == 84, "7 actions; 84 feature cells: 21 lanes of 16 bytes per board");

namespace {

using u64 = unsigned long long;
constexpr uint32_t TARGET_BLOCK = 256;
constexpr int BOARD_VEC = 21;                 // float4 per board row (84 floats)

inline unsigned target_grid(int64_t items) { return (unsigned)std::min<int64_t>((items + TARGET_BLOCK - 1) / TARGET_BLOCK, 65536); }

__global__ __launch_bounds__(TARGET_BLOCK) void k_target_blend(const float* __restrict__ zs, const float* __restrict__ rq, int64_t n, int64_t lambda_e6,
                                                               float* __restrict__ out, uint32_t* __restrict__ bad) {
    uint32_t mine_bad = 0u;
    for (int64_t i = (int64_t)blockIdx.x * TARGET_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * TARGET_BLOCK) {
        const float z = zs[i], r = rq[i];
        if (!sample_in_unit(z) || !sample_in_unit(r)) mine_bad = SAMPLE_BAD_VALUE;
        out[i] = target_blend(lambda_e6, z, r);
    }
    if (mine_bad) atomicOr(bad, mine_bad);
}

// one thread per tuple; whole workgroups (no early return: the sum below meets in LDS)
__global__ __launch_bounds__(TARGET_BLOCK) void k_target_kl(SampleWindow w, const float* __restrict__ priors, int64_t n, float* __restrict__ kl,
                                                            u64* __restrict__ K, u64* __restrict__ SK, uint32_t* __restrict__ bad) {
    __shared__ u64 s_w[TARGET_BLOCK / 64];
    const int64_t i = (int64_t)blockIdx.x * TARGET_BLOCK + threadIdx.x;
    u64 k = 0ull;
    if (i < n) {
        uint64_t mine, theirs;
        uint32_t b = sample_check(w, i, false, &mine, &theirs);
        float pi[TARGET_ACTIONS], pr[TARGET_ACTIONS];
#pragma unroll
        for (int a = 0; a < TARGET_ACTIONS; ++a) {
            pi[a] = w.pis[(size_t)i * TARGET_ACTIONS + a];
            pr[a] = priors[(size_t)i * TARGET_ACTIONS + a];
            if (!sample_is_prior(pr[a])) b |= SAMPLE_BAD_PRIOR;
        }
        if (b) atomicOr(bad, b);                 // the call is refused: nothing behind this pass runs
        else {
            const float v = target_kl(pi, pr);
            k = (u64)target_kl_fixed(v);
            kl[i] = v;
            K[i] = k;
        }
    }
    u64 x = k;
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
    if ((threadIdx.x & 63u) == 0u) s_w[threadIdx.x >> 6] = x;
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 t = 0;
        for (uint32_t w = 0; w < TARGET_BLOCK / 64; ++w) t += s_w[w];
        if (t) atomicAdd(SK, t);
    }
}

__global__ __launch_bounds__(TARGET_BLOCK) void k_target_copies(const u64* __restrict__ K, const u64* __restrict__ SK, int64_t n, int64_t share_e6,
                                                                uint64_t seed, uint32_t* __restrict__ counts) {
    const u64 sk = *SK;
    for (int64_t i = (int64_t)blockIdx.x * TARGET_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * TARGET_BLOCK)
        counts[i] = target_copies(target_weight(share_e6, n, K[i], sk), seed, (uint64_t)i);
}

// one thread per output row: the binary search over Q
__global__ __launch_bounds__(TARGET_BLOCK) void k_target_rows(const uint64_t* __restrict__ Q, int64_t n, int64_t total, uint32_t* __restrict__ idx) {
    for (int64_t r = (int64_t)blockIdx.x * TARGET_BLOCK + threadIdx.x; r < total; r += (int64_t)gridDim.x * TARGET_BLOCK)
        idx[r] = (uint32_t)draw_search(Q, n, (uint64_t)r);
}

// LANES lanes per output row: lanes 0 .. 20 carry 16 bytes of the row's board each (BOARDS), the last lane the state's 16 bytes, pi and z
// (a pi row is 28 bytes: no 16-byte alignment to use)
template <bool BOARDS>
__global__ __launch_bounds__(TARGET_BLOCK) void k_target_gather(const uint32_t* __restrict__ idx, int64_t total, const ulonglong2* __restrict__ states,
                                                                const float4* __restrict__ boards, const float* __restrict__ pis,
                                                                const float* __restrict__ zs, ulonglong2* __restrict__ o_states,
                                                                float4* __restrict__ o_boards, float* __restrict__ o_pis, float* __restrict__ o_zs) {
    constexpr int LANES = BOARDS ? BOARD_VEC + 1 : 1;
    const int64_t items = total * LANES;
    for (int64_t it = (int64_t)blockIdx.x * TARGET_BLOCK + threadIdx.x; it < items; it += (int64_t)gridDim.x * TARGET_BLOCK) {
        const int64_t r = it / LANES;
        const int c = (int)(it % LANES);
        const size_t i = idx[r];
        if (BOARDS && c < BOARD_VEC) {
            o_boards[(size_t)r * BOARD_VEC + c] = boards[i * BOARD_VEC + c];
            continue;
        }
        if (o_states) o_states[r] = states[i];
        if (o_pis) {
#pragma unroll
            for (int a = 0; a < TARGET_ACTIONS; ++a) o_pis[(size_t)r * TARGET_ACTIONS + a] = pis[i * TARGET_ACTIONS + a];
        }
        if (o_zs) o_zs[r] = zs[i];
    }
}

}  // namespace

void launch_target_blend(const float* zs, const float* root_q, int64_t n, int64_t lambda_e6, float* out, uint32_t* bad, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_target_blend, dim3(target_grid(n)), dim3(TARGET_BLOCK), 0, s, zs, root_q, n, lambda_e6, out, bad);
}
void launch_target_kl(const SampleWindow& w, const float* priors, int64_t n, float* kl, uint64_t* K, uint64_t* SK, uint32_t* bad, hipStream_t s) {
    if (n <= 0) return;
    const unsigned nb = (unsigned)((n + TARGET_BLOCK - 1) / TARGET_BLOCK);          // n <= 2^24: at most 65536 workgroups
    hipLaunchKernelGGL(k_target_kl, dim3(nb), dim3(TARGET_BLOCK), 0, s, w, priors, n, kl, (u64*)K, (u64*)SK, bad);
}
void launch_target_copies(const uint64_t* K, const uint64_t* SK, int64_t n, int64_t share_e6, uint64_t seed, uint32_t* counts, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_target_copies, dim3(target_grid(n)), dim3(TARGET_BLOCK), 0, s, (const u64*)K, (const u64*)SK, n, share_e6, seed, counts);
}
void launch_target_gather(const uint64_t* Q, int64_t n, int64_t total, uint32_t* idx, const ulonglong2* states, const float* boards, const float* pis,
                          const float* zs, ulonglong2* o_states, float* o_boards, float* o_pis, float* o_zs, hipStream_t s) {
    if (n <= 0 || total <= 0) return;
    hipLaunchKernelGGL(k_target_rows, dim3(target_grid(total)), dim3(TARGET_BLOCK), 0, s, Q, n, total, idx);
    if (o_boards)
        hipLaunchKernelGGL(k_target_gather<true>, dim3(target_grid(total * (BOARD_VEC + 1))), dim3(TARGET_BLOCK), 0, s, idx, total, states,
                           (const float4*)boards, pis, zs, o_states, (float4*)o_boards, o_pis, o_zs);
    else
        hipLaunchKernelGGL(k_target_gather<false>, dim3(target_grid(total)), dim3(TARGET_BLOCK), 0, s, idx, total, states, (const float4*)nullptr, pis, zs,
                           o_states, (float4*)nullptr, o_pis, o_zs);
}

}  // namespace az
