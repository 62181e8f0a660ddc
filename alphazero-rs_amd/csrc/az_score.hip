// az_score.hip -- the device side of az_net_evaluate and az_samples_holdout (csrc/az_score.h, DESIGN.md sections 4.1l and 8.3): the pass
// that validates the tuples and hands the forwards their states, the score kernel that runs behind every chunk's forward, and the hold-out
// mask.  Integer sums only where lanes meet: no result depends on the schedule.
#include "az_score.h"

#include "az_game.h"

namespace az {

static_assert(TARGET_ACTIONS == ConnectFour::ACTIONS && ConnectFour::FEATURES == 84, "7 actions; 84 feature cells");
static_assert(MIRROR_BOTTOM == C4_BOTTOM && (C4_FULL >> 5 & 1ull) && !(C4_FULL >> 6 & 1ull), "az_score.h restates az_game.h's pack word and top cell (c4_top: bit c * 7 + 5)");

namespace {

using u64 = unsigned long long;
constexpr uint32_t SCORE_BLOCK = 256;

inline unsigned score_blocks(int64_t items) { return (unsigned)((items + SCORE_BLOCK - 1) / SCORE_BLOCK); }      // n <= 2^24: at most 65536

__global__ __launch_bounds__(SCORE_BLOCK) void k_score_states(SampleWindow w, int strict, int64_t n, ulonglong2* __restrict__ out,
                                                              uint32_t* __restrict__ bad) {
    const int64_t i = (int64_t)blockIdx.x * SCORE_BLOCK + threadIdx.x;
    if (i >= n) return;
    uint64_t mine, theirs;
    const uint32_t b = sample_check(w, i, strict != 0, &mine, &theirs);
    if (b) atomicOr(bad, b);                     // the call is refused; the forwards behind this pass see an empty board in the tuple's place
    out[i] = b ? make_ulonglong2(0ull, 0ull) : make_ulonglong2(mine, theirs);
}

// one thread per row; whole workgroups (no early return: the sums below meet in LDS)
__global__ __launch_bounds__(SCORE_BLOCK) void k_score(const float* __restrict__ net_pi, const float* __restrict__ net_v,
                                                       const ulonglong2* __restrict__ states, const float* __restrict__ pis,
                                                       const float* __restrict__ zs, const uint32_t* __restrict__ weights, int64_t first, int rows,
                                                       u64* __restrict__ sums, float* __restrict__ ce_out, float* __restrict__ se_out,
                                                       float* __restrict__ kl_out) {
    __shared__ u64 s_w[SCORE_BLOCK / 64][SCORE_SUMS];
    const int r = (int)(blockIdx.x * SCORE_BLOCK + threadIdx.x);
    u64 x[SCORE_SUMS] = {0ull, 0ull, 0ull, 0ull, 0ull};
    if (r < rows) {
        const int64_t i = first + r;
        float p[TARGET_ACTIONS], pi[TARGET_ACTIONS];
#pragma unroll
        for (int a = 0; a < TARGET_ACTIONS; ++a) {
            p[a] = net_pi[(size_t)r * 8 + a];
            pi[a] = pis[(size_t)i * TARGET_ACTIONS + a];
        }
        const ulonglong2 st = states[i];
        const float ce = score_ce(pi, p), kl = target_kl(pi, p), se = score_se(net_v[r], zs[i]);
        const u64 w = weights ? (u64)weights[i] : 1ull;
        x[0] = w * (u64)score_fixed(ce);
        x[1] = w * (u64)score_fixed(kl);
        x[2] = w * (u64)score_fixed(se);
        x[3] = w * (u64)score_hit(pi, p, st.x, st.y);
        x[4] = w;
        if (ce_out) ce_out[i] = ce;
        if (se_out) se_out[i] = se;
        if (kl_out) kl_out[i] = kl;
    }
#pragma unroll
    for (int j = 0; j < SCORE_SUMS; ++j)
        for (int off = 32; off > 0; off >>= 1) x[j] += __shfl_xor(x[j], off);
    if ((threadIdx.x & 63u) == 0u)
        for (int j = 0; j < SCORE_SUMS; ++j) s_w[threadIdx.x >> 6][j] = x[j];
    __syncthreads();
    if (threadIdx.x < SCORE_SUMS) {
        u64 t = 0;
        for (uint32_t w = 0; w < SCORE_BLOCK / 64; ++w) t += s_w[w][threadIdx.x];
        if (t) atomicAdd(&sums[threadIdx.x], t);
    }
}

__global__ __launch_bounds__(SCORE_BLOCK) void k_score_holdout(const ulonglong2* __restrict__ states, int64_t n, uint64_t seed, uint64_t thresh24,
                                                               uint8_t* __restrict__ held) {
    const int64_t i = (int64_t)blockIdx.x * SCORE_BLOCK + threadIdx.x;
    if (i >= n) return;
    const ulonglong2 s = states[i];
    held[i] = score_held(seed, score_holdout_key(s.x, s.y), thresh24) ? 1 : 0;
}

}  // namespace

void launch_score_states(const SampleWindow& w, int strict, int64_t n, ulonglong2* out, uint32_t* bad, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_score_states, dim3(score_blocks(n)), dim3(SCORE_BLOCK), 0, s, w, strict, n, out, bad);
}
void launch_score(const float* net_pi, const float* net_v, const ulonglong2* states, const float* pis, const float* zs, const uint32_t* weights,
                  int64_t first, int rows, uint64_t* sums, float* ce, float* se, float* kl, hipStream_t s) {
    if (rows <= 0) return;
    hipLaunchKernelGGL(k_score, dim3(score_blocks(rows)), dim3(SCORE_BLOCK), 0, s, net_pi, net_v, states, pis, zs, weights, first, rows, (u64*)sums, ce,
                       se, kl);
}
void launch_score_holdout(const ulonglong2* states, int64_t n, uint64_t seed, uint64_t thresh24, uint8_t* held, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_score_holdout, dim3(score_blocks(n)), dim3(SCORE_BLOCK), 0, s, states, n, seed, thresh24, held);
}

}  // namespace az
