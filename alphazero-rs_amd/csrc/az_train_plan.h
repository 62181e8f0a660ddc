// az_train_plan.h -- which kernel chain every layer of one NNet::train step takes, decided once from the seven route switches and the
// shape (batch b, width C).  HIP-free: enqueue_step and the launchers of az_train.hip consume it, az_set_option fills the switches, and the
// g++ twin of the tests (tests/cpp/train_plan_twin.cpp) compiles this text and is held to an independent restatement of the rules
// (tests/test_train_plan_cpu.py; DESIGN.md section 8, "the step plan").
//
//   layers      l = 0..5: conv1..conv4, fc1, fc2.  Rows M_l = {42 b, 42 b, 20 b, 6 b, b, b}, contraction K_l = {18 (row stride 20), 9 C,
//               9 C, 9 C, 6 C, 1024}, outputs N_l = {C, C, C, C, 1024, 512}
//   x3          "train_gemm" 1: the backward GEMMs above conv1 as bf16 x 3; with "train_fwd_x3" also conv2..conv4's forward as f16 x 3
//   gathered    conv2..conv4's GEMMs gather their A rows from the activations (ImplicitA): no im2col matrix, no col2im behind conv2
//   a GemmPlan  names the kernel family and the GEMM as that kernel sees it (output [M][N], contraction K), which fixes its split-K
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <initializer_list>

namespace az {

struct TrainSwitches {          // az_set_option "train_<member>", each 0 / 1 ("train_graph" is no route: az_train.h trainer_set_graph)
    int gemm = 1;               // the GEMMs as bf16 / f16 x 3 on the 16-bit matrix cores; 0: every GEMM on v_mfma_f32_16x16x4_f32
    int fwd_dma = 1;            // f32 forward GEMMs fed by LDS-DMA (k_gemm_f32_dma) where its shape rule holds; 0: register-staged k_gemm_f32
    int fwd_x3 = 1;             // conv2..conv4 forward as f16 x 3; 0: f32
    int wgrad_tr = 1;           // wgrad on k_wgrad3_tr (transposed LDS reads) where its shapes hold; 0: transpose kernels + k_gemm3
    int implicit = 1;           // the gathered conv GEMMs where their shapes hold; 0: im2col / col2im
    int gemm3_ring = 1;         // the big x 3 GEMMs on k_gemm3_ring (one 8-wave workgroup per CU, 3-stage ring); 0: k_gemm3
    int fork = 0;               // the weight split and the wgrad chains on a second stream branch (no gain: profiles/README.md)
};

// the tile and step sizes the rules below depend on; az_train.hip asserts that its kernels' constants agree
constexpr int PLAN_BN_SMALL_ROWS = 64, PLAN_F32_BK = 16, PLAN_DMA_BK = 16, PLAN_G3_BM = 128, PLAN_G3R_BM = 256, PLAN_X3_BK = 32;

enum GemmKernel : int32_t { GK_NONE = 0, GK_F32_64, GK_F32_128, GK_F32_DMA, GK_GEMM3, GK_GEMM3_RING, GK_WGRAD3_TR };
enum FwdRoute : int32_t { FWD_F32 = 0, FWD_X3_COL, FWD_X3_GATHER };      // gemm_nn / f16 x 3 from the im2col pairs / gathered f16 x 3
enum WgradRoute : int32_t {
    WGRAD_F32 = 0,              // gemm_tn
    WGRAD_TR_GATHER,            // k_wgrad3_tr, A gathered from the layer's input activations
    WGRAD_TR_ACT,               // k_wgrad3_tr from the previous layer's bf16 pairs (the FC layers)
    WGRAD_TR_COL,               // k_wgrad3_tr from the stored im2col pairs
    WGRAD_TRANSPOSE,            // k_transpose_split of both operands, then launch_gemm3
};
enum DgradRoute : int32_t { DGRAD_NONE = 0, DGRAD_F32, DGRAD_X3, DGRAD_X3_GATHER };
enum DgradDst : int32_t { DST_NONE = 0, DST_DACT, DST_DCOL };
enum : int32_t { BN_OUT_F16 = 1, BN_OUT_BF16 = 2 };                     // BatchNorm-forward extras: half pairs + the scale, bf16 pairs
enum : int32_t { COL_F32 = 1, COL_F16 = 2, COL_BF16 = 4 };              // k_im2col outputs; 0: not launched
enum WeightSplit : int32_t { SPLIT_NONE = 0, SPLIT_IN_PREP, SPLIT_SIDE_START, SPLIT_AFTER_HEADS };      // where k_split_weights' work runs
enum FwdPrep : int32_t { PREP_NONE = 0, PREP_ONE, PREP_TWO };           // k_weight_prep / k_transpose_split<true> + k_act_scales

struct GemmPlan { int32_t kernel, M, N, K, side_ws; };                  // side_ws 1: the side branch's split-K workspace

struct LayerPlan {
    int32_t fwd, bn_small, bn_extra, im2col, wgrad, dgrad, dgrad_dst, col2im;      // im2col: the k_im2col behind this layer (l <= 2)
    GemmPlan fwd_gemm, wgrad_gemm, dgrad_gemm;
};

struct StepPlan {
    int32_t x3, fork, perm_conv2, split, prep;      // perm_conv2: conv2's split weights permuted for the gathered dgrad
    LayerPlan layer[6];
};

constexpr int TRAIN_PLAN_INTS = 5 + 6 * (8 + 3 * 5);

// ---- the launchers' kernel-family rules --------------------------------------------------------------------------------------------
// k_gemm_f32: 128 x 128 tiles when K is long and the output still yields >= 64 of them, else 64 x 64
inline bool gemm_f32_big(int M, int N, int K) { return K >= 256 && ((M + 127) / 128) * ((N + 127) / 128) >= 64; }
// k_gemm_f32_dma: 128 x 128 tiles, whole 16-wide K-steps (at least 8), rows that keep the 16-byte DMA aligned
inline bool gemm_f32_dma_ok(int M, int N, int K, int64_t lda) {
    return M >= 128 && K % PLAN_DMA_BK == 0 && K >= 8 * PLAN_DMA_BK && N % 128 == 0 && lda % 4 == 0;
}
// k_gemm3_ring instead of k_gemm3: a gathered A exists on the ring kernel only; else the switch, a contraction long enough to fill and
// drain the ring (conv4's wgrad has 12 K-steps: 14.9 us on k_gemm3, 15.8 on the ring) and at most a tenth of the row tiles' rows beyond M
inline bool gemm3_on_ring(bool gathered_a, bool ring, int M, int Kc) {
    const int mt = (M + PLAN_G3R_BM - 1) / PLAN_G3R_BM;
    return gathered_a || (ring && Kc / PLAN_X3_BK >= 16 && (mt * PLAN_G3R_BM - M) * 10 <= mt * PLAN_G3R_BM);
}

// ---- split-K -------------------------------------------------------------------------------------------------------------------------
struct SplitK { int steps_per_slice, splits; };
// `want` slices of a contraction of `steps` K-steps, fewer while their partial sums (out_elems floats each) do not fit the workspace; the
// slices are then made equal, which can drop some more.  No slice is empty.
inline SplitK splitk_pick(int steps, int want, size_t out_elems, size_t ws_floats) {
    int splits = want > 1 ? want : 1;
    while (splits > 1 && (size_t)splits * out_elems > ws_floats) --splits;
    const int sps = (steps + splits - 1) / splits;
    return SplitK{sps, (steps + sps - 1) / sps};
}
struct SplitWant { int steps, want; };
// how many slices each kernel family asks for: enough workgroups for the device's 256 CUs without a second round of a few, and a minimum
// of K-steps per slice (the ring kernels are 3 deep: 6; the others 8)
inline SplitWant gemm_split_want(const GemmPlan& g) {
    auto lesser = [](int a, int b) { return a < b ? a : b; };
    switch (g.kernel) {
    case GK_F32_64: case GK_F32_128: {
        const int big = g.kernel == GK_F32_128, TM = big ? 128 : 64, tiles = ((g.M + TM - 1) / TM) * ((g.N + TM - 1) / TM);
        const int steps = (g.K + PLAN_F32_BK - 1) / PLAN_F32_BK;
        return {steps, lesser((big ? 768 : 1536) / (tiles > 1 ? tiles : 1), steps / 8)};
    }
    case GK_F32_DMA: {          // two workgroups per CU: 512 slots a round
        const int tiles = ((g.M + 127) / 128) * (g.N / 128), steps = g.K / PLAN_DMA_BK;
        return {steps, lesser(512 / tiles, steps / 8)};
    }
    case GK_GEMM3: {            // about two workgroups per CU
        const int tiles = ((g.M + PLAN_G3_BM - 1) / PLAN_G3_BM) * (g.N / 128), steps = g.K / PLAN_X3_BK;
        return {steps, lesser((512 + tiles / 2) / tiles, steps / 8)};
    }
    case GK_GEMM3_RING: {       // ONE workgroup per CU: never more than 256 of them while the tiles fit
        const int tiles = ((g.M + PLAN_G3R_BM - 1) / PLAN_G3R_BM) * (g.N / 128), steps = g.K / PLAN_X3_BK;
        return {steps, lesser(256 / tiles, steps / 6)};
    }
    case GK_WGRAD3_TR: {        // out [Kin][N] in 256 x 128 tiles, the contraction in 32-row steps
        const int tiles = (g.M / 256) * (g.N / 128), steps = g.K / PLAN_X3_BK;
        return {steps, lesser(256 / tiles, steps / 6)};
    }
    default: return {1, 1};
    }
}
inline SplitK gemm_splitk(const GemmPlan& g, size_t ws_floats) {
    const SplitWant w = gemm_split_want(g);
    return splitk_pick(w.steps, w.want, (size_t)g.M * (size_t)g.N, ws_floats);
}

// ---- the plan ------------------------------------------------------------------------------------------------------------------------
inline GemmPlan plan_gemm_f32(int M, int N, int K, bool dma = false) {
    return GemmPlan{dma ? GK_F32_DMA : gemm_f32_big(M, N, K) ? GK_F32_128 : GK_F32_64, M, N, K, 0};
}
inline GemmPlan plan_gemm3(bool gathered_a, bool ring, int M, int N, int Kc, bool side_ws = false) {
    return GemmPlan{gemm3_on_ring(gathered_a, ring, M, Kc) ? GK_GEMM3_RING : GK_GEMM3, M, N, Kc, side_ws ? 1 : 0};
}

inline StepPlan train_step_plan(const TrainSwitches& sw, bool side_stream_exists, int b, int C) {
    const int M[6] = {b * 42, b * 42, b * 20, b * 6, b, b}, K[6] = {18, 9 * C, 9 * C, 9 * C, 6 * C, 1024}, N[6] = {C, C, C, C, 1024, 512};
    const int64_t lda[6] = {20, 9ll * C, 9ll * C, 9ll * C, 6ll * C, 1024};
    const bool x3 = sw.gemm == 1, fx3 = x3 && sw.fwd_x3, fork = x3 && sw.fork && side_stream_exists, ring = sw.gemm3_ring != 0;
    // the gathered conv GEMMs need the f16 x 3 forward and k_wgrad3_tr's shapes on all three convs (42 b, 20 b, 6 b rows in 32s)
    const bool gathered = fx3 && sw.implicit && sw.wgrad_tr && b % 16 == 0 && b * 20 > PLAN_BN_SMALL_ROWS && C % 256 == 0;
    auto tr_shape = [&](int l, int rows) { return x3 && sw.wgrad_tr && rows % 32 == 0 && K[l] % 256 == 0 && N[l] % 128 == 0; };
    auto col_tr = [&](int l) { return l >= 1 && l <= 3 && tr_shape(l, M[l]); };
    auto fc_tr = [&](int l) { return l >= 4 && l <= 5 && tr_shape(l, b); };
    StepPlan p{};
    p.x3 = x3; p.fork = fork; p.perm_conv2 = gathered;
    p.split = !x3 ? SPLIT_NONE : fork ? SPLIT_SIDE_START : fx3 ? SPLIT_IN_PREP : SPLIT_AFTER_HEADS;
    p.prep = !fx3 ? PREP_NONE : fork ? PREP_TWO : PREP_ONE;
    for (int l = 0; l < 6; ++l) {
        LayerPlan& q = p.layer[l];
        const bool conv234 = l >= 1 && l <= 3;
        if (conv234 && gathered) { q.fwd = FWD_X3_GATHER; q.fwd_gemm = plan_gemm3(true, ring, M[l], N[l], K[l]); }
        else if (conv234 && fx3) { q.fwd = FWD_X3_COL; q.fwd_gemm = plan_gemm3(false, ring, M[l], N[l], K[l]); }
        else { q.fwd = FWD_F32; q.fwd_gemm = plan_gemm_f32(M[l], N[l], K[l], sw.fwd_dma && gemm_f32_dma_ok(M[l], N[l], K[l], lda[l])); }
        q.bn_small = M[l] <= PLAN_BN_SMALL_ROWS;
        q.bn_extra = (l <= 2 && gathered ? BN_OUT_F16 | BN_OUT_BF16 : 0) | ((l == 3 || l == 4) && fc_tr(l + 1) ? BN_OUT_BF16 : 0);
        if (l <= 2 && !gathered)
            q.im2col = (fx3 ? COL_F16 : 0) | (col_tr(l + 1) ? COL_BF16 : 0) | (!fx3 || !col_tr(l + 1) ? COL_F32 : 0);
        // wgrad: dW [K][N] = A^T dz
        if (l == 0 || !x3) { q.wgrad = WGRAD_F32; q.wgrad_gemm = plan_gemm_f32(K[l], N[l], M[l]); }
        else if (conv234 && gathered) q.wgrad = WGRAD_TR_GATHER;
        else if (fc_tr(l)) q.wgrad = WGRAD_TR_ACT;
        else if (col_tr(l)) q.wgrad = WGRAD_TR_COL;
        else { q.wgrad = WGRAD_TRANSPOSE; q.wgrad_gemm = plan_gemm3(false, ring, K[l], N[l], (M[l] + 63) / 64 * 64, fork); }
        if (q.wgrad == WGRAD_TR_GATHER || q.wgrad == WGRAD_TR_ACT || q.wgrad == WGRAD_TR_COL)
            q.wgrad_gemm = GemmPlan{GK_WGRAD3_TR, K[l], N[l], M[l], fork ? 1 : 0};
        // dgrad: d input [M][K] = dz W^T; conv2's gathered form is the transposed convolution as one GEMM over (tap, n), straight into dact
        if (l == 0) continue;
        q.dgrad_dst = l >= 4 || (l == 1 && gathered) ? DST_DACT : DST_DCOL;
        if (!x3) { q.dgrad = DGRAD_F32; q.dgrad_gemm = plan_gemm_f32(M[l], K[l], N[l]); }
        else if (l == 1 && gathered) { q.dgrad = DGRAD_X3_GATHER; q.dgrad_gemm = plan_gemm3(true, ring, b * 42, C, 9 * N[l]); }
        else { q.dgrad = DGRAD_X3; q.dgrad_gemm = plan_gemm3(false, ring, M[l], K[l], N[l]); }
        q.col2im = conv234 && q.dgrad != DGRAD_X3_GATHER;
    }
    return p;
}

// the plan as TRAIN_PLAN_INTS int32, in declaration order (the tests' twin and the diagnostic library's az_diag_train_plan) -> the count,
// or -1 when cap is too small
inline int train_plan_encode(const StepPlan& p, int32_t* out, int cap) {
    if (cap < TRAIN_PLAN_INTS) return -1;
    int n = 0;
    for (int32_t v : {p.x3, p.fork, p.perm_conv2, p.split, p.prep}) out[n++] = v;
    for (const LayerPlan& q : p.layer) {
        for (int32_t v : {q.fwd, q.bn_small, q.bn_extra, q.im2col, q.wgrad, q.dgrad, q.dgrad_dst, q.col2im}) out[n++] = v;
        for (const GemmPlan* g : {&q.fwd_gemm, &q.wgrad_gemm, &q.dgrad_gemm})
            for (int32_t v : {g->kernel, g->M, g->N, g->K, g->side_ws}) out[n++] = v;
    }
    return n;
}

}  // namespace az
