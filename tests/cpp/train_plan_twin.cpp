// csrc/az_train_plan.h compiled by g++ behind ctypes (tests/train_plan_twin.py): the step plan of NNet::train for batches of calls, the
// split-K of every GEMM a plan names, and splitk_pick alone.  TEST INFRASTRUCTURE ONLY.
#include <cstdint>

#include "az_train_plan.h"

using namespace az;

extern "C" {

int twin_plan_ints() { return TRAIN_PLAN_INTS; }

// in [n][10]: gemm, fwd_dma, fwd_x3, wgrad_tr, implicit, gemm3_ring, fork, side stream exists, b, C -> out [n][TRAIN_PLAN_INTS]
void twin_train_plans(int64_t n, const int32_t* in, int32_t* out) {
    for (int64_t i = 0; i < n; ++i) {
        const int32_t* r = in + i * 10;
        const TrainSwitches sw{r[0], r[1], r[2], r[3], r[4], r[5], r[6]};
        (void)train_plan_encode(train_step_plan(sw, r[7] != 0, r[8], r[9]), out + i * TRAIN_PLAN_INTS, TRAIN_PLAN_INTS);
    }
}

// gemms [n][5]: kernel, M, N, K, side_ws (a GemmPlan as encoded; kernel 0 rows give zeros) -> out [n][4]: steps, want, steps per slice, splits
void twin_gemm_splits(int64_t n, const int32_t* gemms, int64_t ws_main, int64_t ws_side, int32_t* out) {
    for (int64_t i = 0; i < n; ++i) {
        const int32_t* r = gemms + i * 5;
        int32_t* o = out + i * 4;
        o[0] = o[1] = o[2] = o[3] = 0;
        if (r[0] == GK_NONE) continue;
        const GemmPlan g{r[0], r[1], r[2], r[3], r[4]};
        const SplitWant w = gemm_split_want(g);
        const SplitK k = gemm_splitk(g, (size_t)(g.side_ws ? ws_side : ws_main));
        o[0] = w.steps; o[1] = w.want; o[2] = k.steps_per_slice; o[3] = k.splits;
    }
}

// in [n][4]: steps, want, out_elems, ws_floats -> out [n][2]: steps per slice, splits
void twin_splitk_pick(int64_t n, const int64_t* in, int32_t* out) {
    for (int64_t i = 0; i < n; ++i) {
        const SplitK k = splitk_pick((int)in[4 * i], (int)in[4 * i + 1], (size_t)in[4 * i + 2], (size_t)in[4 * i + 3]);
        out[2 * i] = k.steps_per_slice; out[2 * i + 1] = k.splits;
    }
}

}  // extern "C"
