// csrc/az_train_plan.h compiled alone by g++ and run as a stand-alone program under AddressSanitizer and UBSan
// (tests/test_train_plan_cpu.py): train_step_plan over every batch 2 .. 256, C in {128, 256, 384, 512}, all 128 switch combinations, the side
// stream present and absent; train_plan_encode into an exactly-sized buffer; the split-K of every GEMM each plan names.  Prints "ok".
// TEST INFRASTRUCTURE ONLY.  Build: g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I alphazero-rs_amd/csrc
#include <cstdio>
#include <vector>

#include "az_train_plan.h"

#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

int main() {
    using namespace az;
    const size_t ws_main = (size_t)96 << 20, ws_side = (size_t)16 << 20;      // trainer_create's two split-K workspaces
    std::vector<int32_t> flat((size_t)TRAIN_PLAN_INTS);
    long plans = 0, gemms = 0;
    for (int C = 128; C <= 512; C += 128)
        for (int m = 0; m < 256; ++m)
            for (int b = 2; b <= 256; ++b) {
                const TrainSwitches sw{m & 1, (m >> 1) & 1, (m >> 2) & 1, (m >> 3) & 1, (m >> 4) & 1, (m >> 5) & 1, (m >> 6) & 1};
                const bool side = (m >> 7) & 1;
                const StepPlan p = train_step_plan(sw, side, b, C);
                CHECK(train_plan_encode(p, flat.data(), TRAIN_PLAN_INTS - 1) == -1);
                CHECK(train_plan_encode(p, flat.data(), (int)flat.size()) == TRAIN_PLAN_INTS);
                CHECK(p.fork == (sw.gemm && sw.fork && side ? 1 : 0));
                ++plans;
                for (const LayerPlan& q : p.layer)
                    for (const GemmPlan* g : {&q.fwd_gemm, &q.wgrad_gemm, &q.dgrad_gemm}) {
                        if (g->kernel == GK_NONE) continue;
                        CHECK(g->M > 0 && g->N > 0 && g->K > 0 && (g->side_ws == 0 || p.fork));
                        const SplitWant w = gemm_split_want(*g);
                        const size_t ws = g->side_ws ? ws_side : ws_main, out = (size_t)g->M * (size_t)g->N;
                        const SplitK k = gemm_splitk(*g, ws);
                        CHECK(w.steps >= 1 && k.splits >= 1 && k.steps_per_slice >= 1);
                        CHECK(k.splits == 1 || (size_t)k.splits * out <= ws);
                        CHECK(k.splits * k.steps_per_slice >= w.steps && (k.splits - 1) * k.steps_per_slice < w.steps);
                        CHECK(w.want > 1 || k.splits == 1);
                        ++gemms;
                    }
            }
    CHECK(plans == 4L * 256 * 255 && gemms > 16 * plans);
    const SplitK one = splitk_pick(12, 0, 1000, 10), two = splitk_pick(13, 5, 100, 250);
    CHECK(one.splits == 1 && one.steps_per_slice == 12 && two.splits == 2 && two.steps_per_slice == 7);
    std::printf("ok\n");
    return 0;
}
