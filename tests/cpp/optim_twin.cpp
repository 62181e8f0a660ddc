// g++ twin of csrc/az_optim.h (no HIP, no engine).  Prints, one record per line:
//   lr <warmup> <total> <mode> <floor_e6> <t> <f32 bits>      over the grid of tests/test_train_optim_cpu.py
//   clip <norm bits> <c bits> <f32 bits>                       norms below, at and above c, and non-finite ones
//   seg <C> <index> <decays> <trainable>                        both edges of every segment of the parameter layout
// With arguments `lr <lr_e9> <steps> <warmup> <total> <mode> <floor_e6>` it prints the f32 bits of that schedule's steps 1 .. steps instead
// (the GPU tests take their cosine table from here: the same libm as the engine's host code).
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "az_optim.h"

// az_net.h's Layout, restated: that header needs HIP.  tests/test_train_optim_cpu.py holds the indices below to net_ref.layout.
struct Layout {
    int C;
    int64_t conv_w[4], conv_b[4], conv_bn[4], fc_w[2], fc_b[2], fc_bn[2], pi_w, pi_b, v_w, v_b, total;
    explicit Layout(int c) : C(c) {
        int64_t o = 0;
        for (int l = 0; l < 4; ++l) {
            const int cin = l == 0 ? 2 : C;
            conv_w[l] = o; o += 9ll * cin * C;
            conv_b[l] = o; o += C;
            conv_bn[l] = o; o += 4ll * C;
        }
        const int fin[2] = {6 * C, 1024}, fout[2] = {1024, 512};
        for (int l = 0; l < 2; ++l) {
            fc_w[l] = o; o += (int64_t)fin[l] * fout[l];
            fc_b[l] = o; o += fout[l];
            fc_bn[l] = o; o += 4ll * fout[l];
        }
        pi_w = o; o += 512 * 7; pi_b = o; o += 7;
        v_w = o; o += 512; v_b = o; o += 1;
        total = o;
    }
};

static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
static uint64_t bits(double d) { uint64_t u; std::memcpy(&u, &d, 8); return u; }

int main(int argc, char** argv) {
    if (argc == 8 && !std::strcmp(argv[1], "lr")) {
        const float lr = (float)((double)std::atoll(argv[2]) * 1e-9);
        const int64_t steps = std::atoll(argv[3]), warmup = std::atoll(argv[4]), total = std::atoll(argv[5]);
        const int mode = std::atoi(argv[6]);
        const double floor = (double)std::atoll(argv[7]) / 1e6;
        for (int64_t t = 1; t <= steps; ++t) std::printf("%" PRIu32 "\n", bits(az::optim_lr(lr, t, warmup, total, mode, floor)));
        return 0;
    }
    const float lr = (float)(1000000.0 * 1e-9);
    const int64_t warmups[] = {0, 1, 7}, totals[] = {0, 1, 20, 5}, floors_e6[] = {0, 100000, 1000000};
    for (int64_t w : warmups)
        for (int64_t total : totals)
            for (int mode = 0; mode < 3; ++mode)
                for (int64_t f : floors_e6)
                    for (int64_t t = 1; t <= 26; ++t)
                        std::printf("lr %" PRId64 " %" PRId64 " %d %" PRId64 " %" PRId64 " %" PRIu32 "\n", w, total, mode, f, t,
                                    bits(az::optim_lr(lr, t, w, total, mode, (double)f / 1e6)));
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const double cs[] = {0.5, 1.0, 3.25, 1e6}, rel[] = {0.0, 1e-3, 0.5, 1.0 - 1e-9, 1.0, 1.0 + 1e-9, 1.5, 7.0, 1e9};
    for (double c : cs) {
        for (double r : rel) std::printf("clip %" PRIu64 " %" PRIu64 " %" PRIu32 "\n", bits(c * r), bits(c), bits(az::optim_clip_scale(c * r, c)));
        std::printf("clip %" PRIu64 " %" PRIu64 " %" PRIu32 "\n", bits(c - 1e-6), bits(c), bits(az::optim_clip_scale(c - 1e-6, c)));
        std::printf("clip %" PRIu64 " %" PRIu64 " %" PRIu32 "\n", bits(inf), bits(c), bits(az::optim_clip_scale(inf, c)));
        std::printf("clip %" PRIu64 " %" PRIu64 " %" PRIu32 "\n", bits(nan), bits(c), bits(az::optim_clip_scale(nan, c)));
    }
    for (int C : {128, 512}) {
        const Layout L(C);
        const int64_t starts[] = {L.conv_w[0], L.conv_b[0], L.conv_bn[0], L.conv_w[1], L.conv_b[1], L.conv_bn[1], L.conv_w[2], L.conv_b[2], L.conv_bn[2],
                                  L.conv_w[3], L.conv_b[3], L.conv_bn[3], L.fc_w[0], L.fc_b[0], L.fc_bn[0], L.fc_w[1], L.fc_b[1], L.fc_bn[1],
                                  L.pi_w, L.pi_b, L.v_w, L.v_b, L.total};
        for (int64_t s : starts)
            for (int64_t i : {s - 1, s})
                if (i >= 0 && i < L.total) std::printf("seg %d %" PRId64 " %d %d\n", C, i, (int)az::optim_decays(L, i), (int)az::optim_trainable(L, i));
        // inside a BatchNorm block: gamma | beta | moving mean | moving variance
        const int64_t bns[] = {L.conv_bn[0], L.conv_bn[1], L.conv_bn[2], L.conv_bn[3], L.fc_bn[0], L.fc_bn[1]};
        const int64_t widths[] = {C, C, C, C, 1024, 512};
        for (int k = 0; k < 6; ++k)
            for (int q = 1; q < 4; ++q)
                for (int64_t i : {bns[k] + q * widths[k] - 1, bns[k] + q * widths[k]})
                    std::printf("seg %d %" PRId64 " %d %d\n", C, i, (int)az::optim_decays(L, i), (int)az::optim_trainable(L, i));
    }
    return 0;
}
