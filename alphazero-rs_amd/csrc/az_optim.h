// az_optim.h -- the opt-in rules of NNet::train's optimiser ("train_weight_decay_e9", "train_clip_norm_e6", "train_lr_warmup_steps",
// "train_lr_decay", "train_lr_floor_e6", "train_lr_total_steps", "train_ema_decay_e9"; include/az_engine.h): the learning-rate schedule,
// the gradient-norm clip factor and which parameters decay.  HIP-free apart from the host/device qualifier (AZO_HD, as az_noise.h has
// AZN_HD): the trainer's kernels, its host code and the g++ twin of the tests (tests/cpp/optim_twin.cpp) compile this text.
#pragma once
#include <cmath>
#include <cstdint>
#if defined(__HIPCC__)
#define AZO_HD __host__ __device__ __forceinline__
#else
#define AZO_HD inline
#endif

namespace az {

constexpr int64_t OPTIM_WD_E9_MAX = 1000000000, OPTIM_CLIP_E6_MAX = 1000000000000, OPTIM_STEPS_MAX = 2147483647, OPTIM_FLOOR_E6_MAX = 1000000,
                  OPTIM_EMA_E9_MAX = 999999999;
constexpr int OPTIM_DECAY_NONE = 0, OPTIM_DECAY_COSINE = 1, OPTIM_DECAY_LINEAR = 2;

// The f32 learning rate of applied step t (1-based, counted from az_net_train_begin): lr * warm * dec in double, rounded once.
//   warm = warmup > 0 ? min(1, t / warmup) : 1
//   dec  = 1 when mode == 0 or total == 0; else with x = clamp((t - warmup) / max(1, total - warmup), 0, 1)
//          cosine: floor + (1 - floor) * 0.5 * (1 + cos(pi x));  linear: floor + (1 - floor) * (1 - x)
// Only the host evaluates this (the device never calls cos): the value reaches the kernels through StepState (az_train.hip).
inline float optim_lr(float lr, int64_t t, int64_t warmup, int64_t total, int mode, double floor) {
    const double warm = warmup > 0 ? std::fmin(1.0, (double)t / (double)warmup) : 1.0;
    double dec = 1.0;
    if (mode != OPTIM_DECAY_NONE && total != 0) {
        const int64_t span = total - warmup > 1 ? total - warmup : 1;
        const double x = std::fmin(1.0, std::fmax(0.0, (double)(t - warmup) / (double)span));
        if (mode == OPTIM_DECAY_COSINE) dec = floor + (1.0 - floor) * (0.5 * (1.0 + std::cos(3.14159265358979323846 * x)));
        else dec = floor + (1.0 - floor) * (1.0 - x);
    }
    return (float)(((double)lr * warm) * dec);
}

// torch.nn.utils.clip_grad_norm_: the factor every gradient is multiplied by, min(1, c / (norm + 1e-6)) in double, rounded to f32.
// A non-finite norm propagates (NaN stays NaN, +inf gives 0), as in torch.
AZO_HD float optim_clip_scale(double norm, double c) {
    const double r = c / (norm + 1e-6);
    return (float)(r < 1.0 ? r : (r != r ? r : 1.0));
}

// The segments of the flat parameter vector in order (`Layout` of az_net.h, or any type with its fields): per conv / FC layer l
// 4 l + {0: weights, 1: the bias in front of BatchNorm, 2: gamma and beta, 3: the moving averages}, then 24 pi_w, 25 pi_b, 26 v_w, 27 v_b.
// Branch-free: one comparison per boundary.
template <class L>
AZO_HD int optim_segment(const L& y, int64_t i) {
    int s = 0;
    for (int l = 0; l < 4; ++l) {
        const int64_t n = l == 3 ? (int64_t)y.fc_w[0] - y.conv_bn[3] : (int64_t)y.conv_w[l + 1] - y.conv_bn[l];      // 4 x the layer's width
        s += (i >= y.conv_b[l]) + (i >= y.conv_bn[l]) + (i >= y.conv_bn[l] + n / 2) + (i >= y.conv_bn[l] + n);
    }
    for (int l = 0; l < 2; ++l) {
        const int64_t n = l == 1 ? (int64_t)y.pi_w - y.fc_bn[1] : (int64_t)y.fc_w[1] - y.fc_bn[0];
        s += (i >= y.fc_b[l]) + (i >= y.fc_bn[l]) + (i >= y.fc_bn[l] + n / 2) + (i >= y.fc_bn[l] + n);
    }
    return s + (i >= y.pi_b) + (i >= y.v_w) + (i >= y.v_b);
}
// weights decay (conv_w[0..3], fc_w[0..1], pi_w, v_w); biases, gamma, beta and the moving averages never do
AZO_HD bool optim_segment_decays(int s) { return s < 24 ? (s & 3) == 0 : (s & 1) == 0; }
// everything but the moving averages is the optimiser's
AZO_HD bool optim_segment_trainable(int s) { return s >= 24 || (s & 3) != 3; }
template <class L>
AZO_HD bool optim_decays(const L& layout, int64_t i) { return optim_segment_decays(optim_segment(layout, i)); }
template <class L>
AZO_HD bool optim_trainable(const L& layout, int64_t i) { return optim_segment_trainable(optim_segment(layout, i)); }

}  // namespace az
