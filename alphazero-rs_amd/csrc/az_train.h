// az_train.h -- NNet::train on the device (src/nnet.rs:38; recipe of connect_four_net.py:13-21, :102-151).
//
// f32 training of the policy+value net on the engine's flat parameter layout (az_net.hip `Layout`, the weights
// file): forward in BatchNorm training mode, softmax cross-entropy + mean squared error, backward, Adam.
// By default conv2..conv4's forward GEMMs run as f16 x 3 on the f16 matrix cores and every backward GEMM above conv1 as bf16 x 3 on the
// bf16 matrix cores (f32 accumulation), conv1 and the FC forwards on the f32 matrix cores (v_mfma_f32_16x16x4_f32); with "train_gemm" 0
// every GEMM runs there.  Which kernel chain a layer takes is decided once per step by train_step_plan (az_train_plan.h).  The column
// reductions are two-stage and every split-K sum is taken in slice order, so a step is deterministic run to run.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "az_train_plan.h"

namespace az {

struct Trainer;

struct TrainHyper {
    float lr = 1e-3f;            // connect_four_net.py:21
    float beta1 = 0.9f, beta2 = 0.999f, adam_eps = 1e-8f;
    float bn_momentum = 0.99f;   // tf.layers.batch_normalization default
    float bn_eps = 1e-3f;
    float dropout = 0.3f;        // connect_four_net.py:15
};

// The opt-in optimiser rules of one training session (az_optim.h; include/az_engine.h "train_weight_decay_e9" ...).  All off (the
// default): a step ends in the plain Adam kernel.
struct TrainOptim {
    float weight_decay = 0.0f;   // decoupled (torch.optim.AdamW), on the weight tensors only
    double clip_norm = 0.0;      // 0 = off; else torch.nn.utils.clip_grad_norm_ over the whole gradient
    int64_t warmup = 0;          // linear warm-up over that many applied steps
    int decay = 0;               // 0 none / 1 cosine / 2 linear, down to floor x lr at step `total`
    double floor = 0.0;
    int64_t total = 0;           // the step entries' horizon; trainer_set_lr_table's callers use their own
    float ema = 0.0f;            // 0 = off; else the decay of the averaged shadow weights
    bool on() const { return weight_decay > 0.0f || clip_norm > 0.0 || warmup > 0 || decay != 0 || ema > 0.0f; }
};

constexpr int TRAIN_MAX_BATCH = 256;

Trainer* trainer_create(int channels, const char** err);
void trainer_destroy(Trainer* t);
// host f32 parameters in weights-file order; resets the Adam moments and the step counter
bool trainer_set_params(Trainer* t, const float* host_params, int64_t count);
bool trainer_get_params(Trainer* t, float* host_params, int64_t count, hipStream_t s);
// the optimiser rules of the session trainer_set_params opened (which resets them to all-off); the shadow starts at the parameters
bool trainer_set_optim(Trainer* t, const TrainOptim& o);
// with the rules on: the schedule of a trainer_run_epoch sequence of `steps` steps in all (step i of it runs at entry i); synchronises
bool trainer_set_lr_table(Trainer* t, const TrainHyper& h, int64_t steps, hipStream_t s);
// the averaged weights (the moving averages are the live ones); false unless the session's rules have ema > 0
bool trainer_get_ema(Trainer* t, float* host_params, int64_t count, hipStream_t s);
// {gradient norm (-1 with clipping off), clip factor (1), learning rate, applied steps since trainer_set_params} of the last step
bool trainer_step_info(Trainer* t, double out[4], hipStream_t s);
// One optimisation step on a device-resident batch: boards [b][2][6][7], pis [b][7], vs [b] (f32).
// mask_seed keys the dropout masks of this step (hash of (mask_seed, layer, element): az_common.h dropout_keep).
// apply = false computes the loss and the gradients only.  The per-step losses are accumulated on the device
// (trainer_read_losses).  Returns false on a HIP error.
bool trainer_step(Trainer* t, const TrainHyper& h, const float* d_boards, const float* d_pis, const float* d_vs, int b,
                  uint64_t mask_seed, bool apply, hipStream_t s);
// sums of (loss_pi, loss_v) over the steps since the last call with reset = true; synchronises the stream
bool trainer_read_losses(Trainer* t, double out[2], bool reset, hipStream_t s);
// gradients of the last step, weights-file order (running-stat slots are 0)
bool trainer_get_grads(Trainer* t, float* host_grads, int64_t count, hipStream_t s);
// device scratch for the caller's batch: [TRAIN_MAX_BATCH] x (84 + 7 + 1) floats
float* trainer_batch_boards(Trainer* t);
float* trainer_batch_pis(Trainer* t);
float* trainer_batch_vs(Trainer* t);
// One epoch of `steps` optimisation steps on device-resident samples: step i trains on rows d_idx[i*b .. i*b+b) of
// (all_boards [n][84], all_pis [n][7], all_vs [n]); its dropout masks are keyed by mix64(seed_key ^ (gstep0 + i)).
// The launch sequence of a step is captured in a hipGraph and replayed.  Synchronises the stream.
bool trainer_run_epoch(Trainer* t, const TrainHyper& h, const float* all_boards, const float* all_pis, const float* all_vs,
                       const int64_t* d_idx, int64_t steps, int b, uint64_t seed_key, uint64_t gstep0, hipStream_t s);
// The same epoch for az_net_train_samples (az_draw.h): the rows come from `samples` -- feature planes, or 16-byte states whose planes
// are built per batch on the device -- and row k of the epoch is gathered mirrored where d_mir[k] != 0 (d_mir may be nullptr: none).
// Only the gather launch differs from trainer_run_epoch; an unmirrored row taken from boards gives the same floats.
struct TrainSamples {
    const float* boards;          // [n][84], or nullptr: states
    const ulonglong2* states;     // [n] (mine, theirs) bitboards of az_game.h
    const float* pis;             // [n][7]
    const float* vs;              // [n]
};
bool trainer_run_epoch_samples(Trainer* t, const TrainHyper& h, const TrainSamples& samples, const int64_t* d_idx, const uint8_t* d_mir,
                               int64_t steps, int b, uint64_t seed_key, uint64_t gstep0, hipStream_t s);
void trainer_set_graph(Trainer* t, bool on);      // A/B switch: replay a captured graph (default) or launch directly
// the seven route switches (az_train_plan.h), read by the next step.  The first call with fork on creates the second stream and its events
// on the current device; where that fails the fork stays off
void trainer_set_switches(Trainer* t, const TrainSwitches& sw);

// ---- the workspace reader of the per-kernel tests (tests/test_train_layers_gpu.py) ----------------------------------------------------
// Called by the diagnostic library's az_diag_train_* exports only (az_engine.hip under AZ_DIAG): nothing in the shipped library reaches
// these, so `keep` below is always off there and enqueue_step launches what it always launched.
// What a step leaves in the workspace, per layer l = 0..5 (conv1..conv4, fc1, fc2) or per step:
enum TrainDiagBuf {
    TRAIN_DIAG_Z = 0,         // z[l]       [rows of l][N_l]  pre-BatchNorm
    TRAIN_DIAG_A = 1,         // a[l]       [rows of l][N_l]  behind BatchNorm, ReLU and dropout
    TRAIN_DIAG_MEAN = 2,      // mean[l]    [N_l]
    TRAIN_DIAG_INVSTD = 3,    // invstd[l]  [N_l]
    TRAIN_DIAG_LOGITS = 4,    // [b][8]: the seven logits, then v
    TRAIN_DIAG_DHEAD = 5,     // [b][8]
    TRAIN_DIAG_LOSS = 6,      // [b][2]: the sample's (loss_pi, loss_v)
    TRAIN_DIAG_KEPT_DACT = 7, // d loss / d a[l] as it entered layer l's BatchNorm backward (kept steps only)
    TRAIN_DIAG_KEPT_DZ = 8,   // d loss / d z[l] as it left it (kept steps only)
};
// While keep is on, a trainer_step copies the two backward tensors above into buffers of their own, per layer, device to device on the
// step's stream (the scratch they live in is rewritten by the next layer).  trainer_run_epoch never keeps.  Refused (false) while the
// fork is on; the buffers are allocated by the first call that switches keep on.
bool trainer_diag_set_keep(Trainer* t, bool on);
// Copies buffer `what` of layer `layer` for the first `rows` samples of the last step to the host -> bytes copied, or -1 with nothing
// copied: no such buffer or layer, rows <= 0 or above the last step's batch, no step since trainer_set_params, a kept buffer when the
// last step kept nothing.
long long trainer_diag_read(Trainer* t, int what, int layer, int rows, void* out, hipStream_t s);
// The plan a step of batch b would follow under the trainer's switches, as train_plan_encode writes it -> the int32 count, or -1 (b outside
// 2 .. TRAIN_MAX_BATCH, cap below TRAIN_PLAN_INTS).  Host only: nothing is launched.
int trainer_diag_plan(Trainer* t, int b, int32_t* out, int cap);

}  // namespace az
