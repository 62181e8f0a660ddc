// az_net.h -- NNet::predict on the device (src/nnet.rs:35-45).
//
// Three nets answer a leaf batch: the reference's stub (examples/connect_four.rs:12-43),
// a deterministic test fixture, and the policy+value conv net of
// connect_four_net.py:20-95 as bf16 MFMA kernels (az_net.hip).
#pragma once
#include "az_tree.h"

namespace az {

struct ConvNet;        // weights of one model id, az_net.hip
struct NetWorkspace;   // activation workspace of one stream, az_net.hip

// offsets of the flat f32 parameter vector (the weights file)
struct Layout {
    int C;
    int64_t conv_w[4], conv_b[4], conv_bn[4], fc_w[2], fc_b[2], fc_bn[2], pi_w, pi_b, v_w, v_b, total;
    explicit Layout(int c) : C(c) {
        int64_t o = 0;
        for (int l = 0; l < 4; ++l) {
            int cin = l == 0 ? 2 : C;
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


struct NetProfile {          // filled when profiling is on; flops = what the matrix cores were asked to do (a layer that
    double conv2_ms = 0, conv2_flops = 0, total_ms = 0, total_flops = 0;   // runs as a table lookup contributes time, not flops)
    double conv3_ms = 0, conv3_flops = 0;
    double conv4_ms = 0, conv4_flops = 0;      // conv4 alone
    double fc_ms = 0, fc_flops = 0;            // fc1 + fc2 + heads
    double rows = 0;                           // executed rows of the timed forwards
    double conv2_bytes = 0;  // conv2 as a table: table rows gathered + activation rows written (algorithmic bytes)
    uint64_t launches = 0;
};

// pi = 1/7, v = +1 (kind 0) or the hash fixture (kind 1) for rows [0, *eb.n)
void launch_net_fixture(const EvalBatch& eb, int kind, uint64_t salt, hipStream_t s);

// weights of one model id
ConvNet* convnet_create(int channels, const char** err);
void convnet_destroy(ConvNet* n);
// activation workspace of one stream, shared by every model that runs on it
NetWorkspace* netws_create(int channels, int max_batch, const char** err);
void netws_destroy(NetWorkspace* ws);
int64_t convnet_param_count(int channels);
// raw f32 parameters (layout: DESIGN.md "weights file"); BN is folded and weights are
// rounded to bf16 on upload.
bool convnet_set_params(ConvNet* n, const float* host_params, int64_t count);
bool convnet_get_params(const ConvNet* n, float* host_params, int64_t count);
void convnet_init_random(ConvNet* n, uint64_t seed);
// fold finished profile records into *prof (call after the workspace's stream has been synchronised)
void netws_resolve_profile(NetWorkspace* ws, NetProfile* prof);
// k_conv3_auto's device-side accounting: adds (rows, working launches) since the last reset to out[2]; reset clears it
bool netws_conv3_accounting(NetWorkspace* ws, unsigned long long out[2], bool reset);
// Kernel-set switches of the conv net (az_set_option).  They live in the az_engine that was handed to az_set_option and are passed
// down with every forward: one engine's option never changes another engine's results.  The shipped library (built without
// -DAZ_DIAG) only honours conv2_table 0 / 1 and conv3_small 0 / 1; everything else selects superseded kernel generations, forced tiles
// or clock-stamp builds, which are compiled into libaz_engine_diag.so only (tools/).  No option value of either library computes a
// wrong answer: every diagnostic kernel is bit-identical to the shipped one of its layer.
struct NetOptions {
    int conv2_table = 1;    // 1: conv1 + conv2 as table gathers (k_conv2_table_x); 0: conv2 as the MFMA implicit GEMM (same function, other rounding)
    int conv3_small = 1;    // conv3 of a small expected batch on the 4-stage LDS-DMA ring (bit-identical)
    int conv3_planes = 1;   // conv3: the bank-conflict-free LDS image (Conv3Tables; bit-identical); 0 = image rows in order, 128 B each
    int ring_packed = 1;    // the LDS-DMA ring reads its weight stages from the model's packed copy (one stage = 16 KiB of consecutive bytes instead of
                            // 128 rows K * 2 bytes apart; conv4 -3 %; bit-identical); 0 = from the [N][K] weights
    int conv3_tail = 1;     // conv3: a short last round of workgroups is cut into half tiles (k_conv3_auto); 0 = full tiles only (bit-identical)
    int conv3_wreg = 1;     // conv3: the weight operand straight from global memory into registers in MFMA fragment order (k_conv3_auto_wreg; no
                            // weight tile in LDS, no barrier in the K loop; needs conv3_planes); 0 = the weight tile through LDS (k_conv3_auto; bit-identical)
    int net_fp8 = 0;        // 1: conv3 and conv4 on the fp8 (OCP e4m3) matrix path, a numerics class of its own (include/az_engine.h):
                            // conv2's table kernel writes e4m3, both convs run v_mfma_f32_16x16x128_f8f6f4 on the LDS-DMA ring or, for small batches
                            // ("narrow_rows"), on the register-fed skinny GEMM, bit-identically;
                            // needs conv2_table = 1 and the model's fp8 copies (convnet_build_fp8)
    int narrow_rows = 32;   // conv3 / conv4 / fc1 / fc2 of a batch of at most this many rows (x 2 for conv4, x 4 for the FCs) run as the register-fed
                            // skinny GEMM (k_gemm_skinny), decided on the device from the exact row count; 0 = never (bit-identical)
    // ---- diagnostic library only ----
    int gemm_variant = 5;   // 0 128x128 register-staged tiles everywhere; 1 / 2 256x256 LDS-DMA tiles; 3 conv2 image-resident, one 8-wave
                            // workgroup per CU; 5 the shipped set; 13 variant 2 with clock stamps (print_clock_stamps)
    int conv1_table = 1;    // conv2 as a GEMM gathers its image from the conv1 table (1) / runs k_conv1 into act1 (0)
    int conv2_pipe = 1;     // conv2 as a GEMM: k_conv_same_pipe (1) / round 1's k_conv_img2 (0)
    int conv3_pipe = 1;     // conv3: 1 the shipped choice; 2 k_conv_valid_pipe without interleaved fragment reads; 3 with them and per-segment clock
                            // stamps (print_seg_stamps); 0 round 1's kernel (k_conv_valid_img2)
    int conv3_ring = 0;     // force conv3 onto the ring (1 / 2: 128-row tiles with 2 / 4 stages, 3: device-picked tile)
    int conv4_big = 0;      // conv4 on the 256x256 kernel (1 always, 2 from 4096 rows)
    int fc_ring = 1;        // 1 ring with the tile picked on the device; 2 picked on the host; 3 plain 128-row ring; 0 register-staged tiles
    int ring_tile[6] = {0, 0, 0, 0, 0, 0};   // per layer: forced BM * 10 + NS
};
// diagnostic variant 13 only: per-block {shader cycles, 100 MHz ticks} of the conv2 K loop
bool netws_read_clock_stamps(NetWorkspace* ws, unsigned long long* out2048);
// diagnostic library's reader: conv3's output of the workspace's last forward, rows x [4][5][C] bf16 -> out; returns the bytes copied or -1
long long netws_read_conv3_out(NetWorkspace* ws, int rows, void* out);
#ifdef AZ_DIAG
// diagnostic library's reader: one layer's activations of the workspace's last forward, `rows` rows of bf16 -> out; returns the bytes
// copied or -1.  layer 1 act1 [8][9][C] (-1 if never allocated), 2 act2 [42][C], 3 act3 [20][C], 4 act4 [6][C], 5 fc1o [1024],
// 6 fc2o [512].  Under net_fp8, act2 and act3 hold e4m3 bytes: these bf16 readers are meaningless there (use the _fp8 readers).
long long netws_read_act(NetWorkspace* ws, int layer, int rows, void* out);
// diagnostic library only: rows [0, rows) of act2 .. fc2o filled with 0xFF bytes (NaNs in bf16 and e4m3) on stream s
bool netws_poison_acts(NetWorkspace* ws, int rows, hipStream_t s);
// diagnostic library's reader: rows [first_row, first_row + n_rows) of a model's conv1 table t1 (which = 1: [19683] rows of [C] bf16)
// or conv2 table u2 (which = 2: [19683 + 1] rows of [9][C] f16, the last one the appended zero row); the bytes copied or -1
long long convnet_read_conv_table(const ConvNet* n, int which, int first_row, int n_rows, void* out);
#endif
// "net_fp8": the e4m3 conv3 output of the workspace's last forward, rows x [4][5][C] bytes -> out (diagnostic library's reader)
long long netws_read_conv3_out_fp8(NetWorkspace* ws, int rows, void* out);
// ... and its e4m3 conv2 output, rows x [6][7][C] bytes
long long netws_read_conv2_out_fp8(NetWorkspace* ws, int rows, void* out);
// "net_fp8": k_gemm_skinny_f8 launches issued on the workspace since it was created (diagnostic library's reader)
unsigned long long netws_fp8_skinny_launches(const NetWorkspace* ws);
// "net_fp8": build the model's fp8 weight copies and scales for its current parameters (no-op when they are current): runs the
// calibration set through the bf16 conv2 / conv3 on stream s in workspace ws, synchronises, allocates on first use.  Never called
// by a forward.
bool convnet_build_fp8(ConvNet* n, NetWorkspace* ws, hipStream_t s);
// (sa2, sa3) of a model whose fp8 copies are current
bool convnet_fp8_scales(const ConvNet* n, float out[2]);
// allocate what a forward under `opt` may need later (conv1's haloed image for the kernel sets that run conv1 as a kernel), so that
// convnet_forward never allocates -- it may run inside a stream capture
bool convnet_prepare(NetWorkspace* ws, const NetOptions& opt);
// forward for rows [0, *eb.n) of model n in workspace ws; n_rows_hint = host-side upper bound used to size the grids.
// If prof != nullptr the forward and its conv2 launch are bracketed with HIP events (resolved later).
// n_rows_typ = expected row count (kernel / tile choice only; 0 = n_rows_hint).
void convnet_forward(ConvNet* n, NetWorkspace* ws, const EvalBatch& eb, int n_rows_hint, int n_rows_typ, hipStream_t s, NetProfile* prof,
                     const NetOptions& opt);

}  // namespace az
