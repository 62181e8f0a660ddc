/* az_engine.h -- C ABI of the MI355X-native AlphaZero self-play engine.
 *
 * Drop-in boundary for the async_mcts + arena hot path of AnimatedRNG/alphazero-rs.
 * The reference has no FFI: its engine is reached through generic Rust traits
 * (`Game`, src/game.rs:10-28; `NNet`, src/nnet.rs:35-45) consumed by
 * `AsyncMcts<G>` (src/async_mcts.rs:14-115), whose callers are
 * `Coach::execute_episode` (src/coach.rs:104-157) and `arena::play_games`
 * (src/arena.rs:62-99).  The entry points below are what a Rust `extern "C"`
 * block would bind to keep `Coach`/`arena` and swap the engine; each cites the
 * reference item it replaces.  INTEGRATION.md shows the Rust-side binding.
 *
 * Conventions
 *   - Plain C types only; opaque handles; every output buffer is allocated and
 *     owned by the caller; inputs are borrowed for the duration of the call.
 *   - Every call returns an az_status (0 = ok).  The reference panics instead
 *     (unwrap/assert!); the panic sites map onto the status codes below.
 *   - A handle is used by one host thread at a time; calls are synchronous on
 *     return.  The one exception is a SHARED tree batch (az_tree_share): its
 *     slot calls (az_tree_slot_*) are made by many host threads at once, one
 *     thread per held slot; while any of them is in flight no other call may be
 *     made on the same engine (or on any of its trees), and az_tree_destroy comes
 *     only after every slot has been released.  One HIP stream per engine.  Engines on different devices may be
 *     driven from different host threads freely.  Two engines on the SAME device
 *     driven from two threads at once need "search_graph" 0 on both: while one
 *     thread captures its search loop as a hipGraph, HIP refuses the blocking
 *     copies of the other thread (hipErrorStreamCaptureImplicit, reported as
 *     AZ_ERR_HIP).  Measured gain of that arrangement: none (profiles/README.md).
 *     The same holds for training's captured step: such engines set "train_graph" 0 as well.
 *     A COLLECTIVE (az_comm_init with a local or an RCCL id, az_gather_samples, az_allreduce_u64, az_arena with
 *     allreduce_wld) blocks until every rank of the communicator has called it, so the ranks of an in-process
 *     communicator (az_comm_local_id) are driven by one host thread each; a rank that never arrives is waited for
 *     (there is no timeout, as with RCCL).
 *     az_arena overlaps its two models' searches on two HIP streams (the engine's own and a side stream that the engine creates
 *     at the first such call, shares with az_tournament and keeps until az_destroy); streams share the device's few hardware queues, so a
 *     process that keeps many other streams alive can make the two share one (measured: 2755 -> 1860 games/s with one extra
 *     idle stream).
 *   - Game state: Connect Four as two 7x6 bitboards in canonical form
 *     {mine, theirs} (side to move = mine); bit(col,row) = col*7 + row with
 *     row 0 = bottom; bit col*7+6 is always clear.
 *   - Feature tensors are NCHW [B,2,6,7] f32, plane 0 = side to move, plane 1 =
 *     opponent, row 0 = top (connect_four_game.rs:219-237 with repair S8).
 *   - Pointers may be host or device memory unless stated otherwise (the
 *     library copies with hipMemcpyDefault).
 */
#ifndef AZ_ENGINE_H
#define AZ_ENGINE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AZ_ACTIONS 7       /* connect_four_game.rs:14 */
#define AZ_FEATURES 84     /* 2*6*7, connect_four_game.rs:86-88 */
#define AZ_MAX_PLIES 42

typedef enum az_status {
    AZ_OK = 0,
    AZ_ERR_BAD_ARGUMENT = 1,   /* contract violations the reference asserts (src/async_mcts.rs:192, src/coach.rs:83) */
    AZ_ERR_CAPACITY = 2,       /* node arena exhausted: assert!(idx < buf.len()), src/node.rs:237 */
    AZ_ERR_HIP = 3,            /* HIP runtime / launch failure */
    AZ_ERR_INVALID_MOVE = 4,   /* arena validity assert, src/arena.rs:31-35 */
    AZ_ERR_TERMINAL_ROOT = 5,  /* get_action_prob on a finished game: p.unwrap() panic, src/async_mcts.rs:85 */
    AZ_ERR_NO_MODEL = 6,       /* model_id was never initialised / loaded */
    AZ_ERR_IO = 7,             /* checkpoint read/write */
    AZ_ERR_UNSUPPORTED = 8
} az_status;

/* Which network answers NNet::predict for a model id. */
typedef enum az_net_kind {
    AZ_NET_STUB = 0,   /* DumbConnectFourNnet, examples/connect_four.rs:12-43: pi = 1/7, v = +1 */
    AZ_NET_HASH = 1,   /* deterministic pseudo-random net (test fixture, exact in f32) */
    AZ_NET_CONV = 2    /* policy+value conv net, connect_four_net.py:20-95, bf16 MFMA */
} az_net_kind;

/* The numerics class of a conv model (az_net_set_class): the engine's "net_fp8" option decides (default), or the model is pinned. */
typedef enum { AZ_NET_CLASS_ENGINE = -1, AZ_NET_CLASS_BF16 = 0, AZ_NET_CLASS_FP8 = 1 } az_net_class;

typedef struct az_engine az_engine;
typedef struct az_tree az_tree;

typedef struct az_config {
    int32_t device;        /* HIP device ordinal */
    int32_t max_batch;     /* largest leaf batch the conv net is sized for (0 = 8192) */
    int32_t net_channels;  /* conv width; 0 = 512 (connect_four_net.py:21) */
    int32_t profile;       /* !=0: bracket the dominant kernels with HIP events (az_get_stats) */
    int32_t game;          /* az_game: which Game (src/game.rs:10-28) the trees play; 0 = Connect Four */
} az_config;

/* The Game the engine's trees are instantiated for (trait Game, src/game.rs:10-28; the device-side seam is
 * alphazero-rs_amd/csrc/az_game.h).  AZ_GAME_CONNECT_FOUR is the reference's one implementor
 * (examples/connect_four_lib/connect_four_game.rs); AZ_GAME_CONNECT_THREE is the same board, moves, features and nets with
 * three in a row winning: the seam's second instantiation (its CPU twin lives with the tests), there to prove the rules are a policy. */
typedef enum az_game { AZ_GAME_CONNECT_FOUR = 0, AZ_GAME_CONNECT_THREE = 1 } az_game;

/* Counters (SURVEY.md 8b "Introspection"); all cumulative since az_create / az_reset_stats. */
typedef struct az_stats {
    uint64_t games;          /* finished self-play / arena games */
    uint64_t moves;          /* get_action_prob calls */
    uint64_t simulations;    /* search_iteration calls, src/async_mcts.rs:219 */
    uint64_t expansions;     /* upgrade -> Some(true), src/node.rs:290-323 */
    uint64_t leaf_evals;     /* NNet::predict rows (root priors included) */
    uint64_t link_hits;      /* upgrade -> Some(false), src/node.rs:285-289 */
    uint64_t terminal_hits;  /* simulations that ended on an existing terminal node */
    uint64_t depth_sum;      /* best_child calls (selection levels) */
    uint64_t samples;        /* training tuples emitted (before symmetries) */
    uint64_t net_launches;   /* conv2 launches timed (profile mode) */
    double net_conv2_ms;     /* summed conv2 kernel time (profile mode) */
    double net_conv2_flops;  /* summed conv2 MFMA flops (profile mode); 0 while conv2 runs as a table lookup */
    double net_total_ms;     /* summed whole-forward time (profile mode) */
    double net_total_flops;  /* summed whole-forward flops of the layers that ran as arithmetic (profile mode) */
    double tree_ms;          /* summed select+backup kernel time (profile mode) */
    double tree_bytes;       /* summed algorithmic tree bytes, SURVEY.md 8d (profile mode) */
    double device_ms;        /* summed wall time spent inside engine calls */
    /* leaf de-duplication ("eval_dedup"): requested = rows the trees asked for (== leaf_evals), executed = rows the net
     * really ran (requested - cache hits - in-batch duplicates; == requested when de-duplication is off) */
    uint64_t leaf_rows_requested;
    uint64_t leaf_rows_executed;
    uint64_t eval_cache_hits;
    uint64_t eval_batch_dups;
    uint64_t eval_cache_inserts;
    double net_conv3_ms;           /* summed conv3 kernel time (profile mode) */
    double net_conv3_flops;        /* summed conv3 algorithmic flops (profile mode) */
    double net_conv2_bytes;        /* conv2 as a table ("conv2_table"): summed algorithmic bytes (table rows gathered + rows written) */
    uint64_t tree_launches;        /* select/backup launches (profile mode brackets every "profile_every"-th of them) */
    uint64_t tree_launches_timed;  /* ... of which tree_ms was measured on */
    uint64_t tree_arena_allocs;  /* tree arenas hipMalloc'ed by az_selfplay / az_arena since az_create (kept and reused across
                                  * calls of the same shape; not cleared by az_reset_stats) */
    double net_conv4_ms;           /* summed conv4 kernel time (profile mode) */
    double net_conv4_flops;
    double net_fc_ms;              /* summed fc1 + fc2 + heads kernel time (profile mode) */
    double net_fc_flops;
    double net_rows_timed;         /* executed rows of the timed forwards (profile mode) */
    uint64_t abandoned_sims;     /* num_threads > 1 only: simulations abandoned where the reference has no legal continuation
                                  * (every child Locked, src/node.rs:366-367; a link into a Locked node, :354); counted in `simulations` */
    uint64_t net_conv3_image_rows;      /* rows (boards) conv3 processed on the image-resident kernel k_conv3_auto, counted on the device ... */
    uint64_t net_conv3_image_launches;  /* ... and the launches of it that did that work (a launch that finds the batch on the small-batch
                                         * kernel's side of the hand-over exits at once and is not counted): what a profiler's average
                                         * duration of k_conv3_auto has to be divided into.  Always on (two atomics per launch). */
} az_stats;

/* ---- lifecycle ---------------------------------------------------------- */
az_status az_create(const az_config* cfg, az_engine** out);
/* Destroy every az_tree of the engine first: a tree borrows the engine's stream. */
void az_destroy(az_engine* e);
const char* az_last_error(const az_engine* e);
/* Tuning switches (no reference counterpart).  EVERY option is state of the engine it is set on: two engines in one process never
 * see each other's settings.  Unknown keys or values return AZ_ERR_BAD_ARGUMENT.  Keys of libaz_engine.so (each choice of a
 * bit-identical group computes the same bits; tests/test_net_gpu.py):
 *   the net  "conv2_table"  1 (default): conv1 + conv2 as nine gathered rows of a per-model table (conv2 is linear in conv1's output,
 *                           which is one of 3^9 table rows per position; 198 of the net's 329 MFLOP per leaf are never executed);
 *                           0: conv2 as the MFMA implicit GEMM -- the same function with its own rounding (each batch-independent and
 *                           within the stated tolerance of the fp32 reference)
 *                           Range of the table set: a table entry u (one tap's sum over the input channels of conv2's folded weight
 *                           times conv1's output, before the bias) is stored in f16 -- relative error 2^-11 for |u| >= 2^-14,
 *                           absolute 2^-25 below that, and |u| must stay below 65504.  The scale of conv1's activations alone does
 *                           not matter (conv1 x 2^k with conv2's weights x 2^-k leaves every u unchanged; held for k = -12 .. 12 by
 *                           tests/test_net_layers_gpu.py); a net whose per-tap conv2 sums leave that range wants "conv2_table" 0
 *            "conv3_small"  1 (default): conv3 of a small expected batch runs on the 4-stage LDS-DMA ring; 0: never.  Bit-identical
 *            "conv3_tail"   1 (default): a short last round of conv3 workgroups is cut into half tiles; 0: full tiles.  Bit-identical
 *            "conv3_planes" 1 (default): conv3's LDS image in the bank-conflict-free layout; 0: image rows in order.  Bit-identical
 *            "conv3_wreg"   1 (default): conv3's weight operand straight from global memory into registers (a fragment-ordered copy of the
 *                           model's weights, no weight tile in LDS, no barrier per K-step); 0: through LDS.  Bit-identical
 *            "ring_packed"  1 (default): the LDS-DMA ring kernels (conv4, fc1, fc2, small conv3) stream their weight stages from a packed
 *                           copy of the model (16 KiB of consecutive bytes per stage); 0: from the [N][K] weights.  Bit-identical
 *            "narrow_rows"  n (default 32, 0 = off): batches of at most n boards (conv3; 2n for conv4, 4n for the FCs) run the
 *                           register-fed skinny GEMM; the hand-over is decided on the device from the exact row count.  Bit-identical
 *            "net_fp8"      0 (default) / 1: conv3 and conv4 of every conv-net forward of this engine (search, self-play, arena,
 *                           az_net_predict*, shared tree batches) on the FP8 matrix path.  A NUMERICS CLASS of its own, not
 *                           bit-identical to bf16.  Nothing else changes: conv1 / conv2 stay table lookups, fc1 / fc2 / heads stay
 *                           bf16 / f32, the trainer and the weights file are untouched.  The contract:
 *                             format      OCP e4m3fn (not fnuz, not e5m2), round to nearest even, saturating at +-448
 *                             weights     BatchNorm folded in f32 as for bf16; per output channel n the scale
 *                                         sw[n] = 2^floor(log2(448 / max_k |w'[n][k]|)) (1 for an all-zero channel), q = e4m3(w' * sw[n])
 *                             activations one power-of-two scale per tensor, sa2 (conv2's output) and sa3 (conv3's output):
 *                                         s = 2^floor(log2(448 / (4 * amax))), amax = the tensor's maximum over the library's built-in
 *                                         calibration set (1024 legal positions at all plies from the counter RNG, a constant of the
 *                                         library) on the engine's own bf16 path, in chunks of at most max_batch -- a function of the
 *                                         weights alone, the same on every engine, rank and run; values are clamped to +-448 before the
 *                                         conversion, so a larger one saturates and never becomes NaN
 *                             arithmetic  products of two e4m3 values are exact; f32 accumulation inside v_mfma_f32_16x16x128_f8f6f4,
 *                                         K walked 128-channel block outer, tap inner; epilogue acc * (1 / (sw[n] * sa_in)) + bias[n]
 *                                         (the factor is an exact power of two), ReLU; conv3 then * sa3 -> clamp -> e4m3, conv4 -> bf16
 *                             invariants  a row's (pi, v) depends on its state alone (not on the batch size, its place in the batch or
 *                                         the tile the device picked), so de-duplication and the cache stay bit-exact; "conv3_small",
 *                                         "conv3_tail", "conv3_planes", "conv3_wreg", "narrow_rows" and "ring_packed" never change an fp8
 *                                         result (an fp8 model runs conv3 and conv4 on the LDS-DMA ring, or for small batches on the
 *                                         register-fed skinny GEMM, bit-identically)
 *                           Measured error (torch emulation, random nets, 200 legal positions, C = 512): max |dpi| 6.1e-3, |dv| 2.6e-2
 *                           against the textbook f32 net, ten times bf16's 5.9e-4 / 2.7e-3; insensitive to the activation scale (scales
 *                           64 x smaller move the result by 5e-4 / 5e-3).  The fp8 copies and scales are built when the option is
 *                           switched on and at every later weight upload (init, load, set_params, train end), never by a forward.
 *                           Changing the value gives every conv model a new evaluation-cache tag and generation: a persistent cache never
 *                           serves a row of the other class and no captured search graph of the other class is replayed.  Refused
 *                           (AZ_ERR_BAD_ARGUMENT) while a self-play session is open and while "conv2_table" is 0; "conv2_table" = 0 is
 *                           refused while "net_fp8" is 1 or any model's effective class is fp8.  The option is the class of every model
 *                           that az_net_set_class has not pinned
 *   root noise  "root_noise_eps_e6"   0 (default, OFF) .. 1000000: eps = (float)(value / 1e6) (the division in double, rounded once to f32)
 *            "root_noise_alpha_e6" 50000 .. 100000000 (default 1000000): alpha = (float)(value / 1e6)
 *                           DIRICHLET ROOT NOISE of AlphaZero self-play, strictly opt-in: with eps = 0 (set or never set) every output of
 *                           every entry is bit for bit what it is without the feature.  Values out of range and any change while a
 *                           self-play session is open are refused (AZ_ERR_BAD_ARGUMENT).  State of the engine, like every option.  The
 *                           contract (the sampler, operation by operation: csrc/az_noise.h):
 *                             where      every get_action_prob of az_selfplay, az_selfplay_begin / _next (lock-step and
 *                                        "selfplay_async", any num_sim_threads, with slot refill), az_tree_get_action_prob and
 *                                        az_tree_slot_get_action_prob.  NEVER az_arena: the gate is noise-free whatever the options say
 *                             when       once per get_action_prob, after the root has its stored prior (already there, or just stored from
 *                                        the root's own evaluation) and before the call's first selection
 *                             what       for each root child slot with action a, in place in the child record:
 *                                        prior <- (1 - eps) * prior + eps * eta[a]   (f32, round to nearest: 1 - eps, two products, one sum);
 *                                        no re-normalisation; invalid actions stay 0.  The change is PERMANENT: searching the same root
 *                                        again on the same stream mixes the same eta in again (cannot happen inside an episode: a
 *                                        position never recurs).  The evaluation cache, the leaf de-duplication and the eval log
 *                                        (record_evals) keep the raw net outputs
 *                             stream     eta is a function of (seed, game_id, ply = stones on the root board, alpha, valid-move mask)
 *                                        alone -- the triple of the tie-break stream; draw j of action a =
 *                                        rng_draw(seed, game_id, ply, 5 + 256 * a + 65536 * j); uniforms ((r >> 40) + 0.5) * 2^-24
 *                             sampler    eta[a] = g[a] / sum over the valid actions in ascending order, g[a] ~ Gamma(alpha) by
 *                                        Marsaglia-Tsang with polar normals (three draws per round, at most 32 rounds, then g = the
 *                                        shape), the u^(1/alpha) boost (draw 96) for alpha < 1, own polynomial log2 / exp2; a zero sum
 *                                        gives the uniform distribution over the valid moves.  Correctly rounded f32 only: host (g++
 *                                        -O2 -ffp-contract=off) and device builds of csrc/az_noise.h give the same bits
 *                           A captured search graph is keyed on the noise arguments, so one captured with others is never replayed.
 *                           az_root_noise_eta returns eta for given roots (what a host needs to reconstruct a recorded game's noise)
 *   playout cap "playout_cap_sims"  n: 0 (default, OFF), otherwise 1 .. 65535
 *            "playout_cap_full_e6" P: 0 .. 1000000 (default 250000)
 *                           PLAYOUT CAP RANDOMIZATION of self-play (KataGo), strictly opt-in: most moves of an episode are searched with
 *                           n simulations and are played but not recorded; a random share P / 1e6 of the moves gets the full budget
 *                           num_sims, gets root noise if that is on, and is recorded as a training tuple.  With n = 0 (set or never
 *                           set) every output and every counter of every entry is bit for bit what it is without the feature, whatever
 *                           P is.  Values out of range and any change while a self-play session is open are refused
 *                           (AZ_ERR_BAD_ARGUMENT); az_selfplay / az_selfplay_begin refuse n >= num_sims and n % num_sim_threads != 0.
 *                           State of the engine, like every option.  The contract (csrc/az_playout.h), for the
 *                           move of episode game_id at ply (= stones on the board: the triple of the tie-break and move streams):
 *                             mode       full = (rng_draw(seed, game_id, ply, 6) >> 40) < thresh24, thresh24 = (P * 2^24) / 1000000 in
 *                                        unsigned 64-bit arithmetic.  P = 1000000: every move is full and the output is bit for bit that
 *                                        of the feature off; P = 0: every move is fast and an episode emits no tuple (legal)
 *                             full move  exactly the move without the feature: num_sims simulations, root noise mixed in if
 *                                        "root_noise_eps_e6" > 0, tuple recorded
 *                             fast move  get_action_prob with n simulations on the episode's same persistent tree; no root noise (the
 *                                        root's stored prior is not touched); pi from the counts as always (temperature by ply, the
 *                                        tie-break stream unchanged); the move is sampled from pi with the unchanged move draw and goes
 *                                        into moves[] / game_len; NO tuple
 *                             samples    game-id order then ply order, full plies only: count = full plies x (2 if symmetries); z is
 *                                        the game's result from the recorded player's side as always.  az_stats.moves counts every ply,
 *                                        az_stats.samples the recorded ones, az_stats.simulations the budgets actually run
 *                             where      az_selfplay and sessions on every path (lock-step, "fused_search" 0 / 1, every "eval_dedup",
 *                                        num_sim_threads > 1, "selfplay_async", slot refill, both games, fp8 and "eval_mirror" models).
 *                                        NEVER az_arena, az_tree_* or the slot calls: they return what they return without the keys
 *                             eval log   record_evals keeps recording every predict of the episode, fast moves included
 *                             bounds     tree capacity, hash and cache sizes stay those of num_sims (an upper bound of any move)
 *                           A captured search graph is keyed on the playout-cap arguments, so one captured with others is never
 *                           replayed.  az_selfplay_get_full_plies returns which plies were full (to line tuples up with moves[])
 *   forced playouts "forced_playouts_k_e6"  0 (default, OFF) .. 16000000; k = (float)(value / 1e6): the division in double, rounded once
 *                           to f32 (KataGo's k = 2 is 2000000)
 *            "policy_prune" 0 (default) or 1; has an effect only while k > 0, inert with k = 0 whatever its value
 *                           FORCED PLAYOUTS at the root and POLICY TARGET PRUNING (KataGo, Wu 2019, section 3.2), strictly opt-in.  With
 *                           k = 0 (set or never set) every output and every counter of every entry is bit for bit what it is without the
 *                           feature, and the kernels that run are the ones that run without it.  Values out of range and any change
 *                           while a self-play session is open are refused (AZ_ERR_BAD_ARGUMENT).  State of the engine, like every
 *                           option.  The contract (csrc/az_forced.h):
 *                             forced moves  every get_action_prob that can carry root noise: az_selfplay and sessions on every path
 *                                        (lock-step, "selfplay_async", any num_sim_threads, slot refill, both games, fp8 and
 *                                        "eval_mirror" models), az_tree_get_action_prob, az_tree_slot_get_action_prob.  Under a playout
 *                                        cap the FULL moves only: a fast move is exactly the fast move without the keys.  NEVER az_arena.
 *                                        Independent of "root_noise_eps_e6": the root's stored priors are used as they are (the noised
 *                                        ones when noise is on)
 *                             selection  on a forced move, at the first level of a simulation only (the node is the call's root).  For
 *                                        root child slot j < nchild, with the values PUCT has loaded: cc_j the resolved counter,
 *                                        n_j = its visit count (in-flight visits included, as PUCT's N), p_j the stored prior:
 *                                          S = sum of n_j over the root's child slots (u32);  nf_j = sqrt((k * p_j) * (float)S), every
 *                                          operation f32 round-to-nearest, the square root correctly rounded;
 *                                          n_j > 0 && (float)n_j < nf_j:  u_j = +inf;  otherwise u_j is PUCT, unchanged.
 *                                        The arg-max runs over the u_j as always: last-max ties (among several forced children the highest
 *                                        slot wins), and with several simulations in flight the Locked filter and the two abandonment
 *                                        rules see these u_j.  No level below the root changes
 *                             pruning    on a forced move with "policy_prune" = 1, before pi is formed from the final counters:
 *                                        b = the slot with the largest n_j (the highest slot among equals); sq = sqrt(N_root + 1e-6);
 *                                        u* = PUCT of slot b.  For every slot j != b with n_j > 0:  f_j = (uint32_t)nf_j;
 *                                        lo_j = n_j > f_j ? n_j - f_j : 0;  m = n_j;
 *                                          while (m > lo_j && q_j + ((cpuct * p_j) * sq) / (float)m < u*) --m;
 *                                        (would the child, one visit fewer and its Q held fixed, still score below the best child?)
 *                                        If the loop lowered m and it ended at 1, m = 0: a child reduced to a single playout is pruned
 *                                        outright.  Slot b and slots with n_j = 0 keep their counts.  pi is computed from the pruned
 *                                        counts by the unchanged rules (temperature 0 and not 0, tie-break and move streams unchanged);
 *                                        that one pi is both recorded and sampled from.  The `counts` and `q` outputs stay RAW
 *                           A captured search graph is keyed on the forced-playout arguments, so one captured with others is never
 *                           replayed.  Playing strength with the option on is unmeasured
 *   Gumbel search "gumbel_m"  0 (default, OFF), otherwise 2 .. 7: the largest number of root actions considered
 *            "gumbel_c_visit_e6"  0 .. 1000000000 (default 50000000); c_visit = (float)(value / 1e6): the division in double, rounded once
 *            "gumbel_c_scale_e6"  1 .. 100000000 (default 1000000);  c_scale likewise.  The defaults are the paper's Go / chess setting;
 *                           q is used as stored, in [-1, 1]
 *                           GUMBEL ROOT SEARCH with SEQUENTIAL HALVING (Danihelka et al., ICLR 2022), strictly opt-in.  With m = 0 (set or
 *                           never set) every output and every counter of every entry is bit for bit what it is without the feature, and
 *                           the kernels that run are the ones that run without it.  Values out of range and any change while a self-play
 *                           session is open are refused (AZ_ERR_BAD_ARGUMENT).  State of the engine, like every option.  While m > 0,
 *                           az_selfplay, az_selfplay_begin and az_tree_get_action_prob refuse (AZ_ERR_BAD_ARGUMENT) num_sim_threads > 1,
 *                           "selfplay_async" = 1 and "forced_playouts_k_e6" > 0 (both features claim the root's arg-max).  The contract
 *                           (csrc/az_gumbel.h states every formula operation by operation):
 *                             Gumbel moves  every get_action_prob that can carry root noise, on az_selfplay and sessions in lock-step
 *                                        ("fused_search" 0 / 1, every "eval_dedup", slot refill, both games, fp8 and "eval_mirror"
 *                                        models) and on az_tree_get_action_prob.  Under a playout cap the FULL moves only: a fast move is
 *                                        exactly the fast move without the keys.  NEVER az_arena or the slot calls.  Independent of
 *                                        "root_noise_eps_e6": the root's stored priors are used as they are
 *                             baseline   once per Gumbel move, where root noise is mixed in: base_j = the resolved visit count of root
 *                                        child slot j.  d_j = n_j - base_j is the slot's visits in THIS call, t = sum of d_j the index of
 *                                        the current simulation within the move
 *                             variate    g_j = -ln(-ln(U)), U = ((float)(r >> 41) + 0.5f) * 2^-23, r = rng_draw(seed, game_id, ply,
 *                                        8 + 256 * a_j) on the triple of the tie-break stream; every g_j = 0 when the move's temperature
 *                                        is 0 (self-play: ply + 1 >= temp_threshold; the tree call: temp == 0)
 *                             selection  at the first level of a simulation only: l_j = ln(max(p_j, 2^-126));
 *                                        v_mix = sum_{n_b>0} p_b q_b / sum_{n_b>0} p_b (0 when no slot is visited); qh_j = n_j > 0 ? q_j :
 *                                        v_mix;  sigma_j = ((c_visit + (float)max_b n_b) * c_scale) * qh_j;  s_j = (g_j + l_j) + sigma_j.
 *                                        The arg-max (last-max ties, as always) runs over the slots with d_j == c(t), where c(t) is
 *                                        entry t of sequential halving's considered-visit sequence for min(m, nchild) actions and the
 *                                        move's budget (num_sims; of a full move).  PUCT does not decide at the root; no level below
 *                                        the root changes
 *                             result     the SELECTED ACTION is the arg-max of s_j over the slots with the largest d_j; self-play plays
 *                                        it (the move draw is not used) and records it in moves[].  pi = softmax(l_j + sigma_j) over
 *                                        the root's slots, 0 for invalid actions; temperature does not enter.  The `counts` and `q`
 *                                        outputs stay RAW
 *                           The value mix is the paper's in its limit of many visits, WITHOUT the net's raw root value: a root reused
 *                           from an earlier move's tree no longer has its own net value (a deliberate deviation).  A captured search
 *                           graph is keyed on the Gumbel arguments, so one captured with others is never replayed.
 *                           az_tree_get_selected returns the selected actions of the last tree call, az_gumbel_values the variates of
 *                           given roots.  Playing strength with the option on is unmeasured
 *   arena openings "arena_opening_plies"  0 (default, OFF) or an even value 2 .. 12; odd, negative and larger values are refused
 *                           (AZ_ERR_BAD_ARGUMENT).  State of the engine, like every option; only az_arena reads it.
 *                           PAIRED OPENINGS, strictly opt-in: with plies 0 and no opening book (az_arena_set_opening_book) every output
 *                           of every entry is bit for bit what it is without the feature.  The arena searches at temperature 0 and a
 *                           net is a function of the state, so from one position all games of a seating are the same game; with
 *                           openings on, game g of an arena of `total` games (GLOBAL index) and its seat-swapped twin g + total/2
 *                           start from the same position, which differs from pair to pair: the opening's bias cancels inside the pair
 *                           and the tally is over total/2 different games.  The rule (csrc/az_opening.h):
 *                             pair       half = total / 2;  game g belongs to pair p = g % half
 *                             base       book[p % nb] while a book of nb entries is set; else start_board when use_start_board is
 *                                        set; else the initial board.  A book together with use_start_board is refused
 *                             plies      for j = 0 .. n-1, s the current canonical state:
 *                                          C1 = the legal actions a, ascending, behind which the game goes on;
 *                                          C2 = those of C1 after which the next mover has no immediately winning reply;
 *                                          C = C2 if it is not empty, else C1; if C is empty, stop;
 *                                          a = C[rng_choose(rng_draw(seed, p, j, 7), |C|)] (7 = RNG_OPENING; seed = the call's seed)
 *                             used       the longest EVEN prefix of what was played (an odd last ply is dropped): the first seat is
 *                                        to move and the position is {first seat's stones, second seat's stones}, a start_board; it
 *                                        is never finished
 *                             contract   game g is bit for bit (result, move record, eval log) the game of the sharded single-game call
 *                                        {total_games = total, first_game = g, num_games = 1, use_start_board = 1, start_board = the
 *                                        opening of g} with the feature off.  So shards add up to the unsharded arena, and
 *                                        allreduce_wld, record_evals, num_sim_threads, both games, fp8 and "eval_mirror" models behave
 *                                        as they do from a start_board: the tie-break stream stays (seed, global game, ply = stones on
 *                                        the board), tree, hash and cache bounds stay those of a 42-ply game, az_arena_get_moves and
 *                                        az_stats hold only the plies the models played (an opening ply adds to no counter), and a
 *                                        finished start_board takes the early return it takes without the option
 *                           The openings are drawn on the device by one small kernel per az_arena call.  Whether paired openings change
 *                           which candidates a gate accepts is unmeasured
 *   search   "search_graph" n (default 20, even, 0 = off): n simulation steps per captured hipGraph replay (conv nets) ...
 *            "search_graph_rows" n (default 1024): ... for searches whose expected leaf batch has at most n rows (the arena, the drain
 *                           of a self-play call, single trees: there the host's launch calls set the pace; on big batches the kernels do)
 *            "fused_search" 1 (default): the stub / hash nets run a whole search in one launch; 0: one launch per simulation
 *            "selfplay_async" 0 (default) / 1: az_selfplay with FREE-RUNNING slots -- every slot runs backup, move, next root and select on
 *                           its own timeline inside the tree kernel, "selfplay_async_launches" (default 2) launches share one leaf batch
 *                           (trees the cache answered go on, trees that took a row wait for the forward), at most
 *                           "selfplay_async_iters" (default 6) stages per slot and launch.  Same games bit for bit (a game depends on
 *                           its seed, its id and the net's rows, never on the schedule); fewer, larger forwards
 *            "tree_block4"  1 (default): four waves per workgroup in the select / backup kernel; 0: one
 *   leaf de-duplication (bit-exact: a row's (pi, v) depends on its state alone; the reference's per-tree analogue is `seen`,
 *   src/node.rs:282-289)
 *            "eval_dedup"   0 off / 1 conv nets (default) / 2 every net: each distinct state of a leaf batch is evaluated once
 *            "eval_mirror"  0 (default) / 1: mirror-canonical leaf evaluation, a numerics class of its own like "net_fp8".  The board is
 *                           left-right symmetric, a conv net is not mirror-equivariant.  With 1 every forward of a CONV model of this
 *                           engine (search, self-play, sessions, the arena, shared tree batches, az_net_predict*) answers with F
 *                           instead of the raw net N:
 *                             c(s)       = s or mirror(s), whichever has the smaller Game::pack word as an unsigned 64-bit integer; on
 *                                          equal words (a self-symmetric position, the empty board included) s itself, "not mirrored"
 *                             F(s).v     = N(c(s)).v
 *                             F(s).pi[a] = N(c(s)).pi[a] when s is not mirrored, N(c(s)).pi[mirror_action(a)] when it is
 *                           Nothing else is touched: masking, renormalisation, root noise and the stored priors run on F(s) exactly as
 *                           they run on N(s) with 0.  Bit for bit, F(mirror(s)).pi is F(s).pi reversed and v is equal.
 *                           The leaf batch, the election table and the evaluation cache carry c(s) and the RAW N(c(s)): a position and
 *                           its mirror image share one row and one cache entry.  The eval log (record_evals, az_*_get_evals) carries
 *                           the tree's own s with F(s), so replay parity against an unchanged reference keeps working.
 *                           F depends on the state alone: not on "eval_dedup", the cache, the batch, the schedule (lock-step,
 *                           "selfplay_async", sessions, num_sim_threads, shared batches) or any bit-identical kernel option.  It
 *                           composes with the fp8 class (canonicalisation happens before featurisation) and is the same for both
 *                           games.  Stub and hash models are never affected, on any path (fused search, launch per simulation,
 *                           "eval_dedup" = 2).  Refused (AZ_ERR_BAD_ARGUMENT) while a self-play session is open and for other values.
 *                           A real change gives every conv model a new cache tag and generation: no cached row and no captured search
 *                           graph of the other class is ever reused.  With 0 every output and counter is bit for bit what it was
 *            "eval_cache_log2"  upper bound of log2 entries of the engine's evaluation cache (default 30, 0 = none, 10..30; 40 bytes per
 *                           entry).  A call (or session) allocates and clears only what ITS games can fill (4 x its bound on
 *                           inserted rows, at least 2^10): a 1-tree, 25-simulation call touches 40 KB, a call of 8192 episodes
 *                           11 GB, and only bench-sized ones (65536 episodes and more) the full 43 GB -- a seventh of the
 *                           device's 288 GB, and worth it: a self-play session of 1.6 M episodes runs at 10.6 k games/s with
 *                           2^30 entries and at 7.9 k with 2^27, whose table is full after a fifth of it
 *            "eval_cache_max_stones"  only states with at most that many stones are cached (default 42)
 *            "eval_cache_persist"  0 (default): every az_selfplay / az_arena / az_tree_get_action_prob call starts from an empty cache;
 *                           1: entries live until the model's weights change (the full "eval_cache_log2" table)
 *            "dedup_stats"  1 (default) / 0: maintain the five leaf-row counters of az_stats
 *   profile  "profile"      0 / 1: the HIP-event brackets of az_config.profile, switched between calls (bracketed searches launch every
 *                           kernel on its own; a timed region runs with them off, a separate pass with them on gives the kernel times)
 *            "profile_every" n (default 1): with the brackets on, bracket every n-th simulation step (the net_* and tree_ms sums
 *                           then cover that sample of launches; a bracket costs a little idle time between kernels)
 *   NNet::train  "train_epochs" (10), "train_batch" (64, <= 256), "train_seed" (0), "train_lr_e9" (1000000 = 1e-3),
 *            "train_dropout_e6" (300000 = 0.3), "train_graph" 1 (default) / 0: replay a step's launches as a captured hipGraph,
 *            "train_gemm" 1 (default): dgrad / wgrad as bf16 x 3 on the bf16 matrix cores (gradients within 1e-5 of float64
 *                           autograd), 0: every GEMM on v_mfma_f32_16x16x4_f32 (1e-6).  Two numerics classes: the trained
 *                           weights differ, as they do between two f32 summation orders (parity of NNet::train is unpinned by
 *                           the reference, whose training script cannot run; tests/test_train_gpu.py bounds the drift),
 *            "train_fwd_x3" 1 (default): the forward GEMMs of conv2..conv4 as f16 x 3 on the f16 matrix cores (activations x 64 and
 *                           weights x 256 split into half-precision hi / lo pairs, three products, f32 accumulate: 2^-22, the grade of
 *                           the f32 kernel's own accumulation -- gradients stay within 1e-5 of float64 autograd), 0: on
 *                           v_mfma_f32_16x16x4_f32; "train_gemm3_ring" 1 (default) / 0: the big x 3 GEMMs on the 256 x 128 ring kernel,
 *            "train_wgrad_tr" 1 (default) / 0: conv wgrad from the operands as stored, transposed LDS reads (k_wgrad3_tr) instead of
 *                           transpose kernels + k_gemm3; "train_implicit" 1 (default) / 0: conv2..conv4's GEMMs gather their A rows from
 *                           the activations instead of reading im2col matrices (needs batch % 16 == 0 and net_channels % 256 == 0,
 *                           else the im2col path runs); every combination is held to the same bars by tests/test_train_gpu.py,
 *            "train_fork" 0 (default) / 1: with "train_gemm" 1, a step's weight split and wgrad chains run on a second stream
 *                           branch beside the BatchNorm-backward / dgrad chain (bit-identical; measured no faster, so off),
 *            "train_fwd_dma" 1 (default): the forward GEMMs' tiles go global -> LDS by LDS-DMA (k_gemm_f32_dma), 0: register-staged
 *   optimiser rules  seven keys, all 0 (OFF) by default, strictly opt-in (csrc/az_optim.h states every formula):
 *            "train_weight_decay_e9"  0 .. 1000000000; wd = (float)(value / 1e9).  Decoupled decay as torch.optim.AdamW
 *            "train_clip_norm_e6"     0 (off) or 1 .. 1000000000000; c = value / 1e6.  torch.nn.utils.clip_grad_norm_ over the whole gradient
 *            "train_lr_warmup_steps"  0 .. 2147483647: linear warm-up over that many applied steps
 *            "train_lr_decay"         0 none / 1 cosine / 2 linear, from the end of the warm-up down to floor x lr at step `total`
 *            "train_lr_floor_e6"      0 .. 1000000; floor = value / 1e6
 *            "train_lr_total_steps"   0 (no decay) .. 2147483647: `total` for az_net_train_step sessions; az_net_train always uses its
 *                                     own epochs x (n / batch)
 *            "train_ema_decay_e9"     0 (off) or 1 .. 999999999; d = (float)(value / 1e9): an averaged shadow of the weights (az_net_train_ema)
 *                           on         az_net_train_begin (and so az_net_train) reads the seven keys; they hold for that session, whatever is
 *                                      set later.  With any of them on, a step's update runs in ONE other kernel (k_adamw) instead of the
 *                                      Adam kernel, behind one more launch (k_grad_sqnorm) when clipping is on
 *                           where      per applied step t = 1, 2, .. since az_net_train_begin, g the step's gradient:
 *                                        lr_t  = (float)(lr * warm * dec) in double, lr = "train_lr_e9":  warm = warmup > 0 ? min(1, t / warmup)
 *                                                : 1;  dec = 1 when decay = 0 or total = 0, else with x = clamp((t - warmup) / max(1, total -
 *                                                warmup), 0, 1): cosine floor + (1 - floor) * 0.5 * (1 + cos(pi x)), linear floor + (1 - floor)
 *                                                * (1 - x).  Evaluated on the host for both entries
 *                                        scale = clipping on ? (float)min(1, c / (|g| + 1e-6)) : 1, |g| = sqrt of the f64 sum of squares of
 *                                                the whole gradient (fixed chunks, fixed order: the same bits run to run, captured graph or
 *                                                not, "train_fork" 0 / 1); a non-finite norm propagates
 *                                        g' = g * scale;  m, v advance with g' as always
 *                                        p  = p * (1 - lr_t * wd) for every element of the conv, FC, pi and v WEIGHT tensors; biases,
 *                                                BatchNorm gamma / beta and the moving averages never decay
 *                                        p  = p - (lr_t / bc1) * m / (sqrt(v) / sqrt(bc2) + eps)
 *                                        s  = d * s + (1 - d) * p for every parameter but the moving averages; s starts at the weights
 *                                                az_net_train_begin loaded (no de-biasing); a step with apply = 0 does not move it
 *                                      grads_out stays the RAW gradient g.  az_net_train_ema stores the shadow, az_net_train_step_info
 *                                      reports |g|, scale, lr_t and t of the last step
 *                           refused    values outside the ranges above (AZ_ERR_BAD_ARGUMENT, nothing changes)
 *                           purity     with all seven at 0 (set or never set) the trainer launches the kernels it launches without the
 *                                      feature and every weight is bit for bit what it is without it; an engine whose keys were on and are
 *                                      back at 0 trains the same bits as one that never touched them.  Clipping with a c no step reaches
 *                                      (scale exactly 1) is bit-identical to clipping off.  State of the engine, like every option.
 *                                      Playing strength with any of the keys on is unmeasured
 * libaz_engine_diag.so (the same sources built with -DAZ_DIAG; alphazero-rs_amd/build.py) additionally takes the keys of the
 * SUPERSEDED kernel generations and the clock-stamp builds -- "gemm_variant" (0, 1, 2, 3, 5; 13: clock stamps), "fc_ring", "ring_tile",
 * "conv3_ring", "conv2_pipe", "conv3_pipe" (0 .. 3), "conv1_table", "conv4_big", "conv2_table" = 2, "tree_stamps", "print_*" -- which the
 * shipped library refuses (it accepts their default values, so a host may set them unconditionally); csrc/az_net.hip,
 * csrc/az_net_diag.inc.  No value of any key, in either library, computes a wrong answer. */
az_status az_set_option(az_engine* e, const char* key, int64_t value);
az_status az_get_stats(az_engine* e, az_stats* out);
az_status az_reset_stats(az_engine* e);

/* ---- NNet trait, src/nnet.rs:35-45 -------------------------------------- */
/* NNet::new for the stub / hash nets (no weights). salt only matters for AZ_NET_HASH. */
az_status az_net_set_kind(az_engine* e, int32_t model_id, az_net_kind kind, uint64_t salt);
/* Drop a model id and its device memory (weights + conv1 table, 41 MB at C = 512).  The reference never frees a model:
 * its Python side keeps one checkpoint per id on disk (src/nnet.rs:36); a long Coach::learn run (src/coach.rs:296-390: a new
 * id per accepted iteration) calls this for the superseded id.  The activation workspace is per stream, not per model. */
az_status az_net_free(az_engine* e, int32_t model_id);
/* NNet::new with random init: Glorot-uniform kernels, zero bias, BN gamma=1 beta=0 mean=0 var=1 eps=1e-3. */
az_status az_net_init_random(az_engine* e, int32_t model_id, uint64_t seed);
/* NNet::new(checkpoint) / save: flat f32 file, layout in DESIGN.md "weights file". */
az_status az_net_load(az_engine* e, int32_t model_id, const char* path);
az_status az_net_save(az_engine* e, int32_t model_id, const char* path);
/* The numerics class of ONE model.  AZ_NET_CLASS_ENGINE (every id's default) follows the engine's "net_fp8" option; BF16 and FP8 pin
 * the model whatever the option says, so one engine can seat a net against its own fp8 copy in az_arena, or play self-play in fp8
 * and the gate in bf16.  The class is state of the model id: it survives weight uploads into the id (az_net_init_random, _load,
 * _set_params, az_net_train* ending in it), az_net_free drops it, a fresh id starts at ENGINE.  Every forward of the model (search,
 * self-play, arena, az_net_predict*, shared tree batches) runs in its EFFECTIVE class (0 bf16 / 1 fp8).  A call that changes the
 * effective class gives this model, and no other, a new evaluation-cache tag and generation (no cached row and no captured search
 * graph of the other class is used again) and, towards fp8, builds its fp8 copies and scales -- never a forward does; a call
 * that leaves the effective class as it is keeps the tag.  AZ_ERR_BAD_ARGUMENT: an unknown id, a stub / hash model, FP8 while
 * "conv2_table" is 0, any change while a self-play session is open. */
az_status az_net_set_class(az_engine* e, int32_t model_id, int32_t net_class /* an az_net_class */);
/* stored = what was set (an az_net_class), effective = 0 (bf16) or 1 (fp8); either may be NULL. */
az_status az_net_get_class(az_engine* e, int32_t model_id, int32_t* stored, int32_t* effective);
/* Raw f32 parameter exchange (same order as the weights file); count from az_net_param_count. */
int64_t az_net_param_count(const az_engine* e);
az_status az_net_set_params(az_engine* e, int32_t model_id, const float* params, int64_t n);
az_status az_net_get_params(az_engine* e, int32_t model_id, float* params, int64_t n);
/* NNet::predict(board [B,2,6,7], model_id) -> (pi [B,7], v [B]), src/nnet.rs:40-44 */
az_status az_net_predict(az_engine* e, int32_t model_id, const float* boards, int32_t B, float* pi, float* v);
/* Same on canonical bitboards [B,2] (what the search feeds the net). */
az_status az_net_predict_states(az_engine* e, int32_t model_id, const uint64_t* states, int32_t B, float* pi, float* v);
/* NNet::train(examples, previous_model_id, model_id), src/nnet.rs:38: start from the weights of prev_id, run the
 * reference's recipe on the device (connect_four_net.py:13-21, :102-151: loss = softmax cross-entropy(pi) + mean
 * squared error(v), Adam, BatchNorm in training mode, dropout on the two FC layers; epochs x (n / batch) steps on
 * batches drawn with replacement), store the result under id. boards [n,2,6,7], pis [n,7], vs [n] f32, host or
 * device. f32 parameters, activations, gradients and optimiser state; the forward GEMMs on the f32 matrix cores, dgrad / wgrad as
 * bf16 x 3 with f32 accumulation ("train_gemm"; csrc/az_train.hip). Hyper-parameters through
 * az_set_option: "train_epochs" (10), "train_batch" (64, <= 256), "train_seed" (0), "train_lr_e9" (1000000 = 1e-3),
 * "train_dropout_e6" (300000 = 0.3). Batches and dropout masks come from the build's counter RNG (B7). */
az_status az_net_train(az_engine* e, int32_t prev_id, int32_t id, const float* boards, const float* pis,
                       const float* vs, int64_t n);
/* (loss_pi, loss_v) averaged over each epoch of the last az_net_train: writes min(epochs, cap_epochs) pairs to out
 * (may be NULL) and returns the number of epochs. */
int32_t az_net_train_history(const az_engine* e, float* out, int32_t cap_epochs);
/* Fine-grained parity entries (what az_net_train is made of). begin: load prev_id's weights, zero the Adam moments.
 * step: ONE optimisation step on an explicit batch (2 <= b <= 256); mask_seed keys this step's dropout masks;
 * apply = 0 leaves the weights alone (loss and gradients only, BatchNorm moving averages still advance);
 * loss_out[2] = (loss_pi, loss_v), grads_out[az_net_param_count] = d loss / d parameter in weights-file order
 * (both may be NULL). end: store the weights under model_id. */
az_status az_net_train_begin(az_engine* e, int32_t prev_id);
az_status az_net_train_step(az_engine* e, const float* boards, const float* pis, const float* vs, int32_t b,
                            uint64_t mask_seed, int32_t apply, float* loss_out, float* grads_out);
az_status az_net_train_end(az_engine* e, int32_t model_id);
/* The averaged weights of "train_ema_decay_e9" as a model: every parameter is the shadow s, the BatchNorm moving averages are the live
 * trainer's.  Valid after an az_net_train_begin that saw the key > 0 -- between begin and end, after end, after az_net_train -- until
 * the next az_net_train_begin; AZ_ERR_BAD_ARGUMENT otherwise (no training yet, a session with the key at 0).  Stores like
 * az_net_set_params (the id's class is kept, its cached rows are dropped). */
az_status az_net_train_ema(az_engine* e, int32_t model_id);
/* out = {|g| of the last step (-1 with clipping off), its clip factor (1 with clipping off), its lr_t, applied steps since
 * az_net_train_begin}; after az_net_train: of its last step.  AZ_ERR_BAD_ARGUMENT before any az_net_train_begin. */
az_status az_net_train_step_info(const az_engine* e, double out[4]);

/* ---- AsyncMcts, src/async_mcts.rs:14-115 -------------------------------- */
/* n_games independent AsyncMcts::default(reserve, num_sims, num_threads, max_depth, model_id, cpuct, ..)
 * (src/async_mcts.rs:27-48), each rooted at the initial board (NodeStore::new, src/node.rs:156-166).
 * num_threads = simulations in flight per tree (src/async_mcts.rs:191-217; num_sims % num_threads == 0, :192).
 * 1 is the reference's only deterministic mode.  num_threads > 1 runs the reference's tree-parallel search as a
 * deterministic LOCK-STEP schedule (one legal execution of the racy original; DESIGN.md "several simulations in flight"):
 * per step the threads select in thread order, each seeing the visits and virtual losses (src/node.rs:77-80) of the earlier
 * ones and the `Locked` filter of src/node.rs:359-365 on leaves they hold; the step's leaves are evaluated together and
 * backed up in thread order.  At most 8 threads. */
az_status az_tree_create(az_engine* e, int32_t n_games, uint64_t reserve, int32_t num_sims, int32_t num_threads,
                         int32_t max_depth, int32_t model_id, int32_t cpuct, az_tree** out);
void az_tree_destroy(az_tree* t);
/* AsyncMcts::from_state(s, ..) (src/async_mcts.rs:50-72, NodeStore::from_root, src/node.rs:168-177): forget every
 * tree of the batch and root tree g at root_states[g] (canonical bitboards [G,2]); NULL = the initial board. */
az_status az_tree_reset(az_tree* t, const uint64_t* root_states);
/* get_action_prob(&self, s, temp, episode_id, rng) for every tree at once (src/async_mcts.rs:74-115).
 * states [G,2]; outputs pi [G,7], counts [G,7] (child N), q [G,7] (child Q); counts/q may be NULL.
 * RNG (temp == 0 tie-break) = stream (seed, first_game_id + g, ply = stones on board). */
az_status az_tree_get_action_prob(az_tree* t, const uint64_t* states, float temp, uint64_t seed,
                                  uint64_t first_game_id, float* pi, uint16_t* counts, float* q);
/* The Dirichlet root noise ("root_noise_eps_e6" above) of n roots at the engine's CURRENT alpha, from the device sampler the searches
 * run: eta_out [n,7] for root states [n,2] (canonical bitboards) on the streams (seed, game_ids[i], ply = stones of states[i]); the
 * valid-move mask is the state's, invalid actions get 0.  Independent of eps.  Pointers may be host or device memory. */
az_status az_root_noise_eta(az_engine* e, int32_t n, uint64_t seed, const uint64_t* game_ids, const uint64_t* states, float* eta_out);
/* The selected action of each tree's last az_tree_get_action_prob: actions [G], -1 for every tree when that call was not a Gumbel move
 * ("gumbel_m" above was 0).  The pointer may be host or device memory. */
az_status az_tree_get_selected(az_tree* t, int32_t* actions);
/* The Gumbel variates ("gumbel_m" above) of n roots, from the device code the searches run: g_out [n,7] for root states [n,2] (canonical
 * bitboards) on the streams (seed, game_ids[i], ply = stones of states[i]); invalid actions get 0, and so does every action when
 * temp_is_zero != 0.  Independent of the option's value.  Pointers may be host or device memory. */
az_status az_gumbel_values(az_engine* e, int32_t n, uint64_t seed, const uint64_t* game_ids, const uint64_t* states, int32_t temp_is_zero,
                           float* g_out);
/* ---- a SHARED tree batch: many host threads, one AsyncMcts (slot) each, one batched search ----
 * The reference's inference_thread (src/async_mcts.rs:117-189) answers the leaf boards of every episode thread with one predict
 * once batch_size of them are waiting.  Here a host that keeps Coach::execute_episode per thread (src/coach.rs:202-205, :241-272)
 * gives each thread one slot of a G-tree batch; each thread's blocking az_tree_slot_get_action_prob waits until the batch starts,
 * and one waiting caller (the leader; there is no library-owned thread) runs the whole batch as one search over the requested
 * slots and hands every caller its own result.  A caller's result is bit-identical to what a 1-game az_tree returns for the same
 * calls: it does not depend on which requests shared its batch, on timing or on the thread count.
 * az_tree_share turns the batch into a shared one (no slot held):
 *   window_us = 0: a batch starts when every held slot has a request waiting (the reference's batch_size rule);
 *   window_us > 0: also when the oldest waiting request is that old.  Calling it again only changes the window.
 * Afterwards az_tree_get_action_prob, az_tree_reset and az_tree_record_evals are refused (AZ_ERR_BAD_ARGUMENT).
 * "eval_cache_persist" applies per batch (0: every batch starts from an empty cache).  Slot calls do not set az_last_error. */
az_status az_tree_share(az_tree* t, int32_t window_us);
/* AsyncMcts::default for one slot: the lowest free slot, its tree rebuilt at the initial board before its next search.
 * AZ_ERR_CAPACITY when all G slots are held. */
az_status az_tree_slot_acquire(az_tree* t, int32_t* slot);
/* The thread leaves: batches stop waiting for the slot.  AZ_ERR_BAD_ARGUMENT when the slot is out of range or not held. */
az_status az_tree_slot_release(az_tree* t, int32_t slot);
/* get_action_prob(&self, s, temp, episode_id, rng) for one held slot (src/async_mcts.rs:74-115); blocks until its batch has run.
 * state [2] canonical; pi [7], counts [7] / q [7] may be NULL.  temp, seed and game_id are the request's own: tie-break RNG stream
 * = (seed, game_id, ply = stones), the stream of az_tree_get_action_prob with first_game_id = game_id.  A terminal root
 * (AZ_ERR_TERMINAL_ROOT) or a full tree (AZ_ERR_CAPACITY) fails only its own request; the message is az_tree_slot_error's. */
az_status az_tree_slot_get_action_prob(az_tree* t, int32_t slot, const uint64_t* state, float temp, uint64_t seed,
                                       uint64_t game_id, float* pi, uint16_t* counts, float* q);
/* Message of the slot's last failed az_tree_slot_get_action_prob ("" if none); valid until the slot's next call. */
const char* az_tree_slot_error(const az_tree* t, int32_t slot);
/* out[4] = {batches, requests, largest batch, batches started by the window} since az_tree_share. */
az_status az_tree_share_stats(az_tree* t, uint64_t* out);
/* Record every NNet::predict the search issues, per tree, in order (replay parity). cap = records per tree. */
az_status az_tree_record_evals(az_tree* t, int32_t cap);
/* Copy out the record log: rec_count [G]; states [G,cap,2], pis [G,cap,7], vs [G,cap] (any may be NULL). */
az_status az_tree_get_evals(az_tree* t, int32_t* rec_count, uint64_t* states, float* pis, float* vs);
/* Node count (NodeStore::len, src/node.rs:372-374) per tree, [G]. */
az_status az_tree_node_counts(az_tree* t, uint32_t* out);

/* ---- Coach::execute_episode x many, src/coach.rs:104-157 ------------------ */
typedef struct az_selfplay_params {
    int32_t n_games;         /* episodes to play in this call (global ids first_game_id .. +n_games) */
    int32_t concurrent;      /* game slots resident at once (0 = n_games); finished slots are refilled */
    int32_t num_sims;        /* src/coach.rs:30 */
    int32_t temp_threshold;  /* src/coach.rs:22 */
    int32_t max_depth;       /* src/coach.rs:32 */
    int32_t cpuct;           /* src/coach.rs:33 */
    int32_t model_id;
    int32_t symmetries;      /* !=0: emit identity + mirror per position (get_symmetries), else identity only */
    uint64_t reserve;        /* mcts_reserve_size, src/coach.rs:20 (clamped to the reachable bound) */
    uint64_t seed;
    uint64_t first_game_id;
    int32_t record_evals;    /* records per EPISODE kept for az_selfplay_get_evals (0 = off); works with slot refill */
    int32_t num_sim_threads; /* simulations in flight per tree, src/coach.rs:31, :249 (0 = 1; see az_tree_create) */
} az_selfplay_params;

/* Training tuples (s, pi, z) in game-id order then ply order; TrainingSample, src/nnet.rs:22-27. */
typedef struct az_samples {
    int64_t capacity;     /* in: tuples the arrays can hold (n_games*42, x2 with symmetries, always suffices) */
    int64_t count;        /* out */
    uint64_t* states;     /* [capacity,2] canonical bitboards (may be NULL) */
    float* boards;        /* [capacity,2,6,7] features (may be NULL) */
    float* pis;           /* [capacity,7] */
    float* zs;            /* [capacity] */
    int32_t* game_len;    /* [n_games] plies per game (may be NULL) */
    uint8_t* moves;       /* [n_games,42] actions played (may be NULL) */
} az_samples;

az_status az_selfplay(az_engine* e, const az_selfplay_params* p, az_samples* out);
/* The same as a SESSION (no reference counterpart: the reference's Coach collects an iteration's episodes from a rayon pool,
 * src/coach.rs:246-260, in whatever order they finish).  az_selfplay_begin fixes the episodes (p->n_games of them, ids 0 ..
 * n_games-1, first_game_id / seed as in az_selfplay) and fills the slots; az_selfplay_next(k, out) plays until the NEXT k episodes
 * in id order have finished and returns exactly the tuples az_selfplay would return for them (an episode depends on its id,
 * the seed and the net alone) -- while the slots they freed already play later episodes.  A host that fetches its episodes in
 * chunks (one training-set shard, one bench step at a time) thereby pays the drain of the last slots once per session, not
 * once per chunk.  az_selfplay_end closes the session (az_destroy does too); one session per engine; the model may not be
 * changed while it is open.  az_selfplay is begin + next(n_games) + end.
 *
 * THE SESSION CONTRACT (calls interleaved with an open session; tests/session_contract.py lists every export and every option key
 * with its class, tests/test_session_contract_gpu.py holds each row to it under both drivers, lock-step and "selfplay_async").  An open
 * session owns its model, its view of the evaluation cache and the options it captured at az_selfplay_begin.  Between az_selfplay_begin
 * and az_selfplay_end every other call is of exactly one class:
 *   REFUSED   AZ_ERR_BAD_ARGUMENT on entry, before any work, with an az_last_error that names the entry (the slot call: with
 *             az_tree_slot_error).  Nothing changes: every option and counter reads as before, the session stays usable and its
 *             remaining chunks are what they would have been.  These are
 *               - every entry that runs a tree search (a search sizes, clears and retags the evaluation cache): az_selfplay,
 *                 az_selfplay_begin, az_arena, az_tournament, az_tree_get_action_prob, az_tree_slot_get_action_prob, az_tree_share;
 *               - the sample and solver entries that use the engine's workspaces: az_samples_merge, _blend_z, _surprise, _holdout,
 *                 az_net_train_samples, az_net_train_draw, az_solve, az_move_quality;
 *               - any change of a conv model's class by az_net_set_class (a call that leaves the stored class as it is returns AZ_OK);
 *               - the options "net_fp8", "eval_mirror", "conv2_table", "eval_dedup", "eval_cache_log2", "eval_cache_persist",
 *                 "eval_cache_max_stones", "selfplay_async", "selfplay_async_launches", "selfplay_async_iters", "selfplay_record_search"
 *                 and the root-move keys (root noise, playout cap, forced playouts, Gumbel).
 *   BY MODEL  refused, as above, when the call's destination is the session's model id, inert for any other id: az_net_free,
 *             az_net_set_kind, az_net_init_random, az_net_load, az_net_set_params, az_net_train, az_net_train_end, az_net_train_ema.
 *             (Should a write reach the session's model all the same, az_selfplay_next notices the changed generation and refuses.)
 *   INERT     accepted; the session's remaining chunks are bit for bit those of the undisturbed session, and the call returns what it
 *             returns with no session open: every other entry (the predicts and az_net_evaluate on any model, the session's included;
 *             the getters; az_tree_create / _reset / _destroy and the tree's logs; az_get_stats / az_reset_stats; the az_comm_* entries
 *             and the collectives; az_net_train_begin / _step; every other option: the bit-identical kernel and schedule switches, the
 *             profile and trainer keys, "arena_opening_plies").
 * az_destroy with a session open closes it first.
 * A TRAINING session (az_net_train_begin .. az_net_train_end) has a rule of the same kind: while it is open az_net_train,
 * az_net_train_samples, az_net_train_draw and az_net_train_set_validation are refused; a second az_net_train_begin is a RESTART -- the
 * open session is dropped without storing anything, and what follows is bit for bit what follows a first az_net_train_begin. */
az_status az_selfplay_begin(az_engine* e, const az_selfplay_params* p);
az_status az_selfplay_next(az_engine* e, int32_t n_games, az_samples* out);
az_status az_selfplay_end(az_engine* e);
/* Which plies of the episodes of the last az_selfplay / az_selfplay_next call were FULL moves ("playout_cap_sims" above), i.e. became
 * tuples: bit `ply` of mask[i] for the i-th episode of that call (42 plies fit a word).  All ones up to game_len when the feature is
 * off.  mask holds as many words as that call returned episodes. */
az_status az_selfplay_get_full_plies(az_engine* e, uint64_t* mask /* [n_games] */);
/* ---- the search's own statistics per tuple (no reference counterpart; csrc/az_target.h) ----
 * az_set_option(e, "selfplay_record_search", 1) (0 = default, OFF; state of the engine; refused while a self-play session is open) makes
 * self-play keep, per episode and ply next to pi:
 *   R        the root value of the move: the visit-weighted mean of the root children's RAW q (the `q` and `counts` of
 *            az_tree_get_action_prob: raw under forced playouts, pruning and Gumbel), summed in ascending action order in f32 and clamped
 *            to [-1, 1]; in the perspective of the side to move, the sign of the tuple's z
 *   prior    the root children's stored prior by action AS THE SEARCH USED IT: root noise is included while that is on; 0 for an invalid
 *            action.  The raw net output is not recovered
 * With the option off no array exists, no kernel is added to any path and every output and counter is what it was.  With it on the tuples
 * are unchanged bit for bit; one small kernel runs in front of each move of the lock-step paths ("fused_search" 0 / 1, every "eval_dedup",
 * num_sim_threads > 1, slot refill, sessions, both games, fp8 and "eval_mirror" models, root noise, playout cap, forced playouts, Gumbel).
 * az_selfplay / az_selfplay_begin refuse (AZ_ERR_BAD_ARGUMENT) the option together with "selfplay_async" = 1.  az_arena, az_tree_* and the
 * slot calls never record.
 * az_selfplay_get_search: rows of the last az_selfplay / az_selfplay_next, tuple for tuple in az_samples' order (the same playout-cap
 * compaction and symmetry expansion: a mirrored tuple's prior is reversed, its R is the same); host or device pointers; either may be NULL.
 * AZ_ERR_BAD_ARGUMENT when that call ran with the option off. */
az_status az_selfplay_get_search(az_engine* e, float* root_q /* [count] */, float* root_prior /* [count,7] */);
/* Eval log of the last az_selfplay with record_evals > 0: rec_count [n_games], states [n_games,cap,2], ... */
az_status az_selfplay_get_evals(az_engine* e, int32_t* rec_count, uint64_t* states, float* pis, float* vs);

/* ---- position averaging: one training tuple per distinct position (no reference counterpart: src/coach.rs:296-329 trains on every
 * copy; credited to the "Lessons from AlphaZero: Connect Four" write-ups).  Strictly opt-in: a host that never calls it runs
 * nothing of it.  A window of self-play tuples holds the empty board once per episode and the first openings thousands of times, each
 * copy with its own noisy pi and its own game's z; az_samples_merge returns one tuple per distinct position, carrying the MEAN pi and the
 * MEAN z of its copies, and NNet::train's cost shrinks with the set.  A pure function of its arguments, deterministic to the bit on every
 * host, rank and schedule (csrc/az_merge.h).  The contract:
 *   in         src->count tuples n (0 .. 2^24), host or device memory: the position from src->states [n,2]; when states is NULL, from
 *              src->boards [n,2,6,7], converted on the device.  src->pis and src->zs are required; capacity, game_len and moves are
 *              ignored
 *   out        dst->count = m, the distinct positions; per position dst->states, dst->boards, dst->pis, dst->zs (states and boards may
 *              be NULL, pis and zs are required); counts [m] the multiplicities (may be NULL; they sum to n).  dst->capacity >= n is
 *              required (m <= n always fits); no dst array (nor counts) may overlap a src array
 *   key        Game::pack(s) of the engine's game, the 64-bit identity of a state (never 0).  With AZ_MERGE_CANONICAL in flags the key
 *              is pack(c(s)), c the canonicalisation of "eval_mirror" (csrc/az_mirror.h): a position and its left-right mirror image
 *              merge, a tuple whose state is the mirrored one contributes pi reversed (mirror_action), and the output state is c(s).
 *              A host that expands symmetries afterwards gets both orientations back.  pack is an identity for REACHABLE states (stones
 *              stacked from the bottom of their columns); the validation below accepts any two disjoint in-board bitboards, and two
 *              such patterns with floating stones can share a key -- they are then merged under the first one's state
 *   order      output group j is the j-th distinct key in order of FIRST OCCURRENCE in the input (ascending lowest input index): the
 *              result does not depend on any hash layout or schedule
 *   k = 1      a group of one copies its tuple bit for bit (under AZ_MERGE_CANONICAL canonicalised, which is exact): a set without
 *              duplicates comes back unchanged
 *   k > 1      each of the eight values (pi[0..6], z) is accumulated as an integer, q(x) = llrint((double)x * 2^38) -- the product is
 *              exact, llrint rounds to nearest even -- summed in int64: S.  The mean is (float)((double)S / (double)(k * 2^38)): C's
 *              int64 -> double conversion, a divisor that is exact in double, one IEEE double division, one rounding to f32.  pi is NOT
 *              renormalised.  Integer addition is associative, so S does not depend on the order in which atomics, wave-level sums or
 *              the per-workgroup LDS tables deliver the addends; z is not always +-1 (a draw is DRAW_EPS), hence a fixed-point grid and
 *              not a win/loss counter.  Absolute quantisation error 2^-39 per value; n <= 2^24 keeps every sum below 2^62
 *   refused    AZ_ERR_BAD_ARGUMENT with nothing written (the data checks run on the device in the first pass): a pi or z outside
 *              [-1, 1] or NaN; a state with overlapping stones or bits outside the 7x6 board; a boards feature that is not exactly 0 or
 *              1, or a cell set in both planes; n > 2^24; dst->capacity < n; a dst array overlapping a src array; unknown flag bits; a
 *              call while a self-play session is open.  n = 0 is legal and gives m = 0
 *   purity     models, trees, the evaluation cache, options and every az_stats counter but device_ms are untouched.  Runs on the
 *              engine's stream in a workspace the engine owns: sized by the call (about 200 bytes per tuple, 340 more per tuple for each
 *              of boards in and boards out: over 10 GB at 2^24 tuples by the boards route), reused by later calls of the same or a
 *              smaller size, and given back when a call needs under a quarter of a workspace of more than 256 MiB
 * Whether averaged targets change playing strength is unmeasured. */
#define AZ_MERGE_CANONICAL 1   /* flags bit 0 */
az_status az_samples_merge(az_engine* e, const az_samples* src, int32_t flags, az_samples* dst, uint32_t* counts);

/* ---- z/q value targets and surprise resampling (no reference counterpart; csrc/az_target.h states every formula operation by operation;
 * DESIGN.md section 4.1k).  Both are pure in az_samples_merge's sense -- models, trees, the cache, options and every az_stats counter but
 * device_ms stay untouched --, run on the engine's stream, take host or device pointers and are refused while a self-play or a training
 * session is open.  Their outputs are ordinary tuples: az_samples_merge, the trainers, the .examples files and az_gather_samples need not know.
 *
 * az_samples_blend_z: zs_out[i] = a * zs[i] + b * root_q[i] with b = (float)lambda_e6 / 1e6f and a = 1.0f - b (four f32 roundings);
 * lambda_e6 = 0 returns zs and 1000000 returns root_q bit for bit.  zs_out may equal zs.  n = 0 is legal.  Refused (AZ_ERR_BAD_ARGUMENT),
 * with nothing written: n < 0, lambda_e6 outside 0 .. 1000000, a NaN or a |value| > 1 in either input.
 *
 * az_samples_surprise: writes tuple i of src c_i times (KataGo's policy surprise weighting as a resampling of the window):
 *   KL_i     KL(pi_i || prior_i) in f32 over the actions with pi >= 2^-126 (prior floored at 2^-126), clamped to [0, 64]
 *   K_i, SK  K_i = llrint(KL_i * 2^32); SK = their sum in u64: an integer sum, so no result depends on the order of the additions
 *   w_i      (1 - s) + s * n * K_i / SK in f64 with s = share_e6 / 1e6 (1 when SK = 0): the weights average 1 -- a share 1 - s spread
 *            uniformly, a share s in proportion to KL
 *   c_i      floor(w_i) + (U_i < frac(w_i)), U_i = (rng_draw(seed, i, 0, RNG_SURPRISE) >> 11) * 2^-53; sum c_i <= 2n
 * It reads src->count, pis, zs and states and/or boards (validated as az_samples_merge validates them; a prior outside [0, 1] is refused as
 * well); n <= 2^24; share_e6 in 0 .. 1000000.  counts[i] = c_i and kl[i] = KL_i (each may be NULL).  With dst set, dst holds tuple i
 * repeated c_i times in input order, every copy bit for bit, in the arrays dst has (pis and zs are required; states / boards only where src
 * has them), and dst->count = sum c_i; dst->capacity >= 2n is required and no dst array may overlap a src array or priors.  share_e6 = 0, or
 * a window with SK = 0, returns the input unchanged with all counts 1.  Every refusal leaves dst, counts and kl unwritten.
 * az_samples_merge turns the duplicates back into multiplicities (its `counts`), which az_net_train_samples draws by.
 * Whether either target changes playing strength is unmeasured. */
az_status az_samples_blend_z(az_engine* e, int64_t n, const float* zs, const float* root_q, int64_t lambda_e6, float* zs_out);
az_status az_samples_surprise(az_engine* e, const az_samples* src, const float* priors /* [n,7] */, int64_t share_e6, uint64_t seed,
                              az_samples* dst /* may be NULL */, uint32_t* counts /* [n], may be NULL */, float* kl /* [n], may be NULL */);

/* ---- NNet::train from merged positions: batch rows drawn in proportion to their multiplicities (no reference counterpart; csrc/az_draw.h,
 * DESIGN.md section 8.2).  Strictly opt-in: az_net_train and every kernel it launches are untouched.  az_samples_merge gives one tuple per
 * distinct position and `counts`; the cross-entropy of k copies against a policy is k times the cross-entropy of their mean pi plus a
 * constant (likewise the squared error of z), and az_net_train draws every batch row with replacement, so drawing merged tuple i with
 * probability counts[i] / sum(counts) IS the raw window's distribution -- at the merged set's size and step count.  The rule:
 *   weights    u32 [n], host or device; NULL = all ones; a weight of 0 is legal (the tuple is never drawn).  Q[i] = weights[0] + .. +
 *              weights[i] in u64 (a device prefix sum), W = Q[n-1]
 *   steps      an epoch has max(1, S / "train_batch") steps, S = n; with AZ_TRAIN_EPOCH_BY_WEIGHT S = W (the raw window's step count)
 *   row        row j of global step t (counted over the call's epochs): r = rng_draw("train_seed", t, j, RNG_BATCH), az_net_train's own
 *              draw; u = (r * W) >> 64 of the 128-bit product; the row is tuple min{ i : Q[i] > u }.  With every weight 1 that is i = u,
 *              az_net_train's row
 *   mirror     with AZ_TRAIN_MIRROR the row is mirrored iff the top bit of rng_draw("train_seed", t, j, RNG_TRAIN_MIRROR = 9) is set:
 *              column c of both planes comes from column 6 - c, pi is reversed, z stays (what a host needs behind AZ_MERGE_CANONICAL,
 *              whose output holds one orientation of every position)
 *   the rest   dropout masks, Adam's bias corrections, the learning-rate table, the averaged shadow and az_net_train_history are
 *              az_net_train's, keyed by the same global step: with weights NULL and flags 0 the result is az_net_train's bit for bit
 * az_net_train_samples reads s->count (n), s->pis, s->zs and s->states [n,2], or s->boards [n,2,6,7] when states is NULL; every array
 * may be host or device memory.  From states the device holds 16 bytes per position and builds each batch's planes from the bits (bit
 * c * 7 + (5 - r) of word p is cell (r, c) of plane p); about 60 bytes per tuple with weights, 368 by az_net_train's planes.
 * az_net_train_draw runs the prefix sum and the draw alone, with the engine's current "train_seed" and "train_batch", for global steps
 * t0 .. t0 + steps: idx_out [steps * batch] and mirror_out [steps * batch] (may be NULL; all 0 without AZ_TRAIN_MIRROR), host or device.
 * It touches no model, no trainer state and no az_stats counter but device_ms (the kind of entry az_root_noise_eta is).
 * Refused with AZ_ERR_BAD_ARGUMENT and nothing written: n < 1 or n > 2^31 - 1; W = 0; unknown flag bits; pis or zs NULL, or states and
 * boards both NULL; a states entry with overlapping stones or bits outside the 7x6 board; a call while a training session
 * (az_net_train_begin) or a self-play session is open.  Playing strength under this route is unmeasured. */
#define AZ_TRAIN_EPOCH_BY_WEIGHT 1
#define AZ_TRAIN_MIRROR          2
az_status az_net_train_samples(az_engine* e, int32_t prev_id, int32_t id, const az_samples* s,
                               const uint32_t* weights, int32_t flags);
az_status az_net_train_draw(az_engine* e, int64_t n, const uint32_t* weights, int32_t flags, uint64_t t0,
                            int64_t steps, int64_t* idx_out /* [steps*b] */, uint8_t* mirror_out /* [steps*b], may be NULL */);

/* ---- held-out loss on the device, a hold-out rule and per-epoch validation inside NNet::train (no reference counterpart; csrc/az_score.h,
 * DESIGN.md sections 4.1l and 8.3).  Strictly opt-in: with no set registered and "train_keep_best" / "train_patience" at 0 every kernel
 * launched and every bit computed is what it was.
 *
 * az_net_evaluate: the loss of model_id AS SELF-PLAY RUNS IT over a whole window in one call.  (p, v) of tuple i is, by definition, what
 * az_net_predict_states returns for its state on this engine now: the model's effective class, "eval_mirror" if it is on, any model kind
 * (the stub and hash nets included).  Per tuple, against its target (pi, z), with weight w_i (u32; 1 when weights is NULL):
 *   ce    t = 0; for a ascending with pi[a] >= 2^-126: t = t + pi[a] * log2(max(p[a], 2^-126)); ce = -(t * ln 2) clamped to [0, 128] (NaN: 128)
 *   kl    az_samples_surprise's KL(pi || p), clamped to [0, 64]
 *   se    (v - z)^2 (a NaN or a value above 4 counts as 4)
 *   hit   the lowest a that maximises pi[a] == the lowest LEGAL a (its column is not full) that maximises p[a]
 * all in f32, operation by operation (csrc/az_score.h), then K(x) = llrint(x * 2^30) and the u64 sums S_ce = sum w_i K(ce_i), S_kl, S_se,
 * S_hit = sum w_i hit_i, W = sum w_i: integer sums, the same bits whatever the order of the additions.
 *   score [AZ_SCORE_FIELDS]   n, W, loss_pi = S_ce / 2^30 / W, loss_v = S_se / 2^30 / W, kl = S_kl / 2^30 / W, top1 = S_hit / W (n and W are
 *                             integers of at most 2^24, exact in a double)
 *   sums [AZ_SCORE_SUMS]      S_ce, S_kl, S_se, S_hit, W (may be NULL)
 *   ce, se, kl [n]            the per-tuple values (each may be NULL; host or device)
 * It reads s->count (n), s->pis, s->zs and s->states [n,2], or s->boards [n,2,6,7] when states is NULL; every array, weights included, may
 * be host or device memory.  The window is staged once; the forwards of all max_batch chunks and the score kernel behind each run on the
 * engine's stream with one synchronisation at the end and no copy of a pi or a v to the host.  The evaluation cache is neither read nor
 * written; no cache tag, generation or captured graph of any model changes; no az_stats counter but device_ms moves.  Allowed wherever
 * az_net_predict_states is.  AZ_ERR_BAD_ARGUMENT, with nothing written: n < 1 or n > 2^24; W = 0 or W > 2^24; pis or zs NULL, or states
 * and boards both NULL; a pi outside [0, 1] or a z outside [-1, 1] (NaN included); a state or plane set az_samples_merge would refuse.
 * AZ_ERR_NO_MODEL: an id that is not initialised.
 *
 * az_samples_holdout: held[i] = (mix64(mix64(seed) ^ k_i) >> 40) < share_e6 * 2^24 / 1000000 (unsigned 64-bit), k_i the key
 * az_samples_merge forms for tuple i under AZ_MERGE_CANONICAL: a function of the position alone, so a position and its mirror image are
 * always on one side and a held-out position stays held out in every window split with the same seed.  Share 0 holds nothing, 1000000
 * everything.  Inputs and validation are az_samples_merge's (states or boards, pis, zs; host or device; n <= 2^24; n = 0 is legal); held
 * [n] u8, host or device.  Refused while a self-play session is open.
 *
 * az_net_train_set_validation: copies the set to the device (16-byte states, about 60 bytes per tuple with weights; validated as
 * az_net_evaluate validates it) and keeps it until the next call or az_destroy; v = NULL clears it.  Refused while a training session is
 * open.  With a set registered, az_net_train and az_net_train_samples score it at the end of every epoch: the weights and BatchNorm moving
 * averages exactly as az_net_train_end would store them at that step (the live weights, not the averaged shadow) go into a model slot no
 * id names, of the effective class of the destination id (a fresh id: the engine's), and are scored as az_net_evaluate scores.  The
 * trainer is only read: with both options below at 0 the stored model is bit for bit the one trained without a set.
 *   "train_keep_best"  0 (default) / 1: store the weights of the epoch with the lowest loss_pi + loss_v (the first such epoch) instead of
 *                      the last epoch's
 *   "train_patience"   0 (default: off) or 1 .. 1000: stop behind the first epoch that ends that many consecutive epochs without a new
 *                      best; az_net_train_history and the validation history then hold the epochs actually run
 * Either option without a registered set makes az_net_train / az_net_train_samples fail with AZ_ERR_BAD_ARGUMENT before they begin.  The
 * fine-grained az_net_train_begin / _step / _end never validate.
 * az_net_train_validation: (loss_pi, loss_v, kl, top1) of each epoch of the last az_net_train / az_net_train_samples: writes
 * min(epochs, cap_epochs) rows to out (may be NULL), *best_epoch (may be NULL) = the first epoch of the lowest loss_pi + loss_v (-1 with
 * no rows), and returns the number of rows (0 when no set was registered).
 * Whether early stopping or keeping the best epoch changes playing strength is unmeasured. */
#define AZ_SCORE_FIELDS 6
#define AZ_SCORE_SUMS   5
az_status az_net_evaluate(az_engine* e, int32_t model_id, const az_samples* s, const uint32_t* weights,
                          double* score /* [AZ_SCORE_FIELDS] */, uint64_t* sums /* [AZ_SCORE_SUMS], may be NULL */,
                          float* ce /* [n], may be NULL */, float* se /* [n], may be NULL */, float* kl /* [n], may be NULL */);
az_status az_samples_holdout(az_engine* e, const az_samples* s, int64_t share_e6, uint64_t seed, uint8_t* held /* [n] */);
az_status az_net_train_set_validation(az_engine* e, const az_samples* v /* NULL clears */, const uint32_t* weights);
int32_t az_net_train_validation(const az_engine* e, double* out /* [cap_epochs,4] */, int32_t cap_epochs, int32_t* best_epoch);

/* ---- arena::play_games, src/arena.rs:62-99 + gate, src/coach.rs:377-390 ---- */
typedef struct az_arena_params {
    int32_t num_games;      /* num/2 per seating, src/arena.rs:83 */
    int32_t num_sims;
    int32_t max_depth;
    int32_t cpuct;
    int32_t new_model_id;   /* first listed player ("new", nmcts, src/coach.rs:345-354) */
    int32_t old_model_id;   /* second listed player ("old", pmcts, src/coach.rs:333-343) */
    uint64_t reserve;
    uint64_t seed;
    /* Sharding (one process per GPU): this call plays games [first_game, first_game + num_games) of an arena of
     * total_games (0 = num_games, first_game must then be 0).  Seating (game < total/2 -> (new, old)) and the RNG
     * stream use the GLOBAL game index, so shards add up to exactly the unsharded arena (3-counter all-reduce).
     * A sharded call plays all num_games of its range (the caller splits an even total). */
    int32_t first_game;
    int32_t total_games;
    int32_t record_evals;     /* records per game and player kept for az_arena_get_evals (0 = off) */
    int32_t num_sim_threads;  /* simulations in flight per tree, src/coach.rs:340, :351 (0 = 1; see az_tree_create) */
    /* play_games' `board: Option<G>` (src/arena.rs:62-67, :12-16): every game starts from this position with the first
     * seat (cur_player = +1) to move; start_board = {first seat's stones, second seat's stones}.  use_start_board = 0: the
     * initial board (None). */
    int32_t use_start_board;
    /* sharded call (total_games > 0) on an engine with a communicator (az_comm_init): != 0 sums out_wld over the ranks
     * (one 3-counter all-reduce over the communicator), so every rank returns the whole arena's tally */
    int32_t allreduce_wld;
    uint64_t start_board[2];
} az_arena_params;
/* out_wld[3] = {Win, Loss, Draw} for the new model (GameResult, src/arena.rs:54-59);
 * results [num_games] (may be NULL): +1 first seat won, -1 second seat won, 0 draw (play_game, src/arena.rs:51). */
az_status az_arena(az_engine* e, const az_arena_params* p, uint64_t out_wld[3], int8_t* results);
/* Eval log of the last az_arena with record_evals > 0, for the trees of player `which` (0 = new model, 1 = old model):
 * rec_count [num_games], states [num_games,cap,2], pis [num_games,cap,7], vs [num_games,cap] (any may be NULL). */
az_status az_arena_get_evals(az_engine* e, int32_t which, int32_t* rec_count, uint64_t* states, float* pis, float* vs);
/* Move record of the last az_arena: game_len [num_games] plies played, moves [num_games][AZ_MAX_PLIES] the actions in order (the
 * board sequence play_game's `verbose` prints, src/arena.rs:20-27; what one reaches for when an arena game diverges).  Either
 * may be NULL. */
az_status az_arena_get_moves(az_engine* e, int32_t* game_len, uint8_t* moves);
/* Opening book of the paired arena openings (option "arena_opening_plies" above): boards [n][2], each entry written as start_board
 * is -- {first seat's stones, second seat's stones}, first seat to move.  Pair p of every later az_arena starts from entry p % n
 * (plus "arena_opening_plies" random plies).  n = 0 clears the book; at most 65536 entries; the book is copied into the engine.
 * Refused with AZ_ERR_BAD_ARGUMENT, leaving the previous book in place: overlapping stones, bits outside the 7x6 board, an entry
 * that is finished under the engine's game, n out of range.  While a book is set, az_arena with use_start_board != 0 is refused. */
az_status az_arena_set_opening_book(az_engine* e, const uint64_t* boards, int32_t n);
/* Openings of the last az_arena: boards [num_games][2] the position each game started from, len [num_games] the random plies played
 * onto its base, moves [num_games][12] those actions (zero behind len).  Without the feature: the common start position and len = 0.
 * Any pointer may be NULL.  AZ_ERR_BAD_ARGUMENT before the first az_arena. */
az_status az_arena_get_openings(az_engine* e, uint64_t* boards, int32_t* len, uint8_t* moves);

/* ---- az_tournament: one batched round robin of K models (no reference counterpart).  Strictly opt-in.
 * az_arena seats two models; ranking K checkpoints by it costs K (K - 1) / 2 calls, each a chain of 42 plies x num_sims dependent steps
 * that leaves the GPU almost empty.  This call plays the games of ALL pairs in one such chain.
 *   model_ids [num_models]   K = 2 .. 16 pairwise distinct, initialised model ids
 *   games_per_pair           n, even, >= 2: n / 2 per seating, as az_arena's num_games
 *   num_sims, max_depth, cpuct, num_sim_threads (0 = 1), reserve, seed: as the fields of az_arena_params
 * The pairs are (i, j), i < j, in lexicographic order, P = K (K - 1) / 2 of them; game g of pair p has TOURNAMENT INDEX p * n + g.
 * THE CONTRACT: game (p, g) is bit for bit -- result, length, every move, opening -- game g of az_arena on the same engine with the same
 * options, called with num_games = n, new_model_id = model_ids[i], old_model_id = model_ids[j], the same num_sims, max_depth, cpuct,
 * reserve, seed and num_sim_threads, and every other field 0.  Seating, the tie-break stream (seed, g, ply) and the opening of pair
 * g % (n / 2) therefore use the index INSIDE the pair; "arena_opening_plies" and the opening book apply exactly as to az_arena, so every
 * pair of models plays the same n / 2 openings in both seatings, which is what a rating wants.  SWITCH OPENINGS ON for a tournament:
 * without them every game of a pair at temperature 0 is one of two games.  Per-model classes (az_net_set_class), "net_fp8",
 * "eval_mirror", the evaluation cache, both games and stub, hash and conv models work as in az_arena; root noise, playout cap, forced
 * playouts and Gumbel never apply, as in az_arena.  There is no start_board (the openings are the book and the random plies), no
 * sharding and no communicator: the call plays on one engine.
 *   wld [K][K][3]            wld[i][j] = {W, L, D} from model_ids[i]'s side = az_arena's out_wld of that pair; wld[j][i] = {L, W, D}; the
 *                            diagonal is 0
 *   results [P * n]          (may be NULL) az_arena's convention, in tournament order: +1 when the first seat won
 * Afterwards az_arena_get_moves and az_arena_get_openings return the P * n games in tournament order (az_move_quality runs on them
 * unchanged); az_arena_get_evals is refused, there is no eval log here.  az_stats.games and the tree counters advance as over the P
 * az_arena calls (leaf_rows_executed by no more: the pairs share openings and each model's leaves of a step share one election table).
 * How it runs: one tree batch per MODEL ((K - 1) n trees, 2 P n in all, the arena's two per game), one search per model and ply on the
 * engine's stream and at most three side streams of the engine's own (models dealt round robin; ids that share weights share a stream).
 * Refused with AZ_ERR_BAD_ARGUMENT, nothing written and the last move record kept: K outside 2 .. 16; n odd or < 2; P * n > 65536; a
 * NULL model_ids or wld; a repeated or uninitialised model id; a conv model whose (K - 1) n threads rows exceed az_config.max_batch;
 * whatever az_arena refuses for num_sims, max_depth, reserve and num_sim_threads; an open self-play session.
 * The parameters travel as arguments, not as a struct: the set of ABI structs is closed. */
az_status az_tournament(az_engine* e, const int32_t* model_ids, int32_t num_models, int32_t games_per_pair, int32_t num_sims,
                        int32_t max_depth, int32_t cpuct, int32_t num_sim_threads, uint64_t reserve, uint64_t seed, uint64_t* wld,
                        int8_t* results);
/* Ratings from a result matrix (alphazero-rs_amd/csrc/az_rating.h).  Takes no engine: the library answers it without a GPU.
 * Bradley-Terry with a draw counted as half a win, by Hunter's MM iteration; every sum in ascending j, in double.
 *   wld [K][K][3]   as az_tournament writes it (the diagonal is ignored); K = 2 .. 16
 *   prior_games     >= 0, finite: virtual games added to every pair, half won by each side (s_ij = W + D/2 + prior/2,
 *                   n_ij = W + L + D + prior).  2 is the recommended value; 0 with a model that has no games, or only wins or only
 *                   losses, diverges (the iteration then stops at its limit of 100 000 sweeps)
 *   elo [K]         400 log10(gamma_i) minus the mean over the models, gamma the fixed point of
 *                   gamma_i = S_i / sum_j n_ij / (gamma_i + gamma_j), S_i = sum_j s_ij, iterated from gamma = 1 (each sweep scaled to
 *                   sum gamma = K) until max_i |gamma'_i - gamma_i| / gamma_i < 1e-13
 *   elo_se [K]      (may be NULL) (400 / ln 10) / sqrt(sum_j n_ij gamma_i gamma_j / (gamma_i + gamma_j)^2).  APPROXIMATE: the diagonal
 *                   of the Fisher information only, which ignores the covariance between the models; prior games count as games
 *   sweeps          (may be NULL) sweeps run
 * Refused with AZ_ERR_BAD_ARGUMENT, nothing written: K outside 2 .. 16, a negative or non-finite prior_games, a NULL wld or elo. */
az_status az_rating_fit(const uint64_t* wld, int32_t K, double prior_games, double* elo, double* elo_se, int32_t* sweeps);

/* ---- exact endgame solver and move-quality report (no reference counterpart).  Strictly opt-in: a host that never calls these runs
 * nothing of them.  The game-theoretic value of a late position can be computed exactly; a move then either keeps that value or throws it
 * away, which is an ABSOLUTE measure of play that needs no opponent.  The search, its frozen rule and the table entry are in
 * alphazero-rs_amd/csrc/az_solve.h, the kernels in az_solve.hip.
 *
 * az_solve: n positions (0 .. 2^24; canonical {mine, theirs}, host or device memory), every root action of each.
 *   move_values [n,7]   the outcome for the side to move after it plays the action: -1, 0, +1; AZ_SOLVE_ILLEGAL for an action that is
 *                       not legal and for every action of a finished position; AZ_SOLVE_UNKNOWN when the search of that action needed
 *                       more than max_nodes nodes, or the position has fewer than min_stones stones
 *   values [n]          (may be NULL) +1 if any action is +1; else AZ_SOLVE_UNKNOWN if any legal action is UNKNOWN; else the maximum
 *                       over the legal actions.  A finished position: the value of its ended_code as the tree sees it (+1 when the
 *                       side that moved in has won, 0 for a full board)
 *   nodes [n,7]         (may be NULL) nodes the search of the action entered (0 for an action decided without a search; max_nodes
 *                       for an UNKNOWN one)
 *   max_nodes           budget per (position, action), 1 .. 2^30
 *   min_stones          0 .. 42: positions with fewer stones are not searched (every legal action UNKNOWN, 0 nodes)
 *   tt_log2             0 = no transposition table, else 8 .. 16: 2^tt_log2 8-byte entries per resident lane, private to the item
 *   max_lanes           0 = the grid is sized from the device (CUs x resident waves x 64), else a multiple of 64 that caps it.  The
 *                       grid is also capped so that the table stays under 4 GiB
 *   The result of every (position, action) -- value, node count, UNKNOWN or not -- is a pure function of (state, action, max_nodes,
 *   min_stones, tt_log2, game): it does not depend on n, the grid, the schedule or the other positions of the call.
 *   refused             AZ_ERR_BAD_ARGUMENT with nothing written: a parameter out of range; n outside 0 .. 2^24; NULL states or
 *                       move_values; a state with overlapping stones, bits outside the board or floating stones (the search needs a
 *                       reachable stacking); a call while a self-play session is open.  n = 0 is legal
 *   purity              models, trees, the evaluation cache, options and every az_stats counter but device_ms are untouched.  Runs on
 *                       the engine's stream in workspaces the engine owns (lanes x 8 B << tt_log2 of table, about 60 bytes per
 *                       position), reused by later calls and given back as az_samples_merge's is
 *
 * az_move_quality: n recorded games (at most 2^24 / 42), replayed on the device.  start_boards [n,2] as az_arena_get_openings returns
 *   them (NULL = the initial board), game_len [n] and moves [n,AZ_MAX_PLIES] as az_arena_get_moves and az_samples.game_len / moves
 *   return them.  Every position that is reached is solved as by az_solve and the move played there classified:
 *   ply_class [n,AZ_MAX_PLIES]   AZ_MQ_SKIPPED behind game_len and at positions with fewer than min_stones stones; AZ_MQ_KEPT when the
 *                       value after the move equals the position's value (a played move of value +1 is KEPT even when siblings are
 *                       UNKNOWN); AZ_MQ_WIN_TO_DRAW, AZ_MQ_WIN_TO_LOSS, AZ_MQ_DRAW_TO_LOSS; AZ_MQ_UNKNOWN when the position's value,
 *                       or the played move's value where it is needed, is UNKNOWN
 *   ply_value [n,AZ_MAX_PLIES]   (may be NULL) the position's value as az_solve's values[i]; AZ_SOLVE_UNKNOWN where the class is SKIPPED
 *   refused             as az_solve, and: an illegal move in a record, a game_len outside 0 .. 42 or beyond the end of its game, a
 *                       start board that is not a reachable stacking
 *   The report counts exact value-losing moves from min_stones on.  It says nothing about the opening, nor about a ply the budget
 *   left UNKNOWN. */
#define AZ_SOLVE_ILLEGAL (-128)
#define AZ_SOLVE_UNKNOWN 127
#define AZ_MQ_SKIPPED 0
#define AZ_MQ_KEPT 1
#define AZ_MQ_WIN_TO_DRAW 2
#define AZ_MQ_WIN_TO_LOSS 3
#define AZ_MQ_DRAW_TO_LOSS 4
#define AZ_MQ_UNKNOWN 5
az_status az_solve(az_engine* e, const uint64_t* states, int32_t n, uint32_t max_nodes, int32_t min_stones, int32_t tt_log2, int32_t max_lanes,
                   int8_t* move_values, int8_t* values, uint32_t* nodes);
az_status az_move_quality(az_engine* e, const uint64_t* start_boards, const int32_t* game_len, const uint8_t* moves, int32_t n,
                          uint32_t max_nodes, int32_t min_stones, int32_t tt_log2, int32_t max_lanes, uint8_t* ply_class, int8_t* ply_value);

/* ---- the collective of the sharded Coach loop (no reference counterpart: the reference is one process,
 * src/coach.rs:241-272 fans episodes out over a rayon pool; here one process per GPU plays a shard of the global
 * episode ids and the (s, pi, z) tuples meet once per episode batch) --------------------------------------------------
 * RCCL over xGMI on the engine's own stream.  az_comm_unique_id is called on ONE rank; the host ships the 128 bytes to the
 * others by its own means (a file, MPI, torch.distributed ...) and every rank calls az_comm_init with them.
 * The id alone decides the backend: an id of az_comm_local_id makes the same collectives run between engines of this process,
 * without RCCL (below). */
#define AZ_COMM_ID_BYTES 128
az_status az_comm_unique_id(az_engine* e, uint8_t id[AZ_COMM_ID_BYTES]);
/* An id for an IN-PROCESS communicator of `world` ranks: engines of this process (same or different devices) that
 * call az_comm_init(e, rank, world, id) with it form a world without RCCL.  The id is a magic prefix, a process-unique serial and
 * `world`; it serves one world.  az_comm_init with it returns once all `world` ranks have joined; refused at once
 * (AZ_ERR_BAD_ARGUMENT): a world that differs from the id's, a rank already taken, an id whose world is already complete, an
 * unknown serial or another process's id, an engine that already has a communicator.  Peer access between the members' devices
 * is enabled where the hardware allows it.  The collectives return what the RCCL backend returns, bit for bit, with the same
 * verdicts; the data moves host-synchronously (each rank packs and synchronises its stream, the receivers copy every rank's block
 * on their own streams, two barriers; no stream waits on another engine's event).  Also AZ_ERR_BAD_ARGUMENT on every rank, with
 * one message naming the ranks, never a hang: ranks in different collectives or passing different n to az_allreduce_u64; a
 * rank that left (az_comm_destroy or az_destroy): the other ranks' pending and later collectives fail, a blocked one is woken. */
az_status az_comm_local_id(az_engine* e, int32_t world, uint8_t id[AZ_COMM_ID_BYTES]);
az_status az_comm_init(az_engine* e, int32_t rank, int32_t world, const uint8_t id[AZ_COMM_ID_BYTES]);
az_status az_comm_destroy(az_engine* e);
/* One gather of the packed tuples of `local` (count tuples: states [count,2], pis [count,7], zs [count]; host or device)
 * to dst_rank: an all-gather of the per-rank counts (counts_out [world], may be NULL), then ONE gather of 48-byte packed
 * tuples in rank order.  On dst_rank `gathered` receives them (capacity in, count out; states / pis / zs required, host or
 * device); on other ranks `gathered` may be NULL.  dst_rank = -1: every rank receives (the same exchange as an all-gather: the
 * replicated trainer of the sharded Coach loop).  Collective: every rank of the communicator calls it. */
az_status az_gather_samples(az_engine* e, const az_samples* local, int32_t dst_rank, az_samples* gathered, int64_t* counts_out);
/* In-place sum over the ranks of n (<= 64) u64 counters (the arena's W/L/D; host memory).  Collective. */
az_status az_allreduce_u64(az_engine* e, uint64_t* values, int32_t n);

#ifdef __cplusplus
}
#endif
#endif /* AZ_ENGINE_H */
