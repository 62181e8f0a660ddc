//! Raw bindings of include/az_engine.h (EVERY exported entry point, checked against the header by
//! tests/test_abi_cpu.py) plus a safe `Mi355xNNet` with the reference's `NNet` trait surface (src/nnet.rs:35-45:
//! `new`, `predict`, `train`), an `Mi355xMcts` with `AsyncMcts`'s (`default`, `from_state`, `get_action_prob`,
//! src/async_mcts.rs:27-115), a `SharedMcts` whose slots many episode threads search on at once (az_tree_share), and helpers that replace the self-play fan-out (src/coach.rs:241-272) and the arena gate
//! (src/coach.rs:333-390) with one engine call each.  NOT compiled in this repository (no Rust toolchain here).
#![allow(non_camel_case_types)]
use std::ffi::{CStr, CString};
use std::os::raw::{c_char, c_int};
use std::path::Path;

use ndarray::{Array1, Array2, ArrayView1, ArrayView2, ArrayViewD};

#[repr(C)] pub struct az_engine { _p: [u8; 0] }
#[repr(C)] pub struct az_tree { _p: [u8; 0] }

#[repr(C)] #[derive(Default, Clone, Copy)]
pub struct az_config { pub device: i32, pub max_batch: i32, pub net_channels: i32, pub profile: i32, pub game: i32 }

#[repr(C)] #[derive(Default, Clone, Copy)]
pub struct az_stats {
    pub games: u64, pub moves: u64, pub simulations: u64, pub expansions: u64, pub leaf_evals: u64,
    pub link_hits: u64, pub terminal_hits: u64, pub depth_sum: u64, pub samples: u64, pub net_launches: u64,
    pub net_conv2_ms: f64, pub net_conv2_flops: f64, pub net_total_ms: f64, pub net_total_flops: f64,
    pub tree_ms: f64, pub tree_bytes: f64, pub device_ms: f64,
    pub leaf_rows_requested: u64, pub leaf_rows_executed: u64, pub eval_cache_hits: u64, pub eval_batch_dups: u64,
    pub eval_cache_inserts: u64, pub net_conv3_ms: f64, pub net_conv3_flops: f64, pub net_conv2_bytes: f64,
    pub tree_launches: u64, pub tree_launches_timed: u64, pub tree_arena_allocs: u64,
    pub net_conv4_ms: f64, pub net_conv4_flops: f64, pub net_fc_ms: f64, pub net_fc_flops: f64, pub net_rows_timed: f64,
    pub abandoned_sims: u64, pub net_conv3_image_rows: u64, pub net_conv3_image_launches: u64,
}

#[repr(C)] #[derive(Clone, Copy)]
pub struct az_selfplay_params {
    pub n_games: i32, pub concurrent: i32, pub num_sims: i32, pub temp_threshold: i32,
    pub max_depth: i32, pub cpuct: i32, pub model_id: i32, pub symmetries: i32,
    pub reserve: u64, pub seed: u64, pub first_game_id: u64, pub record_evals: i32, pub num_sim_threads: i32,
}
#[repr(C)]
pub struct az_samples {
    pub capacity: i64, pub count: i64, pub states: *mut u64, pub boards: *mut f32,
    pub pis: *mut f32, pub zs: *mut f32, pub game_len: *mut i32, pub moves: *mut u8,
}
#[repr(C)] #[derive(Clone, Copy)]
pub struct az_arena_params {
    pub num_games: i32, pub num_sims: i32, pub max_depth: i32, pub cpuct: i32,
    pub new_model_id: i32, pub old_model_id: i32, pub reserve: u64, pub seed: u64,
    pub first_game: i32, pub total_games: i32, pub record_evals: i32, pub num_sim_threads: i32,
    pub use_start_board: i32, pub allreduce_wld: i32, pub start_board: [u64; 2],
}

/// flags bit 0 of az_samples_merge: a position and its left-right mirror image merge (the state kept is the canonical one)
pub const AZ_MERGE_CANONICAL: i32 = 1;
/// flags of az_net_train_samples / az_net_train_draw: an epoch has sum(weights) / batch steps (not n / batch); rows are mirrored at random
pub const AZ_TRAIN_EPOCH_BY_WEIGHT: i32 = 1;
pub const AZ_TRAIN_MIRROR: i32 = 2;

/// az_solve: an action that is not legal (or a finished position) / a search that exhausted max_nodes (or a position below min_stones)
pub const AZ_SOLVE_ILLEGAL: i8 = -128;
pub const AZ_SOLVE_UNKNOWN: i8 = 127;
/// classes of az_move_quality
pub const AZ_MQ_SKIPPED: u8 = 0;
pub const AZ_MQ_KEPT: u8 = 1;
pub const AZ_MQ_WIN_TO_DRAW: u8 = 2;
pub const AZ_MQ_WIN_TO_LOSS: u8 = 3;
pub const AZ_MQ_DRAW_TO_LOSS: u8 = 4;
pub const AZ_MQ_UNKNOWN: u8 = 5;

extern "C" {
    // ---- lifecycle
    pub fn az_create(cfg: *const az_config, out: *mut *mut az_engine) -> c_int;
    pub fn az_destroy(e: *mut az_engine);
    pub fn az_last_error(e: *const az_engine) -> *const c_char;
    /// Keys: include/az_engine.h.  "net_fp8" = 1 (default 0) runs conv3 and conv4 of this engine's conv-net forwards on the FP8
    /// (OCP e4m3) matrix path: a numerics class of its own, no new export.
    pub fn az_set_option(e: *mut az_engine, key: *const c_char, value: i64) -> c_int;
    pub fn az_get_stats(e: *mut az_engine, out: *mut az_stats) -> c_int;
    pub fn az_reset_stats(e: *mut az_engine) -> c_int;
    // ---- NNet trait, src/nnet.rs:35-45
    pub fn az_net_set_kind(e: *mut az_engine, model_id: i32, kind: c_int, salt: u64) -> c_int;
    pub fn az_net_free(e: *mut az_engine, model_id: i32) -> c_int;
    /// net_class: AZ_NET_CLASS_ENGINE (-1, follow "net_fp8"), AZ_NET_CLASS_BF16 (0) or AZ_NET_CLASS_FP8 (1); state of the model id
    pub fn az_net_set_class(e: *mut az_engine, model_id: i32, net_class: i32) -> c_int;
    pub fn az_net_get_class(e: *mut az_engine, model_id: i32, stored: *mut i32, effective: *mut i32) -> c_int;
    pub fn az_net_init_random(e: *mut az_engine, model_id: i32, seed: u64) -> c_int;
    pub fn az_net_load(e: *mut az_engine, model_id: i32, path: *const c_char) -> c_int;
    pub fn az_net_save(e: *mut az_engine, model_id: i32, path: *const c_char) -> c_int;
    pub fn az_net_param_count(e: *const az_engine) -> i64;
    pub fn az_net_set_params(e: *mut az_engine, model_id: i32, params: *const f32, n: i64) -> c_int;
    pub fn az_net_get_params(e: *mut az_engine, model_id: i32, params: *mut f32, n: i64) -> c_int;
    pub fn az_net_predict(e: *mut az_engine, model_id: i32, boards: *const f32, B: i32, pi: *mut f32, v: *mut f32) -> c_int;
    pub fn az_net_predict_states(e: *mut az_engine, model_id: i32, states: *const u64, B: i32, pi: *mut f32, v: *mut f32) -> c_int;
    pub fn az_net_train(e: *mut az_engine, prev_id: i32, id: i32, boards: *const f32, pis: *const f32, vs: *const f32, n: i64) -> c_int;
    pub fn az_net_train_history(e: *const az_engine, out: *mut f32, cap_epochs: i32) -> i32;
    pub fn az_net_train_begin(e: *mut az_engine, prev_id: i32) -> c_int;
    pub fn az_net_train_step(e: *mut az_engine, boards: *const f32, pis: *const f32, vs: *const f32, b: i32, mask_seed: u64,
                             apply: i32, loss_out: *mut f32, grads_out: *mut f32) -> c_int;
    pub fn az_net_train_end(e: *mut az_engine, model_id: i32) -> c_int;
    pub fn az_net_train_ema(e: *mut az_engine, model_id: i32) -> c_int;
    pub fn az_net_train_step_info(e: *const az_engine, out: *mut f64) -> c_int;
    /// NNet::train from an az_samples (s.count tuples; s.states, or s.boards when states is null; s.pis; s.zs; host or device): every
    /// batch row is tuple i with probability weights[i] / sum(weights) (u32, null = all ones: az_net_train's draw), flags = AZ_TRAIN_*
    pub fn az_net_train_samples(e: *mut az_engine, prev_id: i32, id: i32, s: *const az_samples, weights: *const u32, flags: i32) -> c_int;
    /// the draw alone for global steps t0 .. t0 + steps: idx_out [steps * "train_batch"], mirror_out the same length (may be null)
    pub fn az_net_train_draw(e: *mut az_engine, n: i64, weights: *const u32, flags: i32, t0: u64, steps: i64, idx_out: *mut i64,
                             mirror_out: *mut u8) -> c_int;
    // held-out loss on the device, the hold-out rule, per-epoch validation inside NNet::train (score: [6], sums: [5] or null)
    pub fn az_net_evaluate(e: *mut az_engine, model_id: i32, s: *const az_samples, weights: *const u32, score: *mut f64, sums: *mut u64,
                           ce: *mut f32, se: *mut f32, kl: *mut f32) -> c_int;
    pub fn az_samples_holdout(e: *mut az_engine, s: *const az_samples, share_e6: i64, seed: u64, held: *mut u8) -> c_int;
    pub fn az_net_train_set_validation(e: *mut az_engine, v: *const az_samples, weights: *const u32) -> c_int;
    pub fn az_net_train_validation(e: *const az_engine, out: *mut f64, cap_epochs: i32, best_epoch: *mut i32) -> i32;
    // ---- AsyncMcts, src/async_mcts.rs:14-115
    pub fn az_tree_create(e: *mut az_engine, n_games: i32, reserve: u64, num_sims: i32, num_threads: i32, max_depth: i32,
                          model_id: i32, cpuct: i32, out: *mut *mut az_tree) -> c_int;
    pub fn az_tree_destroy(t: *mut az_tree);
    pub fn az_tree_reset(t: *mut az_tree, root_states: *const u64) -> c_int;
    pub fn az_tree_get_action_prob(t: *mut az_tree, states: *const u64, temp: f32, seed: u64, first_game_id: u64,
                                   pi: *mut f32, counts: *mut u16, q: *mut f32) -> c_int;
    pub fn az_tree_record_evals(t: *mut az_tree, cap: i32) -> c_int;
    pub fn az_tree_get_evals(t: *mut az_tree, rec_count: *mut i32, states: *mut u64, pis: *mut f32, vs: *mut f32) -> c_int;
    pub fn az_tree_node_counts(t: *mut az_tree, out: *mut u32) -> c_int;
    pub fn az_tree_share(t: *mut az_tree, window_us: i32) -> c_int;
    pub fn az_tree_slot_acquire(t: *mut az_tree, slot: *mut i32) -> c_int;
    pub fn az_tree_slot_release(t: *mut az_tree, slot: i32) -> c_int;
    pub fn az_tree_slot_get_action_prob(t: *mut az_tree, slot: i32, state: *const u64, temp: f32, seed: u64, game_id: u64,
                                        pi: *mut f32, counts: *mut u16, q: *mut f32) -> c_int;
    pub fn az_tree_slot_error(t: *const az_tree, slot: i32) -> *const c_char;
    pub fn az_tree_share_stats(t: *mut az_tree, out: *mut u64) -> c_int;
    /// eta [n,7] of the Dirichlet root noise ("root_noise_eps_e6" / "root_noise_alpha_e6") for root states [n,2] on the streams
    /// (seed, game_ids[i], ply = stones), at the engine's current alpha
    pub fn az_root_noise_eta(e: *mut az_engine, n: i32, seed: u64, game_ids: *const u64, states: *const u64, eta_out: *mut f32) -> c_int;
    pub fn az_tree_get_selected(t: *mut az_tree, actions: *mut i32) -> c_int;
    pub fn az_gumbel_values(e: *mut az_engine, n: i32, seed: u64, game_ids: *const u64, states: *const u64, temp_is_zero: i32, g_out: *mut f32) -> c_int;
    // ---- Coach::execute_episode x many, src/coach.rs:104-157; arena::play_games, src/arena.rs:62-99
    pub fn az_selfplay(e: *mut az_engine, p: *const az_selfplay_params, out: *mut az_samples) -> c_int;
    // the same as a session: the slots stay full across the calls that fetch the episodes (no drain per chunk)
    pub fn az_selfplay_begin(e: *mut az_engine, p: *const az_selfplay_params) -> c_int;
    pub fn az_selfplay_next(e: *mut az_engine, n_games: i32, out: *mut az_samples) -> c_int;
    pub fn az_selfplay_end(e: *mut az_engine) -> c_int;
    /// bit `ply` of mask[i]: that ply of the i-th episode of the last az_selfplay / az_selfplay_next was a full move and became a tuple
    /// ("playout_cap_sims" / "playout_cap_full_e6"; all plies when the playout cap is off)
    pub fn az_selfplay_get_full_plies(e: *mut az_engine, mask: *mut u64) -> c_int;
    pub fn az_selfplay_get_evals(e: *mut az_engine, rec_count: *mut i32, states: *mut u64, pis: *mut f32, vs: *mut f32) -> c_int;
    /// rows of the last az_selfplay / az_selfplay_next in az_samples' order ("selfplay_record_search" = 1): root_q [count] the root value of
    /// each tuple's search, root_prior [count,7] the root's stored priors as the search used them; host or device pointers, either may be null
    pub fn az_selfplay_get_search(e: *mut az_engine, root_q: *mut f32, root_prior: *mut f32) -> c_int;
    /// position averaging: one tuple per distinct position of src (mean pi, mean z, first-occurrence order); flags bit 0 =
    /// AZ_MERGE_CANONICAL merges a position with its mirror image; dst.capacity >= src.count; counts [m] may be null
    pub fn az_samples_merge(e: *mut az_engine, src: *const az_samples, flags: i32, dst: *mut az_samples, counts: *mut u32) -> c_int;
    /// z/q value target: zs_out[i] = (1 - lambda) zs[i] + lambda root_q[i] in f32, lambda = lambda_e6 / 1e6 in 0 .. 1000000; zs_out may be zs
    pub fn az_samples_blend_z(e: *mut az_engine, n: i64, zs: *const f32, root_q: *const f32, lambda_e6: i64, zs_out: *mut f32) -> c_int;
    /// surprise resampling: tuple i of src written counts[i] times into dst (capacity >= 2 src.count; may be null), a share share_e6 / 1e6 of
    /// the weight in proportion to kl[i] = KL(pi_i || priors_i); priors [n,7]; counts [n] and kl [n] may be null
    pub fn az_samples_surprise(e: *mut az_engine, src: *const az_samples, priors: *const f32, share_e6: i64, seed: u64,
                               dst: *mut az_samples, counts: *mut u32, kl: *mut f32) -> c_int;
    /// exact endgame solver: every root action of n canonical positions; move_values [n,7] in {-1, 0, +1, AZ_SOLVE_ILLEGAL, AZ_SOLVE_UNKNOWN},
    /// values [n] and nodes [n,7] may be null; tt_log2 0 or 8..16, max_lanes 0 or a multiple of 64
    pub fn az_solve(e: *mut az_engine, states: *const u64, n: i32, max_nodes: u32, min_stones: i32, tt_log2: i32, max_lanes: i32,
                    move_values: *mut i8, values: *mut i8, nodes: *mut u32) -> c_int;
    /// move-quality report of n recorded games (start_boards may be null): ply_class [n,42] of AZ_MQ_*, ply_value [n,42] may be null
    pub fn az_move_quality(e: *mut az_engine, start_boards: *const u64, game_len: *const i32, moves: *const u8, n: i32,
                           max_nodes: u32, min_stones: i32, tt_log2: i32, max_lanes: i32, ply_class: *mut u8, ply_value: *mut i8) -> c_int;
    pub fn az_arena(e: *mut az_engine, p: *const az_arena_params, out_wld: *mut u64, results: *mut i8) -> c_int;
    pub fn az_arena_get_evals(e: *mut az_engine, which: i32, rec_count: *mut i32, states: *mut u64, pis: *mut f32, vs: *mut f32) -> c_int;
    pub fn az_arena_get_moves(e: *mut az_engine, game_len: *mut i32, moves: *mut u8) -> c_int;
    // paired arena openings ("arena_opening_plies"): the opening book, and where the games of the last az_arena started
    pub fn az_arena_set_opening_book(e: *mut az_engine, boards: *const u64, n: i32) -> c_int;
    pub fn az_arena_get_openings(e: *mut az_engine, boards: *mut u64, len: *mut i32, moves: *mut u8) -> c_int;
    // one batched round robin of num_models models: wld [K][K][3], results [pairs * games_per_pair] in tournament order (game g of pair p of
    // the pairs (i, j), i < j, is game g of az_arena(model_ids[i], model_ids[j]) bit for bit); plain scalars, no new #[repr(C)] type
    pub fn az_tournament(e: *mut az_engine, model_ids: *const i32, num_models: i32, games_per_pair: i32, num_sims: i32, max_depth: i32, cpuct: i32, num_sim_threads: i32, reserve: u64, seed: u64, wld: *mut u64, results: *mut i8) -> c_int;
    // Bradley-Terry ratings from that matrix (no engine, no GPU): elo [K] with mean 0, elo_se [K] (approximate; may be null), sweeps (may be null)
    pub fn az_rating_fit(wld: *const u64, K: i32, prior_games: f64, elo: *mut f64, elo_se: *mut f64, sweeps: *mut i32) -> c_int;
    // ---- the collective of the sharded Coach loop (one process per GPU; RCCL on the engine's stream)
    pub fn az_comm_unique_id(e: *mut az_engine, id: *mut u8) -> c_int;
    // an in-process communicator: engines of this process, one host thread each, form one world without RCCL
    pub fn az_comm_local_id(e: *mut az_engine, world: i32, id: *mut u8) -> c_int;
    pub fn az_comm_init(e: *mut az_engine, rank: i32, world: i32, id: *const u8) -> c_int;
    pub fn az_comm_destroy(e: *mut az_engine) -> c_int;
    pub fn az_gather_samples(e: *mut az_engine, local: *const az_samples, dst_rank: i32, gathered: *mut az_samples, counts_out: *mut i64) -> c_int;
    pub fn az_allreduce_u64(e: *mut az_engine, values: *mut u64, n: i32) -> c_int;
}

/// The reference panics on every error (unwrap/assert!); keep that behaviour.
pub fn check(e: *const az_engine, rc: c_int) {
    if rc != 0 {
        let msg = unsafe { CStr::from_ptr(az_last_error(e)) }.to_string_lossy().into_owned();
        panic!("az_engine status {}: {}", rc, msg);
    }
}

/// `impl NNet` (src/nnet.rs:35-45) over the engine; drop-in for `PythonNNet` (examples/utils/python_nnet.rs).
pub struct Mi355xNNet { pub e: *mut az_engine }

impl Mi355xNNet {
    pub fn new<P: AsRef<Path>>(checkpoint: P) -> Self {                               // NNet::new, src/nnet.rs:36
        let mut e = std::ptr::null_mut();
        assert_eq!(unsafe { az_create(&az_config::default(), &mut e) }, 0, "az_create failed");
        let p = CString::new(checkpoint.as_ref().join("0.aznet").to_str().unwrap()).unwrap();
        if unsafe { az_net_load(e, 0, p.as_ptr()) } != 0 { check(e, unsafe { az_net_init_random(e, 0, 0) }); }
        Mi355xNNet { e }
    }
    /// NNet::predict(board [B,2,6,7], model_id) -> (pi [B,7], v [B]), src/nnet.rs:40-44
    pub fn predict(&self, board: ArrayViewD<f32>, model_id: usize) -> (Array2<f32>, Array1<f32>) {
        let b = board.shape()[0];
        let x = board.as_standard_layout();
        let (mut pi, mut v) = (Array2::<f32>::zeros((b, 7)), Array1::<f32>::zeros(b));
        check(self.e, unsafe { az_net_predict(self.e, model_id as i32, x.as_ptr(), b as i32, pi.as_mut_ptr(), v.as_mut_ptr()) });
        (pi, v)
    }
    /// NNet::train(examples = (boards [N,2,6,7], pis [N,7], vs [N]), previous_model_id, model_id), src/nnet.rs:38:
    /// the reference's recipe on the device (f32 MFMA trainer), result stored under model_id.
    pub fn train(&mut self, boards: ArrayViewD<f32>, pis: ArrayView2<f32>, vs: ArrayView1<f32>, previous_model_id: usize, model_id: usize) {
        let (b, p, v) = (boards.as_standard_layout(), pis.as_standard_layout(), vs.as_standard_layout());
        check(self.e, unsafe { az_net_train(self.e, previous_model_id as i32, model_id as i32, b.as_ptr(), p.as_ptr(), v.as_ptr(), v.len() as i64) });
    }
    /// Drop a superseded model id (Coach::learn moves to model_id + 1 per accepted iteration, src/coach.rs:383-390).
    pub fn free(&mut self, model_id: usize) { check(self.e, unsafe { az_net_free(self.e, model_id as i32) }); }
    /// Pin one model's numerics class (AZ_NET_CLASS_*); -1 hands it back to the engine's "net_fp8" option.
    pub fn set_class(&mut self, model_id: usize, net_class: i32) { check(self.e, unsafe { az_net_set_class(self.e, model_id as i32, net_class) }); }
    /// (stored class, effective class: 0 bf16 / 1 fp8)
    pub fn class(&self, model_id: usize) -> (i32, i32) {
        let (mut s, mut f) = (0i32, 0i32);
        check(self.e, unsafe { az_net_get_class(self.e, model_id as i32, &mut s, &mut f) });
        (s, f)
    }
}
impl Drop for Mi355xNNet { fn drop(&mut self) { unsafe { az_destroy(self.e) } } }

/// n x `AsyncMcts<ConnectFourGame>` (src/async_mcts.rs:14-115) as one tree batch on the device.
pub struct Mi355xMcts { pub e: *mut az_engine, pub t: *mut az_tree, pub n_games: usize }

impl Mi355xMcts {
    /// AsyncMcts::default(reserve_space, num_sims, num_threads, max_depth, model_id, cpuct, ..), src/async_mcts.rs:27-48;
    /// num_threads > 1 = several simulations in flight per tree as a deterministic lock-step schedule (az_engine.h)
    pub fn default(e: *mut az_engine, n_games: usize, reserve_space: usize, num_sims: usize, num_threads: usize, max_depth: usize, model_id: usize, cpuct: i32) -> Self {
        let mut t = std::ptr::null_mut();
        check(e, unsafe { az_tree_create(e, n_games as i32, reserve_space as u64, num_sims as i32, num_threads as i32, max_depth as i32, model_id as i32, cpuct, &mut t) });
        Mi355xMcts { e, t, n_games }
    }
    /// AsyncMcts::from_state(s, ..), src/async_mcts.rs:50-72: every tree re-rooted at its canonical bitboards [n_games, 2]
    pub fn from_state(e: *mut az_engine, root_states: &[u64], reserve_space: usize, num_sims: usize, num_threads: usize, max_depth: usize, model_id: usize, cpuct: i32) -> Self {
        let m = Self::default(e, root_states.len() / 2, reserve_space, num_sims, num_threads, max_depth, model_id, cpuct);
        check(e, unsafe { az_tree_reset(m.t, root_states.as_ptr()) });
        m
    }
    /// get_action_prob(&self, s, temp, episode_id, rng) for every tree, src/async_mcts.rs:74-115: pi [n_games, 7]
    pub fn get_action_prob(&self, states: &[u64], temp: f32, seed: u64, first_game_id: u64) -> Array2<f32> {
        let mut pi = Array2::<f32>::zeros((self.n_games, 7));
        check(self.e, unsafe { az_tree_get_action_prob(self.t, states.as_ptr(), temp, seed, first_game_id, pi.as_mut_ptr(),
                                                       std::ptr::null_mut(), std::ptr::null_mut()) });
        pi
    }
    /// NodeStore::len per tree, src/node.rs:372-374
    pub fn node_counts(&self) -> Vec<u32> {
        let mut out = vec![0u32; self.n_games];
        check(self.e, unsafe { az_tree_node_counts(self.t, out.as_mut_ptr()) });
        out
    }
}
impl Drop for Mi355xMcts { fn drop(&mut self) { unsafe { az_tree_destroy(self.t) } } }

/// One shared tree batch for many episode threads (az_tree_share): the rayon pool of src/coach.rs:202-205, :241-272 keeps
/// `execute_episode`, each thread takes a slot (`mcts()`, one `AsyncMcts::default` per episode), and the engine coalesces the
/// threads' `get_action_prob` calls into batched searches -- the role of `inference_thread` (src/async_mcts.rs:117-189).
/// While slots are in use, make no other call on the engine; drop every `SharedSlot` before the `SharedMcts`.
pub struct SharedMcts { pub t: *mut az_tree }
// The slot calls are made from many threads at once by design (include/az_engine.h threading contract).
unsafe impl Send for SharedMcts {}
unsafe impl Sync for SharedMcts {}

impl SharedMcts {
    /// `slots` trees of AsyncMcts::default(reserve_space, num_sims, num_threads, max_depth, model_id, cpuct, ..);
    /// window_us = 0: a batch starts when every held slot waits, > 0: also when the oldest request is that old
    pub fn new(e: *mut az_engine, slots: usize, reserve_space: usize, num_sims: usize, num_threads: usize, max_depth: usize, model_id: usize,
               cpuct: i32, window_us: i32) -> Self {
        let mut t = std::ptr::null_mut();
        check(e, unsafe { az_tree_create(e, slots as i32, reserve_space as u64, num_sims as i32, num_threads as i32, max_depth as i32, model_id as i32, cpuct, &mut t) });
        check(e, unsafe { az_tree_share(t, window_us) });
        SharedMcts { t }
    }
    /// AsyncMcts::default on a free slot; the slot goes back when the guard drops
    pub fn mcts(&self) -> SharedSlot<'_> {
        let mut slot = -1i32;
        let rc = unsafe { az_tree_slot_acquire(self.t, &mut slot) };
        assert_eq!(rc, 0, "az_tree_slot_acquire: every slot is held (status {})", rc);
        SharedSlot { owner: self, slot }
    }
    /// [batches, requests, largest batch, batches started by the window]
    pub fn stats(&self) -> [u64; 4] {
        let mut s = [0u64; 4];
        assert_eq!(unsafe { az_tree_share_stats(self.t, s.as_mut_ptr()) }, 0);
        s
    }
}
impl Drop for SharedMcts { fn drop(&mut self) { unsafe { az_tree_destroy(self.t) } } }

/// One thread's `AsyncMcts` on a slot of a `SharedMcts`.
pub struct SharedSlot<'a> { owner: &'a SharedMcts, slot: i32 }

impl SharedSlot<'_> {
    /// get_action_prob(&self, s, temp, episode_id, rng), src/async_mcts.rs:74-115, for this slot's tree: blocks until its batch ran;
    /// `state` = canonical bitboards [2]; tie-break stream (seed, episode_id, ply = stones)
    pub fn get_action_prob(&self, state: &[u64; 2], temp: f32, episode_id: u64, seed: u64) -> [f32; 7] {
        let mut pi = [0f32; 7];
        let rc = unsafe { az_tree_slot_get_action_prob(self.owner.t, self.slot, state.as_ptr(), temp, seed, episode_id, pi.as_mut_ptr(),
                                                       std::ptr::null_mut(), std::ptr::null_mut()) };
        if rc != 0 {
            let msg = unsafe { CStr::from_ptr(az_tree_slot_error(self.owner.t, self.slot)) }.to_string_lossy().into_owned();
            panic!("az_engine status {}: {}", rc, msg);
        }
        pi
    }
}
impl Drop for SharedSlot<'_> { fn drop(&mut self) { unsafe { az_tree_slot_release(self.owner.t, self.slot); } } }

/// Counters since az_create / the last reset (SURVEY.md 8b "Introspection").
pub fn stats(e: *mut az_engine) -> az_stats {
    let mut s = az_stats::default();
    check(e, unsafe { az_get_stats(e, &mut s) });
    s
}

/// Replaces the rayon fan-out of `execute_episode` (src/coach.rs:241-272): returns (boards [N,2,6,7], pis [N,7], vs [N]).
pub fn self_play(e: *mut az_engine, p: &az_selfplay_params) -> (Vec<f32>, Vec<f32>, Vec<f32>) {
    let cap = p.n_games as usize * 42 * if p.symmetries != 0 { 2 } else { 1 };
    let (mut boards, mut pis, mut zs) = (vec![0f32; cap * 84], vec![0f32; cap * 7], vec![0f32; cap]);
    let mut out = az_samples { capacity: cap as i64, count: 0, states: std::ptr::null_mut(), boards: boards.as_mut_ptr(),
                               pis: pis.as_mut_ptr(), zs: zs.as_mut_ptr(), game_len: std::ptr::null_mut(), moves: std::ptr::null_mut() };
    check(e, unsafe { az_selfplay(e, p, &mut out) });
    let n = out.count as usize;
    boards.truncate(n * 84); pis.truncate(n * 7); zs.truncate(n);
    (boards, pis, zs)
}

/// The id of an in-process communicator of `world` ranks (az_comm_local_id): hand the same 128 bytes to the `world` engines of
/// this process, each on its own thread, and call `az_comm_init(e, rank, world, id)` on every one of them.
pub fn comm_local_id(e: *mut az_engine, world: i32) -> [u8; 128] {
    let mut id = [0u8; 128];
    check(e, unsafe { az_comm_local_id(e, world, id.as_mut_ptr()) });
    id
}

/// The ONE exchange of a sharded episode batch (each rank played `p.first_game_id ..` of the global episode ids): this rank's
/// (states [n,2], pis [n,7], zs [n]) go to `dst_rank`, which gets everybody's tuples in rank order (else empty vectors);
/// `dst_rank = -1`: every rank receives everything.  `global_episodes` = the number of episodes of the WHOLE batch over all ranks:
/// a receiving rank sizes its buffers from the hard bound 42 plies per episode (uneven shards make any bound derived from the
/// local count too small; the library checks the capacity on every rank before anything is posted, so a wrong bound is an error
/// on all ranks, never a hang).
pub fn gather_samples(e: *mut az_engine, states: &mut [u64], pis: &mut [f32], zs: &mut [f32], rank: i32, world: i32, dst_rank: i32,
                      global_episodes: usize) -> (Vec<u64>, Vec<f32>, Vec<f32>) {
    let n = zs.len();
    let local = az_samples { capacity: n as i64, count: n as i64, states: states.as_mut_ptr(), boards: std::ptr::null_mut(),
                             pis: pis.as_mut_ptr(), zs: zs.as_mut_ptr(), game_len: std::ptr::null_mut(), moves: std::ptr::null_mut() };
    let mut counts = vec![0i64; world as usize];
    if dst_rank >= 0 && rank != dst_rank {
        check(e, unsafe { az_gather_samples(e, &local, dst_rank, std::ptr::null_mut(), counts.as_mut_ptr()) });
        return (vec![], vec![], vec![]);
    }
    let cap = global_episodes * 42;
    let (mut gs, mut gp, mut gz) = (vec![0u64; cap * 2], vec![0f32; cap * 7], vec![0f32; cap]);
    let mut g = az_samples { capacity: cap as i64, count: 0, states: gs.as_mut_ptr(), boards: std::ptr::null_mut(),
                             pis: gp.as_mut_ptr(), zs: gz.as_mut_ptr(), game_len: std::ptr::null_mut(), moves: std::ptr::null_mut() };
    check(e, unsafe { az_gather_samples(e, &local, dst_rank, &mut g, counts.as_mut_ptr()) });
    let m = g.count as usize;
    gs.truncate(m * 2); gp.truncate(m * 7); gz.truncate(m);
    (gs, gp, gz)
}

/// Replaces `play_games` + the tally of src/coach.rs:365-381: (nwins, pwins, draws) for the new model.
pub fn arena(e: *mut az_engine, p: &az_arena_params) -> (u64, u64, u64) {
    let mut wld = [0u64; 3];
    check(e, unsafe { az_arena(e, p, wld.as_mut_ptr(), std::ptr::null_mut()) });
    (wld[0], wld[1], wld[2])
}
