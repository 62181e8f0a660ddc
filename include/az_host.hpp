// az_host.hpp -- C++ host-side mirror of the reference's plugin interface above the C ABI.
//
// The reference is Rust; no Rust toolchain exists in this build environment, so the host side of the
// drop-in is written in C++ with the reference's names, argument meaning and error behaviour (a Rust
// `panic!` becomes a thrown az_host::Panic):
//   Game trait            src/game.rs:10-28           -> ConnectFourGame (connect_four_game.rs:81-238)
//   NNet trait            src/nnet.rs:35-45           -> NNet, Mi355xNNet (az_net_* entry points)
//   AsyncMcts<G>          src/async_mcts.rs:14-115    -> AsyncMcts (az_tree_* entry points, one tree)
//   inference_thread      src/async_mcts.rs:117-189   -> SharedMcts (az_tree_share: one slot per host thread, batched searches)
//   arena::play_game(s)   src/arena.rs:7-99           -> play_game, play_games (closures, Heap's order)
//   Coach::execute_episode src/coach.rs:104-157       -> execute_episode
//   Coach::setup / learn  src/coach.rs:38-103, :169-396 -> Coach (az_selfplay, az_net_train, az_arena; one call each)
// Header-only; links against libaz_engine.so.  Nothing here touches oracle/.
#pragma once
#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <deque>
#include <filesystem>
#include <functional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "az_engine.h"
#include "az_reanalyse.h"
#include "az_search_stop.h"
// Bound weakly, for one reason: the CPU tests link this header against recording doubles of the ABI that define only the entries a
// Coach used before position averaging (tests/cpp/test_root_noise_host_cpu.cpp and its like), and Coach::learn names az_samples_merge.
// With a real engine library the symbol resolves as any other; without it Coach::merge_positions panics instead of calling through null.
#pragma weak az_samples_merge
// The same holds for what Coach::solve_min_stones reaches: with it off (the default) none of these is called.
#pragma weak az_solve
#pragma weak az_move_quality
#pragma weak az_arena_get_moves
#pragma weak az_arena_get_openings
#pragma weak az_allreduce_u64
// Coach::ema_decay: with it 0 (the default) it is never called.
#pragma weak az_net_train_ema
// az_host::tournament / az_host::rating_fit: no Coach calls them.
#pragma weak az_tournament
#pragma weak az_rating_fit
// Coach::merge_weighted / az_host::train_samples / az_host::train_draw: with merge_weighted off (the default) no Coach calls them.
#pragma weak az_net_train_samples
#pragma weak az_net_train_draw
// Coach::value_target_q / Coach::surprise_share / az_host::selfplay_search / blend_z / surprise: with both fields 0 (the default) no Coach calls them.
#pragma weak az_selfplay_get_search
#pragma weak az_samples_blend_z
#pragma weak az_samples_surprise
// Coach::validation_share / az_host::evaluate / samples_holdout / train_set_validation / train_validation: with validation_share 0 (the
// default) no Coach calls them.
#pragma weak az_net_evaluate
#pragma weak az_samples_holdout
#pragma weak az_net_train_set_validation
#pragma weak az_net_train_validation
// Coach::reanalyse_sims / az_host::reanalyse: with reanalyse_sims 0 (the default) no Coach calls it.
#pragma weak az_reanalyse
// az_host::set_search_stop / search_stop_stats: no default path calls them.
#pragma weak az_search_stop_set
#pragma weak az_search_stop_get
#pragma weak az_search_stop_stats

namespace az_host {

struct Panic : std::runtime_error { using std::runtime_error::runtime_error; };

using Policy = std::vector<float>;          // nnet.rs:17
using BoardFeatures = std::vector<float>;   // nnet.rs:9, [2,6,7] row-major
struct TrainingSample { BoardFeatures board; Policy pi; float v; };   // nnet.rs:22-27

// ---- Game: Connect Four on absolute bitboards (player +1 / -1) ------------------------------------------
class ConnectFourGame {
  public:
    uint64_t plus = 0, minus = 0;           // stones of player +1 / -1; bit(col,row) = col*7+row, row 0 = bottom
    static constexpr int H = 6, W = 7;      // connect_four_game.rs:13-14
    static constexpr float DRAW_EPS = 1e-4f;

    static ConnectFourGame get_init_board() { return {}; }
    static std::vector<size_t> get_feature_shape() { return {2, 6, 7}; }
    std::pair<ConnectFourGame, int8_t> get_next_state(int8_t player, uint8_t action) const {
        const uint64_t mask = plus | minus;
        const uint64_t nb = (mask + (1ull << (action * 7))) & (0x3Full << (action * 7));
        if (!nb) throw Panic("C4 move into a full column");           // debug_assert, connect_four_game.rs:98
        ConnectFourGame n = *this;
        (player == 1 ? n.plus : n.minus) |= nb;
        return {n, (int8_t)-player};
    }
    std::array<uint8_t, 7> get_valid_moves(int8_t) const {
        std::array<uint8_t, 7> v{};
        for (int c = 0; c < W; ++c) v[c] = ((plus | minus) >> (c * 7 + 5)) & 1 ? 0 : 1;
        return v;
    }
    float get_game_ended(int8_t player) const {
        if (four(plus)) return player == 1 ? 1.f : -1.f;
        if (four(minus)) return player == -1 ? 1.f : -1.f;
        for (int c = 0; c < W; ++c) if (!(((plus | minus) >> (c * 7 + 5)) & 1)) return 0.f;
        return DRAW_EPS;
    }
    ConnectFourGame get_canonical_form(int8_t player) const {         // side to move becomes +1 (B5)
        ConnectFourGame n;
        n.plus = player == 1 ? plus : minus;
        n.minus = player == 1 ? minus : plus;
        return n;
    }
    std::vector<std::pair<ConnectFourGame, Policy>> get_symmetries(const Policy& pi) const {
        ConnectFourGame f;
        for (int c = 0; c < W; ++c) {
            f.plus |= ((plus >> (c * 7)) & 0x7F) << ((6 - c) * 7);
            f.minus |= ((minus >> (c * 7)) & 0x7F) << ((6 - c) * 7);
        }
        return {{*this, pi}, {f, Policy(pi.rbegin(), pi.rend())}};
    }
    float eval_heuristic() const { return 0.f; }
    BoardFeatures to_features() const {                                // [2,6,7], row 0 = top (S8)
        BoardFeatures f(84, 0.f);
        for (int r = 0; r < H; ++r)
            for (int c = 0; c < W; ++c) {
                const uint64_t bit = 1ull << (c * 7 + (5 - r));
                if (plus & bit) f[r * 7 + c] = 1.f;
                if (minus & bit) f[42 + r * 7 + c] = 1.f;
            }
        return f;
    }
    bool operator==(const ConnectFourGame& o) const { return plus == o.plus && minus == o.minus; }

  private:
    static bool four(uint64_t b) {
        for (int d : {1, 7, 6, 8}) { uint64_t m = b & (b >> d); if (m & (m >> (2 * d))) return true; }
        return false;
    }
};

// the four search parameters of az_solve / az_move_quality (include/az_engine.h)
struct SolveParams { uint32_t max_nodes = 1u << 20; int32_t min_stones = 0, tt_log2 = 12, max_lanes = 0; };

// ---- engine handle + NNet ----------------------------------------------------------------------------------
class Engine {
  public:
    using SolveParams = az_host::SolveParams;
    explicit Engine(int device = 0, int max_batch = 8192, int channels = 512) {
        az_config cfg{device, max_batch, channels, 0, 0};
        if (az_create(&cfg, &e_) != AZ_OK) throw Panic("az_create failed");
    }
    ~Engine() { az_destroy(e_); }
    Engine(const Engine&) = delete;
    Engine& operator=(const Engine&) = delete;
    az_engine* raw() const { return e_; }
    void check(int rc) const { if (rc != AZ_OK) throw Panic(std::string(az_last_error(e_))); }
    // az_net_set_class / az_net_get_class: the numerics class of ONE conv model (ENGINE = the engine's "net_fp8" option decides)
    void net_set_class(size_t model_id, az_net_class c) { check(az_net_set_class(e_, (int32_t)model_id, (int32_t)c)); }
    std::pair<int32_t, int32_t> net_class(size_t model_id) const {     // (stored az_net_class, effective: 0 bf16 / 1 fp8)
        int32_t stored = 0, effective = 0;
        check(az_net_get_class(e_, (int32_t)model_id, &stored, &effective));
        return {stored, effective};
    }
    // Dirichlet root noise of self-play and the tree calls, never of the arena ("root_noise_eps_e6" / "root_noise_alpha_e6",
    // include/az_engine.h): prior <- (1 - eps) * prior + eps * eta at the root, eta ~ Dirichlet(alpha).  eps = 0 switches it off
    // "eval_mirror" (include/az_engine.h, default off): conv models answer on the canonical orientation of a position, pi un-mirrored
    void set_eval_mirror(bool on) { check(az_set_option(e_, "eval_mirror", on ? 1 : 0)); }
    // "selfplay_record_search" (include/az_engine.h): self-play keeps the root value and the root's stored priors of every move
    // (az_host::selfplay_search reads them); never the arena or the tree calls
    void set_record_search(bool on) { check(az_set_option(e_, "selfplay_record_search", on ? 1 : 0)); }
    void set_root_noise(double eps, double alpha = 1.0) {
        check(az_set_option(e_, "root_noise_alpha_e6", (int64_t)std::llround(alpha * 1e6)));
        check(az_set_option(e_, "root_noise_eps_e6", (int64_t)std::llround(eps * 1e6)));
    }
    // Playout cap randomization of self-play, never of the arena or the tree calls ("playout_cap_sims" / "playout_cap_full_e6",
    // include/az_engine.h): a share p_full of an episode's moves is searched with the full num_sims and recorded, every other move with
    // `sims` simulations and only played.  sims = 0 switches it off
    void set_playout_cap(int64_t sims, double p_full = 0.25) {
        check(az_set_option(e_, "playout_cap_full_e6", (int64_t)std::llround(p_full * 1e6)));
        check(az_set_option(e_, "playout_cap_sims", sims));
    }
    // Forced playouts at the root and policy target pruning ("forced_playouts_k_e6" / "policy_prune", include/az_engine.h) on every move
    // root noise can apply to (under a playout cap the full moves only), never the arena.  k = 0 switches both off
    void set_forced_playouts(double k, bool prune = false) {
        check(az_set_option(e_, "policy_prune", prune ? 1 : 0));
        check(az_set_option(e_, "forced_playouts_k_e6", (int64_t)std::llround(k * 1e6)));
    }
    // Gumbel root search with sequential halving ("gumbel_m" / "gumbel_c_visit_e6" / "gumbel_c_scale_e6", include/az_engine.h) on every move
    // root noise can apply to (under a playout cap the full moves only), never the arena or the slot calls.  m = 0 switches it off
    void set_gumbel(int64_t m, double c_visit = 50.0, double c_scale = 1.0) {
        check(az_set_option(e_, "gumbel_c_visit_e6", (int64_t)std::llround(c_visit * 1e6)));
        check(az_set_option(e_, "gumbel_c_scale_e6", (int64_t)std::llround(c_scale * 1e6)));
        check(az_set_option(e_, "gumbel_m", m));
    }
    // The opt-in optimiser rules of NNet::train, read by the next az_net_train / az_net_train_begin ("train_weight_decay_e9",
    // "train_clip_norm_e6", "train_lr_warmup_steps", "train_lr_decay", "train_lr_floor_e6", "train_lr_total_steps", "train_ema_decay_e9",
    // include/az_engine.h).  Everything 0 switches them off
    void set_train_optim(double weight_decay = 0.0, double clip_norm = 0.0, int64_t lr_warmup_steps = 0, int64_t lr_decay = 0, double lr_floor = 0.0,
                         double ema_decay = 0.0, int64_t lr_total_steps = 0) {
        check(az_set_option(e_, "train_weight_decay_e9", (int64_t)std::llround(weight_decay * 1e9)));
        check(az_set_option(e_, "train_clip_norm_e6", (int64_t)std::llround(clip_norm * 1e6)));
        check(az_set_option(e_, "train_lr_warmup_steps", lr_warmup_steps));
        check(az_set_option(e_, "train_lr_decay", lr_decay));
        check(az_set_option(e_, "train_lr_floor_e6", (int64_t)std::llround(lr_floor * 1e6)));
        check(az_set_option(e_, "train_lr_total_steps", lr_total_steps));
        check(az_set_option(e_, "train_ema_decay_e9", (int64_t)std::llround(ema_decay * 1e9)));
    }
    // Paired arena openings ("arena_opening_plies", include/az_engine.h): arena game g and its seat-swapped twin start from the same
    // position, `plies` random quiet plies (even, 2 .. 12) onto the pair's base; never self-play or the tree calls.  0 switches them off
    void set_arena_openings(int64_t plies) { check(az_set_option(e_, "arena_opening_plies", plies)); }
    // az_arena_set_opening_book: boards [n][2] {first seat's stones, second seat's stones}; pair p starts from entry p % n.  Empty clears it
    void arena_set_opening_book(const std::vector<uint64_t>& boards) {
        check(az_arena_set_opening_book(e_, boards.empty() ? nullptr : boards.data(), (int32_t)(boards.size() / 2)));
    }
    // az_selfplay_get_full_plies: bit `ply` of word i = that ply of the i-th episode of the last az_selfplay / az_selfplay_next call
    // (n_games episodes) was a full move and became a tuple
    std::vector<uint64_t> selfplay_full_plies(size_t n_games) const {
        std::vector<uint64_t> mask(n_games, 0);
        check(az_selfplay_get_full_plies(e_, mask.data()));
        return mask;
    }
    // az_solve (include/az_engine.h): the exact outcome of every root action of n canonical positions {mine, theirs}
    struct Solved { std::vector<int8_t> move_values, values; std::vector<uint32_t> nodes; };     // [n][7], [n], [n][7]
    Solved solve(const std::vector<uint64_t>& states, const SolveParams& p = SolveParams()) const {
        if (!az_solve) throw Panic("solve: the linked engine library has no az_solve");
        const size_t n = states.size() / 2;
        Solved r{std::vector<int8_t>(n * 7), std::vector<int8_t>(n), std::vector<uint32_t>(n * 7)};
        check(az_solve(e_, states.data(), (int32_t)n, p.max_nodes, p.min_stones, p.tt_log2, p.max_lanes, r.move_values.data(), r.values.data(), r.nodes.data()));
        return r;
    }
    // az_move_quality: ply_class [n][AZ_MAX_PLIES] of AZ_MQ_* for n recorded games (start_boards [n][2] or nullptr = the initial board)
    std::vector<uint8_t> move_quality(const uint64_t* start_boards, const std::vector<int32_t>& game_len, const std::vector<uint8_t>& moves,
                                      const SolveParams& p, std::vector<int8_t>* ply_value = nullptr) const {
        if (!az_move_quality) throw Panic("move_quality: the linked engine library has no az_move_quality");
        const size_t n = game_len.size();
        std::vector<uint8_t> cls(n * AZ_MAX_PLIES);
        if (ply_value) ply_value->assign(n * AZ_MAX_PLIES, 0);
        check(az_move_quality(e_, start_boards, game_len.data(), moves.data(), (int32_t)n, p.max_nodes, p.min_stones, p.tt_log2, p.max_lanes,
                              cls.data(), ply_value ? ply_value->data() : nullptr));
        return cls;
    }

  private:
    az_engine* e_ = nullptr;
};

// ---- az_tournament / az_rating_fit (include/az_engine.h): one batched round robin of K models, and ratings from its result matrix ----------
// The pairs are (i, j), i < j, in lexicographic order; game g of pair p is bit for bit game g of az_arena {num_games = games_per_pair,
// new_model_id = model_ids[i], old_model_id = model_ids[j], the same search parameters} and has index p * games_per_pair + g.  Paired
// openings (Engine::set_arena_openings / arena_set_opening_book) apply as to the arena: switch them on first.
struct TournamentParams {
    std::vector<int32_t> model_ids;                  // K = 2 .. 16, pairwise distinct
    int32_t games_per_pair = 2;                      // even: half per seating
    int32_t num_sims = 25, max_depth = 1000, cpuct = 1, num_sim_threads = 1;
    uint64_t reserve = 1000000, seed = 0;
};
struct TournamentResult {
    size_t K = 0, games = 0;
    std::vector<uint64_t> wld;                       // [K][K][3]: wld[i][j] = {W, L, D} from model i's side
    std::vector<int8_t> results;                     // [games] +1: the first seat won
    std::vector<int32_t> game_len;                   // [games]
    std::vector<uint8_t> moves;                      // [games][AZ_MAX_PLIES]
};
inline TournamentResult tournament(const Engine& e, const TournamentParams& p) {
    if (!az_tournament || !az_arena_get_moves) throw Panic("tournament: the linked engine library has no az_tournament");
    TournamentResult r;
    r.K = p.model_ids.size();
    r.games = r.K * (r.K > 0 ? r.K - 1 : 0) / 2 * (size_t)std::max(p.games_per_pair, 0);
    r.wld.assign(r.K * r.K * 3, 0);
    r.results.assign(std::max<size_t>(r.games, 1), 0);
    e.check(az_tournament(e.raw(), p.model_ids.data(), (int32_t)r.K, p.games_per_pair, p.num_sims, p.max_depth, p.cpuct, p.num_sim_threads, p.reserve,
                          p.seed, r.wld.data(), r.results.data()));
    r.results.resize(r.games);
    r.game_len.assign(r.games, 0);
    r.moves.assign(r.games * AZ_MAX_PLIES, 0);
    e.check(az_arena_get_moves(e.raw(), r.game_len.data(), r.moves.data()));
    return r;
}
// Bradley-Terry ratings (a draw = half a win): elo [K] with mean 0 and elo_se [K], the diagonal Fisher approximation.  Needs no engine
struct Ratings { std::vector<double> elo, elo_se; int32_t sweeps = 0; };
// NNet::train on n tuples whose batch rows are drawn in proportion to `weights` (az_net_train_samples; nullptr = all ones), from states
// [n,2] -- the device builds each batch's planes from the bits -- or, with states nullptr, from boards [n,2,6,7].  flags: AZ_TRAIN_*.
inline void train_samples(const Engine& e, size_t prev_id, size_t id, int64_t n, const uint64_t* states, const float* boards, const float* pis,
                          const float* zs, const uint32_t* weights = nullptr, int32_t flags = 0) {
    if (!az_net_train_samples) throw Panic("train_samples: the linked engine library has no az_net_train_samples");
    az_samples s{};
    s.capacity = n; s.count = n;
    s.states = const_cast<uint64_t*>(states); s.boards = const_cast<float*>(boards);
    s.pis = const_cast<float*>(pis); s.zs = const_cast<float*>(zs);
    e.check(az_net_train_samples(e.raw(), (int32_t)prev_id, (int32_t)id, &s, weights, flags));
}
// The rows az_net_train_samples would draw for global steps t0 .. t0 + steps at the engine's "train_seed" and "train_batch" (`batch` names
// that value: it sizes the result): the tuple of every row and, under AZ_TRAIN_MIRROR, whether it is mirrored.
struct TrainDraw { std::vector<int64_t> idx; std::vector<uint8_t> mirror; };
inline TrainDraw train_draw(const Engine& e, int64_t n, const uint32_t* weights, int32_t flags, uint64_t t0, int64_t steps, int64_t batch) {
    if (!az_net_train_draw) throw Panic("train_draw: the linked engine library has no az_net_train_draw");
    TrainDraw d;
    d.idx.assign((size_t)std::max<int64_t>(steps * batch, 0), -1);
    d.mirror.assign(d.idx.size(), 0);
    e.check(az_net_train_draw(e.raw(), n, weights, flags, t0, steps, d.idx.data(), d.mirror.data()));
    return d;
}

// ---- held-out loss, the hold-out rule, per-epoch validation (include/az_engine.h; csrc/az_score.h) --------------------------------------
inline az_samples tuples_view(int64_t n, const uint64_t* states, const float* boards, const float* pis, const float* zs) {
    az_samples s{};
    s.capacity = n; s.count = n;
    s.states = const_cast<uint64_t*>(states); s.boards = const_cast<float*>(boards);
    s.pis = const_cast<float*>(pis); s.zs = const_cast<float*>(zs);
    return s;
}
// az_net_evaluate: the loss of a model as self-play runs it over n tuples (states [n,2], or with states nullptr boards [n,2,6,7]; weights
// u32 [n] or nullptr = all ones), scored on the device in one call.  sums = S_ce, S_kl, S_se, S_hit, W; ce / se / kl [n] may be nullptr
struct Score { int64_t n = 0; uint64_t weight_sum = 0; double loss_pi = 0, loss_v = 0, kl = 0, top1 = 0; uint64_t sums[AZ_SCORE_SUMS] = {0, 0, 0, 0, 0}; };
inline Score evaluate(const Engine& e, size_t model_id, int64_t n, const uint64_t* states, const float* boards, const float* pis, const float* zs,
                      const uint32_t* weights = nullptr, float* ce = nullptr, float* se = nullptr, float* kl = nullptr) {
    if (!az_net_evaluate) throw Panic("evaluate: the linked engine library has no az_net_evaluate");
    const az_samples s = tuples_view(n, states, boards, pis, zs);
    double f[AZ_SCORE_FIELDS] = {0, 0, 0, 0, 0, 0};
    Score r;
    e.check(az_net_evaluate(e.raw(), (int32_t)model_id, &s, weights, f, r.sums, ce, se, kl));
    r.n = (int64_t)f[0]; r.weight_sum = (uint64_t)f[1]; r.loss_pi = f[2]; r.loss_v = f[3]; r.kl = f[4]; r.top1 = f[5];
    return r;
}
// az_samples_holdout: held [n] at `share` (0 .. 1) and seed -- a function of the position alone, the same for a position and its mirror image
inline std::vector<uint8_t> samples_holdout(const Engine& e, int64_t n, const uint64_t* states, const float* boards, const float* pis, const float* zs,
                                            double share, uint64_t seed) {
    if (!az_samples_holdout) throw Panic("samples_holdout: the linked engine library has no az_samples_holdout");
    const az_samples s = tuples_view(n, states, boards, pis, zs);
    std::vector<uint8_t> held((size_t)std::max<int64_t>(n, 0), 255);
    e.check(az_samples_holdout(e.raw(), &s, (int64_t)std::llround(share * 1e6), seed, held.data()));
    return held;
}
// az_net_train_set_validation: registers the set az_net_train / az_net_train_samples score at the end of every epoch; n = 0 clears it
inline void train_set_validation(const Engine& e, int64_t n = 0, const uint64_t* states = nullptr, const float* boards = nullptr, const float* pis = nullptr,
                                 const float* zs = nullptr, const uint32_t* weights = nullptr) {
    if (!az_net_train_set_validation) throw Panic("train_set_validation: the linked engine library has no az_net_train_set_validation");
    if (n == 0) { e.check(az_net_train_set_validation(e.raw(), nullptr, nullptr)); return; }
    const az_samples s = tuples_view(n, states, boards, pis, zs);
    e.check(az_net_train_set_validation(e.raw(), &s, weights));
}
// az_net_train_validation: rows [epochs][4] = (loss_pi, loss_v, kl, top1) of the last az_net_train / az_net_train_samples; best_epoch or -1
struct Validation { std::vector<double> rows; int32_t best_epoch = -1; };
inline Validation train_validation(const Engine& e) {
    if (!az_net_train_validation) throw Panic("train_validation: the linked engine library has no az_net_train_validation");
    Validation v;
    v.rows.resize(4 * (size_t)az_net_train_validation(e.raw(), nullptr, 0, nullptr));
    az_net_train_validation(e.raw(), v.rows.data(), (int32_t)(v.rows.size() / 4), &v.best_epoch);
    return v;
}

// ---- search statistics as targets (include/az_engine.h; csrc/az_target.h) --------------------------------------------------------------
// az_selfplay_get_search: the root value and the root's stored priors of the `count` tuples of the last az_selfplay / az_selfplay_next,
// in their order ("selfplay_record_search" must have been 1 for that call)
struct SearchRecord { std::vector<float> root_q, root_prior; };      // [count], [count][7]
inline SearchRecord selfplay_search(const Engine& e, size_t count) {
    if (!az_selfplay_get_search) throw Panic("selfplay_search: the linked engine library has no az_selfplay_get_search");
    SearchRecord r{std::vector<float>(count), std::vector<float>(count * 7)};
    e.check(az_selfplay_get_search(e.raw(), r.root_q.data(), r.root_prior.data()));
    return r;
}
// az_samples_blend_z: (1 - lam) * zs + lam * root_q in f32; lam travels as lambda_e6
inline std::vector<float> blend_z(const Engine& e, const std::vector<float>& zs, const std::vector<float>& root_q, double lam) {
    if (!az_samples_blend_z) throw Panic("blend_z: the linked engine library has no az_samples_blend_z");
    if (zs.size() != root_q.size()) throw Panic("blend_z: zs and root_q differ in length");
    std::vector<float> out(zs.size());
    e.check(az_samples_blend_z(e.raw(), (int64_t)zs.size(), zs.data(), root_q.data(), (int64_t)std::llround(lam * 1e6), out.data()));
    return out;
}
// az_samples_surprise on n tuples given by states [n][2]: tuple i repeated counts[i] times, a share `share` of the weight in proportion to
// KL(pi_i || prior_i).  The expanded set comes back in states / pis / zs
struct Surprised { std::vector<uint64_t> states; std::vector<float> pis, zs, kl; std::vector<uint32_t> counts; };
inline Surprised surprise(const Engine& e, const std::vector<uint64_t>& states, const std::vector<float>& pis, const std::vector<float>& zs,
                          const std::vector<float>& priors, double share, uint64_t seed) {
    if (!az_samples_surprise) throw Panic("surprise: the linked engine library has no az_samples_surprise");
    const size_t n = zs.size();
    if (states.size() != n * 2 || pis.size() != n * 7 || priors.size() != n * 7) throw Panic("surprise: the arrays differ in length");
    Surprised r{std::vector<uint64_t>(4 * n), std::vector<float>(14 * n), std::vector<float>(2 * n), std::vector<float>(n), std::vector<uint32_t>(n)};
    az_samples src{}, dst{};
    src.capacity = src.count = (int64_t)n;
    src.states = const_cast<uint64_t*>(states.data()); src.pis = const_cast<float*>(pis.data()); src.zs = const_cast<float*>(zs.data());
    dst.capacity = (int64_t)(2 * n); dst.states = r.states.data(); dst.pis = r.pis.data(); dst.zs = r.zs.data();
    e.check(az_samples_surprise(e.raw(), &src, priors.data(), (int64_t)std::llround(share * 1e6), seed, &dst, r.counts.data(), r.kl.data()));
    const size_t m = (size_t)dst.count;
    r.states.resize(2 * m); r.pis.resize(7 * m); r.zs.resize(m);
    return r;
}

// ---- az_reanalyse (include/az_reanalyse.h): a fresh search of each of n stored positions with a model as it is now ------------------------
// positions as states [n][2] or (states == nullptr) boards [n][84]; game_ids [n] or nullptr (p.first_game_id + i).  Row i of every array is
// what a one-tree az_tree_get_action_prob says after az_tree_reset(t, &states[i]); want_search = false leaves counts, q and selected empty
struct Reanalysed { std::vector<float> pi, root_q, root_prior, q; std::vector<uint16_t> counts; std::vector<int32_t> selected; };
inline Reanalysed reanalyse(const Engine& e, const az_reanalyse_params& p, int64_t n, const uint64_t* states, const float* boards,
                            const uint64_t* game_ids = nullptr, bool want_search = true) {
    if (!az_reanalyse) throw Panic("reanalyse: the linked engine library has no az_reanalyse");
    if (n < 0) throw Panic("reanalyse: n < 0");
    const size_t N = (size_t)n;
    Reanalysed r;
    r.pi.resize(N * 7); r.root_q.resize(N); r.root_prior.resize(N * 7);
    if (want_search) { r.q.resize(N * 7); r.counts.resize(N * 7); r.selected.resize(N); }
    e.check(az_reanalyse(e.raw(), &p, n, states, boards, game_ids, r.pi.data(), r.root_q.data(), r.root_prior.data(),
                         want_search ? r.counts.data() : nullptr, want_search ? r.q.data() : nullptr, want_search ? r.selected.data() : nullptr));
    return r;
}
// ---- the decided-move stop (include/az_search_stop.h) ---------------------------------------------------------------
// on: a temperature-0 search ends once its move can no longer change; refused while a self-play session is open
inline void set_search_stop(const Engine& e, bool on) {
    if (!az_search_stop_set) throw Panic("set_search_stop: the linked engine library has no az_search_stop_set");
    e.check(az_search_stop_set(e.raw(), on ? 1 : 0));
}
// the four counters over the finished calls; reset clears them afterwards
struct SearchStopStats { uint64_t eligible_moves = 0, stopped_moves = 0, budgeted_sims = 0, skipped_sims = 0; };
inline SearchStopStats search_stop_stats(const Engine& e, bool reset = false) {
    if (!az_search_stop_stats) throw Panic("search_stop_stats: the linked engine library has no az_search_stop_stats");
    uint64_t v[4] = {0, 0, 0, 0};
    e.check(az_search_stop_stats(e.raw(), v, reset ? 1 : 0));
    return SearchStopStats{v[0], v[1], v[2], v[3]};
}
// The Coaches' rule (csrc/az_reanalyse.h states it; alphazero-rs_amd/coach.py is the other host): in iteration `it`, once the new window is
// appended and the oldest dropped, every history entry h but the last is re-searched, tuple j of it on game id
// reanalyse_first_game_id(it, h) + j with seed + it as the call's seed
constexpr uint64_t REANALYSE_ID_BASE = 1ull << 62;
inline uint64_t reanalyse_first_game_id(uint64_t iteration, uint64_t history_index) { return REANALYSE_ID_BASE + (iteration << 40) + (history_index << 32); }
inline size_t reanalyse_entries(size_t history_len) { return history_len > 1 ? history_len - 1 : 0; }

inline Ratings rating_fit(const std::vector<uint64_t>& wld, size_t K, double prior_games = 2.0) {
    if (!az_rating_fit) throw Panic("rating_fit: the linked engine library has no az_rating_fit");
    if (wld.size() != K * K * 3) throw Panic("rating_fit: wld must hold K * K * 3 counts");
    Ratings r{std::vector<double>(K, 0.0), std::vector<double>(K, 0.0), 0};
    if (az_rating_fit(wld.data(), (int32_t)K, prior_games, r.elo.data(), r.elo_se.data(), &r.sweeps) != AZ_OK)
        throw Panic("rating_fit: K outside 2 .. 16, or a negative or non-finite prior_games");
    return r;
}

// The move-quality tally of one arena shard: counts[0] the new model's moves, counts[1] the old model's, each {examined, kept, win_to_draw,
// win_to_loss, draw_to_loss, unknown}.  Game g of the shard has global index first_game + g; the new model holds the first seat in the
// games below total_games / 2 (az_arena), and the first seat moves at the even plies of the record -- a start board, opening or not,
// always has the first seat to move (az_arena_get_openings).
inline void quality_tally(const std::vector<uint8_t>& ply_class, size_t first_game, size_t total_games, uint64_t counts[2][6]) {
    const size_t n = ply_class.size() / AZ_MAX_PLIES;
    for (size_t g = 0; g < n; ++g)
        for (size_t p = 0; p < AZ_MAX_PLIES; ++p) {
            const uint8_t c = ply_class[g * AZ_MAX_PLIES + p];
            if (c == AZ_MQ_SKIPPED) continue;
            const bool new_first = first_game + g < total_games / 2, first_moves = p % 2 == 0;
            uint64_t* row = counts[new_first == first_moves ? 0 : 1];
            ++row[0];
            ++row[c];
        }
}

class NNet {                                                            // src/nnet.rs:35-45
  public:
    virtual ~NNet() = default;
    virtual void train(const float* boards, const float* pis, const float* vs, int64_t n, size_t prev_id, size_t id) = 0;
    virtual void predict(const float* boards, int batch, size_t model_id, float* pi, float* v) const = 0;
};
class Mi355xNNet : public NNet {
  public:
    explicit Mi355xNNet(Engine& e) : e_(e) {}
    void train(const float* b, const float* p, const float* v, int64_t n, size_t prev_id, size_t id) override {
        e_.check(az_net_train(e_.raw(), (int)prev_id, (int)id, b, p, v, n));
    }
    void predict(const float* boards, int batch, size_t model_id, float* pi, float* v) const override {
        e_.check(az_net_predict(e_.raw(), (int)model_id, boards, batch, pi, v));
    }

  private:
    Engine& e_;
};

class AsyncMcts;

// ---- SharedMcts: one shared az_tree whose slots many host threads use at once (az_tree_share) -------------------------
// The reference's episode threads (src/coach.rs:202-205, :241-272) share one inference_thread (src/async_mcts.rs:117-189); here
// each thread builds its AsyncMcts on a slot of one G-tree batch (SharedMcts::mcts), keeps execute_episode as written, and the
// engine coalesces the threads' get_action_prob calls into batched searches.  Destroy the SharedMcts after every AsyncMcts on it.
class SharedMcts {
  public:
    SharedMcts(Engine& e, size_t slots, size_t reserve_space, size_t num_sims, size_t num_threads, size_t max_depth, size_t model_id,
               int32_t cpuct, int32_t window_us = 0) : e_(e) {
        if (num_threads == 0 || num_sims % num_threads != 0)
            throw Panic("assertion failed: self.num_sims % self.num_threads == 0");   // src/async_mcts.rs:192
        e_.check(az_tree_create(e.raw(), (int)slots, reserve_space, (int)num_sims, (int)num_threads, (int)max_depth, (int)model_id, cpuct, &t_));
        const int rc = az_tree_share(t_, window_us);
        if (rc != AZ_OK) { az_tree_destroy(t_); t_ = nullptr; e_.check(rc); }
    }
    ~SharedMcts() { if (t_) az_tree_destroy(t_); }
    SharedMcts(const SharedMcts&) = delete;
    SharedMcts& operator=(const SharedMcts&) = delete;
    // AsyncMcts::default(..) on a free slot (the tree starts at the initial board); the slot is released when the AsyncMcts dies
    inline AsyncMcts mcts();
    // {batches, requests, largest batch, batches started by the window}
    std::array<uint64_t, 4> stats() const {
        std::array<uint64_t, 4> s{};
        if (az_tree_share_stats(t_, s.data()) != AZ_OK) throw Panic("az_tree_share_stats failed");
        return s;
    }
    az_tree* raw() const { return t_; }

  private:
    Engine& e_;
    az_tree* t_ = nullptr;
};

// ---- AsyncMcts: one tree behind az_tree_* (its own 1-game az_tree, or one slot of a SharedMcts) -------------------------------
class AsyncMcts {
  public:
    // AsyncMcts::default(reserve_space, num_sims, num_threads, max_depth, model_id, cpuct, ..), src/async_mcts.rs:27-48
    // num_threads > 1: several simulations in flight per tree, the engine's deterministic lock-step schedule (az_engine.h)
    static AsyncMcts default_(Engine& e, size_t reserve_space, size_t num_sims, size_t num_threads, size_t max_depth,
                              size_t model_id, int32_t cpuct) {
        if (num_threads == 0 || num_sims % num_threads != 0)
            throw Panic("assertion failed: self.num_sims % self.num_threads == 0");   // src/async_mcts.rs:192
        return AsyncMcts(e, reserve_space, num_sims, num_threads, max_depth, model_id, cpuct);
    }
    AsyncMcts(AsyncMcts&& o) noexcept : e_(o.e_), t_(o.t_), slot_(o.slot_) { o.t_ = nullptr; }
    ~AsyncMcts() {
        if (!t_) return;
        if (slot_ >= 0) az_tree_slot_release(t_, slot_);
        else az_tree_destroy(t_);
    }
    // get_action_prob(&self, s, temp, episode_id, rng): `s` canonical; rng = (seed, episode_id) stream (B7)
    Policy get_action_prob(const ConnectFourGame& s, float temp, size_t episode_id, uint64_t seed,
                           std::array<uint16_t, 7>* counts = nullptr, std::array<float, 7>* q = nullptr) const {
        const uint64_t st[2] = {s.plus, s.minus};
        Policy pi(7);
        if (slot_ >= 0) {           // a slot of a SharedMcts: errors are the slot's own (az_last_error belongs to the whole engine)
            const int rc = az_tree_slot_get_action_prob(t_, slot_, st, temp, seed, (uint64_t)episode_id, pi.data(),
                                                        counts ? counts->data() : nullptr, q ? q->data() : nullptr);
            if (rc != AZ_OK) throw Panic(std::string(az_tree_slot_error(t_, slot_)));
            return pi;
        }
        e_.check(az_tree_get_action_prob(t_, st, temp, seed, (uint64_t)episode_id, pi.data(),
                                         counts ? counts->data() : nullptr, q ? q->data() : nullptr));
        return pi;
    }
    int slot() const { return slot_; }

  private:
    friend class SharedMcts;
    AsyncMcts(Engine& e, az_tree* shared, int slot) : e_(e), t_(shared), slot_(slot) {}
    AsyncMcts(Engine& e, size_t reserve, size_t sims, size_t threads, size_t max_depth, size_t model_id, int32_t cpuct) : e_(e) {
        e_.check(az_tree_create(e.raw(), 1, reserve, (int)sims, (int)threads, (int)max_depth, (int)model_id, cpuct, &t_));
    }
    Engine& e_;
    az_tree* t_ = nullptr;
    int slot_ = -1;           // >= 0: slot of a shared tree batch (t_ is the SharedMcts's, not ours)
};

inline AsyncMcts SharedMcts::mcts() {
    int32_t slot = -1;
    const int rc = az_tree_slot_acquire(t_, &slot);
    if (rc == AZ_ERR_CAPACITY) throw Panic("SharedMcts: every slot is held");
    if (rc != AZ_OK) throw Panic("az_tree_slot_acquire failed");
    return AsyncMcts(e_, t_, slot);
}

// ---- arena (src/arena.rs:7-99) ------------------------------------------------------------------------------------
using PlayerAction = std::function<uint8_t(const ConnectFourGame&)>;

inline int8_t play_game(const std::array<const PlayerAction*, 2>& player_actions, const ConnectFourGame* board0) {
    int8_t cur_player = 1;
    ConnectFourGame board = board0 ? *board0 : ConnectFourGame::get_init_board();
    while (board.get_game_ended(cur_player) == 0.f) {                          // :18
        const ConnectFourGame canonical = board.get_canonical_form(cur_player); // :25
        const uint8_t action = (*player_actions[cur_player == 1 ? 0 : 1])(canonical);
        if (canonical.get_valid_moves(1)[action] == 0) throw Panic("Action is not valid!");   // :31-35
        auto nx = board.get_next_state(cur_player, action);
        board = nx.first;
        cur_player = nx.second;
    }
    return (int8_t)(cur_player * (int8_t)std::lround(board.get_game_ended(cur_player)));      // :51
}

struct GameResultCounter { size_t win = 0, loss = 0, draw = 0; };             // Counter<GameResult>, :54-59

inline GameResultCounter play_games(size_t num, const std::array<const PlayerAction*, 2>& player_actions,
                                    const ConnectFourGame* board) {
    GameResultCounter all;
    for (int ordering = 0; ordering < 2; ++ordering) {                         // Heap's permutations of 2: (0,1), (1,0)
        const std::array<const PlayerAction*, 2> seated = {player_actions[ordering], player_actions[1 - ordering]};
        const int win_cond = ordering == 0 ? 1 : -1, lose_cond = -win_cond;    // :80-81
        for (size_t i = 0; i < num / 2; ++i) {                                 // :83
            const int8_t r = play_game(seated, board);
            if (r == win_cond) ++all.win; else if (r == lose_cond) ++all.loss; else ++all.draw;
        }
    }
    return all;
}

// ---- Coach::execute_episode (src/coach.rs:104-157) with the engine's RNG stream --------------------------------------
inline uint64_t mix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    uint64_t z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
inline uint8_t choose_weighted(uint64_t seed, uint64_t episode_id, uint64_t ply, const Policy& pi) {
    const uint64_t r = mix64(mix64(mix64(mix64(seed) ^ episode_id) ^ ply) ^ 2ull);
    float total = 0.f;
    for (float p : pi) total = total + p;
    const float target = (float)(uint32_t)(r >> 40) * (1.0f / 16777216.0f) * total;
    float acc = 0.f;
    int last = 0;
    for (int a = 0; a < (int)pi.size(); ++a)
        if (pi[a] > 0.f) { acc = acc + pi[a]; last = a; if (target < acc) return (uint8_t)a; }
    return (uint8_t)last;
}

inline std::vector<TrainingSample> execute_episode(const AsyncMcts& mcts, size_t temp_threshold, size_t episode_id,
                                                   uint64_t seed, std::vector<uint8_t>* moves = nullptr) {
    struct Ex { BoardFeatures f; int8_t player; Policy pi; };
    std::vector<Ex> train_examples;
    ConnectFourGame board = ConnectFourGame::get_init_board();
    int8_t cur_player = 1;
    size_t episode_step = 0;
    for (;;) {
        ++episode_step;
        const ConnectFourGame canonical = board.get_canonical_form(cur_player);
        const float temp = episode_step < temp_threshold ? 1.f : 0.f;             // :122-126
        const Policy pi = mcts.get_action_prob(canonical, temp, episode_id, seed);   // :128
        for (auto& bp : canonical.get_symmetries(pi)) train_examples.push_back({bp.first.to_features(), cur_player, bp.second});
        const uint8_t action = choose_weighted(seed, episode_id, episode_step - 1, pi);   // :137-138
        if (moves) moves->push_back(action);
        auto nx = board.get_next_state(cur_player, action);
        board = nx.first;
        cur_player = nx.second;
        const float r = board.get_game_ended(cur_player);                            // :144
        if (r != 0.f) {
            std::vector<TrainingSample> out;
            for (auto& ex : train_examples) out.push_back({ex.f, ex.pi, r * (ex.player == cur_player ? 1.f : -1.f)});   // B4
            return out;
        }
    }
}

// ---- Coach (src/coach.rs:17-396) ----------------------------------------------------------------------------------
// The iteration loop around the engine: self-play episodes -> replay window -> <iter>.examples -> [merge duplicate positions, opt-in] -> shuffle ->
// NNet::train(samples, model_id, model_id + 1) -> arena of new vs old -> accept iff nwins + pwins > 0 and
// nwins / (nwins + pwins) >= update_threshold.  Self-play, training and the arena are ONE engine call each.
// The Python host (alphazero-rs_amd/coach.py) runs the same sequence with the same seeds and writes the same files.
//
// <dir>/<iter>.examples ("AZEX0001", the build's own format; the reference's is bincode, src/coach.rs:159-167, A14):
//   char magic[8]; int64 H; int64 lens[H]; f32 boards[N][2][6][7]; f32 pis[N][7]; f32 vs[N]   (N = sum lens; the whole
//   `history` deque, oldest entry first).   <dir>/<model_id>.aznet = az_net_save.
struct HistoryEntry { std::vector<float> boards, pis, vs; size_t len() const { return vs.size(); } };

// Fisher-Yates with the build's counter RNG (the reference shuffles with SmallRng, src/coach.rs:296-297; B7):
// for i = n-1 .. 1: j = ((draw(seed, iteration, i, 5) >> 32) * (i + 1)) >> 32; swap(perm[i], perm[j])
inline std::vector<int64_t> shuffle_permutation(size_t n, uint64_t seed, uint64_t iteration) {
    std::vector<int64_t> perm(n);
    for (size_t i = 0; i < n; ++i) perm[i] = (int64_t)i;
    for (size_t i = n; i-- > 1;) {
        const uint64_t r = mix64(mix64(mix64(mix64(seed) ^ iteration) ^ (uint64_t)i) ^ 5ull);
        const size_t j = (size_t)(((r >> 32) * (uint64_t)(i + 1)) >> 32);
        std::swap(perm[i], perm[j]);
    }
    return perm;
}

// An engine option that holds for one scope only: apply() now when `active`, clear() when the scope is left (also by a throw).
// active == false: the engine is never asked.  Several in one scope are cleared in the reverse of the order they were applied in.
template <class Apply, class Clear>
struct ScopedOption {
    bool active; Clear clear;
    ScopedOption(bool active_, Apply apply, Clear clear_) : active(active_), clear(std::move(clear_)) { if (active) apply(); }
    ~ScopedOption() { if (active) { try { clear(); } catch (...) {} } }
    ScopedOption(const ScopedOption&) = delete;
    ScopedOption& operator=(const ScopedOption&) = delete;
};

class Coach {
  public:
    // samples = the tuples trained on, samples_raw = the tuples of the window before position averaging (equal with merge_positions off)
    // samples_weight (with merge_weighted): the sum of the multiplicities the batches were drawn by (= samples_raw); 0 with it off
    // quality (with solve_min_stones > 0): [0] the new model's arena moves, [1] the old model's, each {examined, kept, win_to_draw, win_to_loss,
    // draw_to_loss, unknown} (quality_tally above); all zero with the report off
    // val_n, val_loss_pi / val_loss_v / val_top1 (one entry per epoch) and best_epoch (with validation_share > 0): the held-out part of the
    // window and its score at the end of every epoch; 0, empty and -1 with it off
    struct Report { size_t iteration, samples, nwins, pwins, draws, model_id; bool accepted; std::vector<float> losses; size_t samples_raw; uint64_t quality[2][6]; size_t samples_weight;
                    size_t val_n; std::vector<double> val_loss_pi, val_loss_v, val_top1; int32_t best_epoch;
                    // reanalysed (with reanalyse_sims > 0): the tuples of the older history entries whose pi this iteration re-searched, and the
                    // seconds that took; 0 with it off
                    size_t reanalysed; double t_reanalyse; };

    // Coach::setup(checkpoint_directory, + the reference's 14 numeric parameters), src/coach.rs:38-103
    static Coach setup(Engine& e, const std::string& checkpoint_directory, size_t mcts_reserve_size, float update_threshold,
                       size_t temp_threshold, size_t max_history_length, size_t max_queue_length, size_t inference_batch_size,
                       size_t num_episode_threads, size_t num_arena_games, size_t num_iters, size_t num_eps, size_t num_sims,
                       size_t num_sim_threads, size_t max_depth, int32_t cpuct) {
        if (inference_batch_size == 0 || num_sims % inference_batch_size != 0)
            throw Panic("assertion failed: num_sims % inference_batch_size == 0");        // src/coach.rs:83
        if (num_sim_threads == 0 || num_sims % num_sim_threads != 0)
            throw Panic("assertion failed: self.num_sims % self.num_threads == 0");             // src/async_mcts.rs:192
        Coach c(e);
        c.num_sim_threads = num_sim_threads;
        c.dir_ = checkpoint_directory;
        c.mcts_reserve_size = mcts_reserve_size; c.update_threshold = update_threshold; c.temp_threshold = temp_threshold;
        c.max_history_length = max_history_length; c.max_queue_length = max_queue_length;
        c.num_episode_threads = num_episode_threads; c.num_arena_games = num_arena_games; c.num_iters = num_iters;
        c.num_eps = num_eps; c.num_sims = num_sims; c.max_depth = max_depth; c.cpuct = cpuct;
        namespace fs = std::filesystem;
        fs::create_directories(c.dir_);
        long best = -1;                                        // resume from the largest numeric stem (:55-81)
        for (auto& ent : fs::directory_iterator(c.dir_)) {
            const std::string stem = ent.path().stem().string();
            if (ent.path().extension() != ".examples" || stem.empty() || stem.find_first_not_of("0123456789") != std::string::npos) continue;
            best = std::max(best, std::stol(stem));
        }
        if (best >= 0) {
            c.load_train_examples((size_t)best);
            c.start_iteration = (size_t)best + 1;
            // <dir>/coach.state = "iteration model_id": the accepted model after that iteration's gate; load it so the
            // restarted run continues from the live weights
            long it = -1, mid = -1;
            if (FILE* f = std::fopen((c.dir_ + "/coach.state").c_str(), "r")) {
                if (std::fscanf(f, "%ld %ld", &it, &mid) != 2) it = -1;
                std::fclose(f);
            }
            if (it == best && mid >= 0) {
                c.model_id = (size_t)mid;
                const std::string w = c.dir_ + "/" + std::to_string(mid) + ".aznet";
                if (fs::exists(w)) e.check(az_net_load(e.raw(), (int32_t)mid, w.c_str()));
            }
        }
        return c;
    }

    std::string examples_path(size_t iteration) const { return dir_ + "/" + std::to_string(iteration) + ".examples"; }

    void save_train_examples(size_t iteration) const {          // src/coach.rs:159-167
        FILE* f = std::fopen(examples_path(iteration).c_str(), "wb");
        if (!f) throw Panic("cannot write " + examples_path(iteration));
        const int64_t H = (int64_t)history.size();
        std::fwrite("AZEX0001", 1, 8, f);
        std::fwrite(&H, sizeof H, 1, f);
        for (auto& h : history) { const int64_t n = (int64_t)h.len(); std::fwrite(&n, sizeof n, 1, f); }
        for (auto& h : history) std::fwrite(h.boards.data(), sizeof(float), h.boards.size(), f);
        for (auto& h : history) std::fwrite(h.pis.data(), sizeof(float), h.pis.size(), f);
        for (auto& h : history) std::fwrite(h.vs.data(), sizeof(float), h.vs.size(), f);
        std::fclose(f);
    }

    void load_train_examples(size_t iteration) {
        FILE* f = std::fopen(examples_path(iteration).c_str(), "rb");
        if (!f) throw Panic("cannot read " + examples_path(iteration));
        char magic[8];
        int64_t H = 0;
        bool ok = std::fread(magic, 1, 8, f) == 8 && std::memcmp(magic, "AZEX0001", 8) == 0 && std::fread(&H, sizeof H, 1, f) == 1 && H >= 0;
        std::vector<int64_t> lens((size_t)(ok ? H : 0));
        ok = ok && std::fread(lens.data(), sizeof(int64_t), lens.size(), f) == lens.size();
        history.clear();
        for (int64_t n : lens) { HistoryEntry h; h.boards.resize((size_t)n * 84); h.pis.resize((size_t)n * 7); h.vs.resize((size_t)n); history.push_back(std::move(h)); }
        for (auto& h : history) ok = ok && std::fread(h.boards.data(), sizeof(float), h.boards.size(), f) == h.boards.size();
        for (auto& h : history) ok = ok && std::fread(h.pis.data(), sizeof(float), h.pis.size(), f) == h.pis.size();
        for (auto& h : history) ok = ok && std::fread(h.vs.data(), sizeof(float), h.vs.size(), f) == h.vs.size();
        std::fclose(f);
        if (!ok) throw Panic("malformed " + examples_path(iteration));
    }

    // One process per GPU: rank r of `world` plays the episode ids shard_range(num_eps, r, world) of every
    // iteration and the arena games shard_range(num_arena_games, r, world); the tuples meet in ONE az_gather_samples (every
    // rank receives: the trainer is replicated) and the arena tally in one 3-counter all-reduce.  world > 1 needs a
    // communicator on the engine (az_comm_unique_id on one rank, the 128 bytes shipped by the host, az_comm_init on all; or, for the
    // engines of ONE process driven by one thread each, az_comm_local_id: examples/connect_four_threads.cpp).
    void shard(int rank, int world) {
        if (world < 1 || rank < 0 || rank >= world) throw Panic("shard: rank outside the world");
        rank_ = rank; world_ = world;
    }
    static std::pair<size_t, size_t> shard_range(size_t n, int rank, int world) {
        return {n * (size_t)rank / (size_t)world, n * (size_t)(rank + 1) / (size_t)world};
    }

    // the self-play fan-out of src/coach.rs:241-272: num_eps x execute_episode, emitted with both symmetries
    HistoryEntry execute_episodes(size_t model_id, size_t iteration, uint64_t seed) {
        if (!(value_target_q >= 0.0 && value_target_q <= 1.0 && surprise_share >= 0.0 && surprise_share <= 1.0))
            throw Panic("value_target_q and surprise_share must be in 0 .. 1");
        if (surprise_share > 0 && world_ > 1) throw Panic("surprise_share needs a world of 1: the weights would be normalised per shard");
        // the target options work on the compact (state, pi, z) tuples before the symmetries are expanded: the sharded path's shape
        if (world_ > 1 || use_comm_at_world_1 || value_target_q > 0 || surprise_share > 0) return execute_episodes_sharded(model_id, iteration, seed);
        az_selfplay_params p{};
        p.n_games = (int32_t)num_eps; p.concurrent = (int32_t)std::min(num_episode_threads, num_eps);
        p.num_sims = (int32_t)num_sims; p.temp_threshold = (int32_t)temp_threshold; p.max_depth = (int32_t)max_depth;
        p.cpuct = cpuct; p.model_id = (int32_t)model_id; p.symmetries = 1; p.reserve = mcts_reserve_size; p.seed = seed;
        p.first_game_id = (uint64_t)(iteration * num_eps);
        p.num_sim_threads = (int32_t)num_sim_threads;
        const size_t cap = num_eps * 42 * 2;
        HistoryEntry h;
        h.boards.resize(cap * 84); h.pis.resize(cap * 7); h.vs.resize(cap);
        az_samples out{};
        out.capacity = (int64_t)cap; out.boards = h.boards.data(); out.pis = h.pis.data(); out.zs = h.vs.data();
        e_.check(az_selfplay(e_.raw(), &p, &out));
        const size_t n = (size_t)out.count;
        h.boards.resize(n * 84); h.pis.resize(n * 7); h.vs.resize(n);
        return h;
    }

    // the same fan-out over the ranks: this rank's shard of the episode ids as compact (state, pi, z) tuples, ONE gather in which
    // every rank receives all of them (rank order = episode-id order), symmetries regenerated here
    HistoryEntry execute_episodes_sharded(size_t model_id, size_t iteration, uint64_t seed) {
        const auto [lo, hi] = shard_range(num_eps, rank_, world_);
        const size_t mine = hi - lo;
        std::vector<uint64_t> st(std::max<size_t>(mine, 1) * 42 * 2);
        std::vector<float> pi(std::max<size_t>(mine, 1) * 42 * 7), z(std::max<size_t>(mine, 1) * 42);
        az_samples loc{};
        loc.capacity = (int64_t)(mine * 42); loc.states = st.data(); loc.pis = pi.data(); loc.zs = z.data();
        if (mine > 0) {
            az_selfplay_params p{};
            p.n_games = (int32_t)mine; p.concurrent = (int32_t)std::min(num_episode_threads, mine);
            p.num_sims = (int32_t)num_sims; p.temp_threshold = (int32_t)temp_threshold; p.max_depth = (int32_t)max_depth;
            p.cpuct = cpuct; p.model_id = (int32_t)model_id; p.symmetries = 0; p.reserve = mcts_reserve_size; p.seed = seed;
            p.first_game_id = (uint64_t)(iteration * num_eps + lo);
            p.num_sim_threads = (int32_t)num_sim_threads;
            const bool targets = value_target_q > 0 || surprise_share > 0;
            {
                // the search record around the episodes only, as the other self-play options are
                ScopedOption record_guard(targets, [&] { e_.set_record_search(true); }, [&] { e_.set_record_search(false); });
                e_.check(az_selfplay(e_.raw(), &p, &loc));
            }
            if (targets) {                                            // this rank's own tuples, before any gather
                const size_t k = (size_t)loc.count;
                st.resize(k * 2); pi.resize(k * 7); z.resize(k);
                const SearchRecord rec = selfplay_search(e_, k);
                if (value_target_q > 0) z = blend_z(e_, z, rec.root_q, value_target_q);          // a blended z is still a z
                if (surprise_share > 0) {                             // a resampled set is still a set of tuples
                    Surprised sp = surprise(e_, st, pi, z, rec.root_prior, surprise_share, seed + (uint64_t)iteration);
                    st.swap(sp.states); pi.swap(sp.pis); z.swap(sp.zs);
                }
                loc.count = (int64_t)z.size(); loc.capacity = loc.count;
                if (z.empty()) { st.resize(2); pi.resize(7); z.resize(1); }
                loc.states = st.data(); loc.pis = pi.data(); loc.zs = z.data();
            }
        }
        const size_t cap = std::max(num_eps * 42, (size_t)loc.count);      // (surprise_share holds at world 1 only: its at most 2x growth is all here)
        std::vector<uint64_t> gs(cap * 2);
        std::vector<float> gp(cap * 7), gz(cap);
        az_samples all{};
        all.capacity = (int64_t)cap; all.states = gs.data(); all.pis = gp.data(); all.zs = gz.data();
        if (world_ > 1 || use_comm_at_world_1) e_.check(az_gather_samples(e_.raw(), &loc, -1, &all, nullptr));
        else {                                                        // one rank and no communicator: its own tuples are all there are
            const size_t k = (size_t)loc.count;
            std::copy(st.begin(), st.begin() + (std::ptrdiff_t)(k * 2), gs.begin());
            std::copy(pi.begin(), pi.begin() + (std::ptrdiff_t)(k * 7), gp.begin());
            std::copy(z.begin(), z.begin() + (std::ptrdiff_t)k, gz.begin());
            all.count = (int64_t)k;
        }
        const size_t n = (size_t)all.count;
        HistoryEntry h;
        h.boards.assign(n * 2 * 84, 0.f); h.pis.resize(n * 2 * 7); h.vs.resize(n * 2);
        for (size_t i = 0; i < n; ++i) {                         // get_symmetries (connect_four_game.rs:205-211): identity, then the mirror
            ConnectFourGame g;
            g.plus = gs[2 * i]; g.minus = gs[2 * i + 1];
            const Policy p(gp.begin() + (std::ptrdiff_t)(i * 7), gp.begin() + (std::ptrdiff_t)(i * 7 + 7));
            size_t k = 2 * i;
            for (auto& bp : g.get_symmetries(p)) {
                const BoardFeatures f = bp.first.to_features();
                std::copy(f.begin(), f.end(), h.boards.begin() + (std::ptrdiff_t)(k * 84));
                std::copy(bp.second.begin(), bp.second.end(), h.pis.begin() + (std::ptrdiff_t)(k * 7));
                h.vs[k] = gz[i];
                ++k;
            }
        }
        return h;
    }

    // Coach::reanalyse_sims: the pi of every tuple of every history entry but the newest becomes az_reanalyse's under the current model
    // (in its self-play class), with the Coach's forced playouts / Gumbel rule on, root noise off and the playout cap untouched; z is kept,
    // or with value_target_q > 0 blended with the fresh root value.  Returns the tuples re-searched.  Every rank holds the whole history and
    // runs the same deterministic calls: no exchange
    size_t reanalyse_history(size_t model_id, size_t iteration, uint64_t seed) {
        if (selfplay_class != AZ_NET_CLASS_ENGINE) e_.net_set_class(model_id, selfplay_class);
        ScopedOption forced_guard(forced_playouts_k > 0, [&] { e_.set_forced_playouts(forced_playouts_k, policy_prune); },
                                  [&] { e_.set_forced_playouts(0.0, false); });
        ScopedOption gumbel_guard(gumbel_m > 0, [&] { e_.set_gumbel(gumbel_m, gumbel_c_visit, gumbel_c_scale); }, [&] { e_.set_gumbel(0); });
        size_t done = 0;
        for (size_t hi = 0; hi < reanalyse_entries(history.size()); ++hi) {
            HistoryEntry& h = history[hi];
            if (h.len() == 0) continue;
            az_reanalyse_params p{};
            p.concurrent = (int32_t)num_episode_threads; p.num_sims = (int32_t)reanalyse_sims; p.max_depth = (int32_t)max_depth; p.cpuct = cpuct;
            p.model_id = (int32_t)model_id; p.num_sim_threads = (int32_t)num_sim_threads; p.temp = 1.0f; p.reserve = mcts_reserve_size;
            p.seed = seed + (uint64_t)iteration; p.first_game_id = reanalyse_first_game_id(iteration, hi);
            Reanalysed r = reanalyse(e_, p, (int64_t)h.len(), nullptr, h.boards.data(), nullptr, false);
            h.pis.swap(r.pi);
            if (value_target_q > 0) h.vs = blend_z(e_, h.vs, r.root_q, value_target_q);
            done += h.len();
        }
        return done;
    }

    // Coach::learn(skip_first_play), src/coach.rs:169-396.  Engine model slots: `model_id` is the current net,
    // `model_id + 1` the candidate.
    static constexpr size_t RESUMED = (size_t)-1;     // learn(): continue from the live model of the resumed run (else 0)
    std::vector<Report> learn(bool skip_first_play, uint64_t seed, size_t model_id = RESUMED) {
        std::vector<Report> report;
        if (model_id == RESUMED) model_id = this->model_id;
        {   // the run's initial model: what a restart would load
            const std::string w = dir_ + "/" + std::to_string(model_id) + ".aznet";
            if (rank_ == 0 && !std::filesystem::exists(w)) e_.check(az_net_save(e_.raw(), (int32_t)model_id, w.c_str()));
        }
        if (eval_mirror) e_.set_eval_mirror(true);
        if (search_stop) set_search_stop(e_, true);
        for (size_t iteration = start_iteration; iteration < start_iteration + num_iters; ++iteration) {
            HistoryEntry h;
            if (!skip_first_play || iteration > start_iteration) {
                if (selfplay_class != AZ_NET_CLASS_ENGINE) e_.net_set_class(model_id, selfplay_class);
                {
                    // root noise around the episodes only: on before az_selfplay, off again behind it (also when it throws)
                    ScopedOption noise_guard(root_noise_eps > 0, [&] { e_.set_root_noise(root_noise_eps, root_noise_alpha); },
                                             [&] { e_.set_root_noise(0.0, root_noise_alpha); });
                    // ... and so is the playout cap
                    ScopedOption cap_guard(playout_cap_sims > 0, [&] { e_.set_playout_cap(playout_cap_sims, playout_cap_full); },
                                           [&] { e_.set_playout_cap(0, playout_cap_full); });
                    // ... and so are forced playouts and pruning
                    ScopedOption forced_guard(forced_playouts_k > 0, [&] { e_.set_forced_playouts(forced_playouts_k, policy_prune); },
                                              [&] { e_.set_forced_playouts(0.0, false); });
                    // ... and so is Gumbel root search
                    ScopedOption gumbel_guard(gumbel_m > 0, [&] { e_.set_gumbel(gumbel_m, gumbel_c_visit, gumbel_c_scale); }, [&] { e_.set_gumbel(0); });
                    h = execute_episodes(model_id, iteration, seed);
                }
                if (h.len() > max_queue_length) {                   // keep the newest max_queue_length (:275-277)
                    const size_t drop = h.len() - max_queue_length;
                    h.boards.erase(h.boards.begin(), h.boards.begin() + (std::ptrdiff_t)(drop * 84));
                    h.pis.erase(h.pis.begin(), h.pis.begin() + (std::ptrdiff_t)(drop * 7));
                    h.vs.erase(h.vs.begin(), h.vs.begin() + (std::ptrdiff_t)drop);
                }
            }
            history.push_back(std::move(h));                                    // :282: pushed even when the play was skipped
            if (history.size() > max_history_length) history.pop_front();      // :285-288
            size_t reanalysed = 0;
            double t_reanalyse = 0.0;
            if (reanalyse_sims > 0) {                                 // before the save: a resumed run reads what this one trained on
                const auto t0 = std::chrono::steady_clock::now();
                reanalysed = reanalyse_history(model_id, iteration, seed);
                t_reanalyse = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            }
            if (rank_ == 0) save_train_examples(iteration);                       // :291-293 (one writer per run)
            size_t n = 0;
            for (auto& h : history) n += h.len();
            if (n == 0) throw Panic("assertion failed: training set is empty");   // :305
            std::vector<float> ab, ap, av;
            ab.reserve(n * 84); ap.reserve(n * 7); av.reserve(n);
            for (auto& h : history) { ab.insert(ab.end(), h.boards.begin(), h.boards.end()); ap.insert(ap.end(), h.pis.begin(), h.pis.end()); av.insert(av.end(), h.vs.begin(), h.vs.end()); }
            const size_t n_raw = n;
            size_t val_n = 0;
            if (validation_share > 0) {                               // the split: before merge and shuffle, by the position alone
                if (!(validation_share < 1.0)) throw Panic("validation_share must be in 0 .. 1 (exclusive)");
                const std::vector<uint8_t> held = samples_holdout(e_, (int64_t)n, nullptr, ab.data(), ap.data(), av.data(), validation_share, seed);
                std::vector<float> vb, vp, vv, tb, tp, tv;
                for (size_t i = 0; i < n; ++i) {
                    std::vector<float>&b = held[i] ? vb : tb, &p = held[i] ? vp : tp, &v = held[i] ? vv : tv;
                    b.insert(b.end(), ab.begin() + (std::ptrdiff_t)(i * 84), ab.begin() + (std::ptrdiff_t)((i + 1) * 84));
                    p.insert(p.end(), ap.begin() + (std::ptrdiff_t)(i * 7), ap.begin() + (std::ptrdiff_t)((i + 1) * 7));
                    v.push_back(av[i]);
                }
                val_n = vv.size();
                if (val_n == n) throw Panic("validation_share holds the whole window out");
                if (val_n > 0) {
                    train_set_validation(e_, (int64_t)val_n, nullptr, vb.data(), vp.data(), vv.data());
                    ab.swap(tb); ap.swap(tp); av.swap(tv);
                    n = av.size();
                }
            } else if (keep_best || patience) {
                throw Panic("keep_best and patience need validation_share > 0");
            }
            if (merge_weighted && !merge_positions) throw Panic("merge_weighted requires merge_positions");
            std::vector<uint64_t> as;                                 // merge_weighted: the merged states (no planes are made)
            std::vector<uint32_t> mult;                               // ... and their multiplicities
            if (merge_positions) {                                    // one tuple per distinct position of the window: mean pi, mean z
                if (!az_samples_merge) throw Panic("merge_positions: the linked engine library has no az_samples_merge");
                std::vector<float> mb(merge_weighted ? 0 : n * 84), mp(n * 7), mv(n);
                az_samples src{}, dst{};
                src.count = (int64_t)n; src.boards = ab.data(); src.pis = ap.data(); src.zs = av.data();
                dst.capacity = (int64_t)n; dst.pis = mp.data(); dst.zs = mv.data();
                if (merge_weighted) { as.resize(n * 2); mult.resize(n); dst.states = as.data(); }
                else dst.boards = mb.data();
                e_.check(az_samples_merge(e_.raw(), &src, merge_canonical ? AZ_MERGE_CANONICAL : 0, &dst, merge_weighted ? mult.data() : nullptr));
                n = (size_t)dst.count;
                mb.resize(merge_weighted ? 0 : n * 84); mp.resize(n * 7); mv.resize(n);
                as.resize(merge_weighted ? n * 2 : 0); mult.resize(merge_weighted ? n : 0);
                ab.swap(mb); ap.swap(mp); av.swap(mv);
            }
            const std::vector<int64_t> perm = shuffle_permutation(n, seed, iteration);   // :296-297
            std::vector<float> sb(merge_weighted ? 0 : n * 84), sp(n * 7), sv(n);
            std::vector<uint64_t> ss(as.size());
            std::vector<uint32_t> sw(mult.size());
            size_t weight_sum = 0;
            for (size_t i = 0; i < n; ++i) {
                const size_t src = (size_t)perm[i];
                if (merge_weighted) {                                 // the multiplicities travel with their tuples
                    ss[2 * i] = as[2 * src]; ss[2 * i + 1] = as[2 * src + 1];
                    sw[i] = mult[src];
                    weight_sum += mult[src];
                } else {
                    std::memcpy(&sb[i * 84], &ab[src * 84], 84 * sizeof(float));
                }
                std::memcpy(&sp[i * 7], &ap[src * 7], 7 * sizeof(float));
                sv[i] = av[src];
            }
            e_.check(az_set_option(e_.raw(), "train_seed", (int64_t)(seed + iteration)));
            {
                ScopedOption optim_guard(weight_decay > 0 || clip_norm > 0 || lr_warmup_steps > 0 || lr_decay != 0 || ema_decay > 0,
                                         [&] { e_.set_train_optim(weight_decay, clip_norm, lr_warmup_steps, lr_decay, lr_floor, ema_decay); },
                                         [&] { e_.set_train_optim(); });
                // the validation set and its two options hold for this training only
                ScopedOption validation_guard(val_n > 0,
                                              [&] { e_.check(az_set_option(e_.raw(), "train_keep_best", keep_best ? 1 : 0));
                                                    e_.check(az_set_option(e_.raw(), "train_patience", (int64_t)patience)); },
                                              [&] { az_set_option(e_.raw(), "train_keep_best", 0); az_set_option(e_.raw(), "train_patience", 0);
                                                    az_net_train_set_validation(e_.raw(), nullptr, nullptr); });
                if (merge_weighted)       // rows in proportion to the multiplicities, mirrored at random under merge_canonical; an epoch keeps the merged set's cost
                    train_samples(e_, model_id, model_id + 1, (int64_t)n, ss.data(), nullptr, sp.data(), sv.data(), sw.data(), merge_canonical ? AZ_TRAIN_MIRROR : 0);
                else
                    e_.check(az_net_train(e_.raw(), (int32_t)model_id, (int32_t)model_id + 1, sb.data(), sp.data(), sv.data(), (int64_t)n));   // :329
            }
            if (ema_decay > 0) {                                      // the candidate is the averaged model
                if (!az_net_train_ema) throw Panic("ema_decay: the linked engine library has no az_net_train_ema");
                e_.check(az_net_train_ema(e_.raw(), (int32_t)model_id + 1));
            }
            if (rank_ == 0) e_.check(az_net_save(e_.raw(), (int32_t)model_id + 1, (dir_ + "/" + std::to_string(model_id + 1) + ".aznet").c_str()));
            Report r{};
            r.iteration = iteration; r.samples = n; r.samples_raw = n_raw; r.samples_weight = weight_sum; r.model_id = model_id;
            r.losses.resize(2 * (size_t)az_net_train_history(e_.raw(), nullptr, 0));
            az_net_train_history(e_.raw(), r.losses.data(), (int32_t)(r.losses.size() / 2));
            r.val_n = val_n; r.best_epoch = -1;
            r.reanalysed = reanalysed; r.t_reanalyse = t_reanalyse;
            if (val_n > 0) {
                const Validation v = train_validation(e_);
                for (size_t k = 0; k < v.rows.size() / 4; ++k) { r.val_loss_pi.push_back(v.rows[4 * k]); r.val_loss_v.push_back(v.rows[4 * k + 1]); r.val_top1.push_back(v.rows[4 * k + 3]); }
                r.best_epoch = v.best_epoch;
            }
            // arena: new (first listed) vs old, both seatings (:333-375)
            az_arena_params a{};
            a.num_games = (int32_t)num_arena_games; a.num_sims = (int32_t)num_sims; a.max_depth = (int32_t)max_depth; a.cpuct = cpuct;
            a.new_model_id = (int32_t)model_id + 1; a.old_model_id = (int32_t)model_id; a.reserve = mcts_reserve_size;
            a.seed = seed + 7919ull * (uint64_t)(iteration + 1);
            a.num_sim_threads = (int32_t)num_sim_threads;
            if (world_ > 1 || use_comm_at_world_1) {                 // this rank's games of the arena, one 3-counter all-reduce
                const size_t total = 2 * (num_arena_games / 2);      // num/2 per seating (src/arena.rs:83)
                const auto [alo, ahi] = shard_range(total, rank_, world_);
                a.first_game = (int32_t)alo; a.num_games = (int32_t)(ahi - alo); a.total_games = (int32_t)total; a.allreduce_wld = 1;
                if (total == 0) { a.total_games = 0; a.first_game = 0; a.num_games = 0; a.allreduce_wld = 0; }
            }
            if (selfplay_class != AZ_NET_CLASS_ENGINE) {            // the gate is judged in bf16 whatever the episodes were played in
                e_.net_set_class(model_id + 1, AZ_NET_CLASS_BF16);
                e_.net_set_class(model_id, AZ_NET_CLASS_BF16);
            }
            uint64_t wld[3] = {0, 0, 0};
            {
                // paired openings around the gate only: on before az_arena, off again behind it (also when it throws)
                ScopedOption openings_guard(arena_opening_plies > 0, [&] { e_.set_arena_openings(arena_opening_plies); },
                                            [&] { e_.set_arena_openings(0); });
                e_.check(az_arena(e_.raw(), &a, wld, nullptr));
            }
            r.nwins = (size_t)wld[0]; r.pwins = (size_t)wld[1]; r.draws = (size_t)wld[2];
            std::printf("NEW/PREV WINS : %zu / %zu; DRAWS : %zu\n", r.nwins, r.pwins, r.draws);        // :381
            r.accepted = !(r.pwins + r.nwins == 0 || (float)r.nwins / (float)(r.pwins + r.nwins) < update_threshold);   // :383-390
            std::printf(r.accepted ? "ACCEPTING NEW MODEL\n" : "REJECTING NEW MODEL\n");
            if (solve_min_stones > 0) {                               // the exact move-quality report of the arena just played; decides nothing
                if (!az_move_quality || !az_arena_get_moves || !az_arena_get_openings || !az_allreduce_u64)
                    throw Panic("solve_min_stones: the linked engine library has no az_move_quality");
                const bool sharded = a.total_games > 0;
                const size_t local = sharded ? (size_t)a.num_games : 2 * (num_arena_games / 2), total = sharded ? (size_t)a.total_games : local;
                if (local > 0) {
                    std::vector<int32_t> len(local);
                    std::vector<uint8_t> moves(local * AZ_MAX_PLIES);
                    std::vector<uint64_t> boards(local * 2);
                    e_.check(az_arena_get_moves(e_.raw(), len.data(), moves.data()));
                    e_.check(az_arena_get_openings(e_.raw(), boards.data(), nullptr, nullptr));
                    Engine::SolveParams sp;
                    sp.max_nodes = solve_max_nodes; sp.min_stones = (int32_t)solve_min_stones;
                    quality_tally(e_.move_quality(boards.data(), len, moves, sp), sharded ? (size_t)a.first_game : 0, total, r.quality);
                }
                if (world_ > 1 || use_comm_at_world_1) e_.check(az_allreduce_u64(e_.raw(), &r.quality[0][0], 12));
                for (int m = 0; m < 2; ++m)
                    std::printf("MOVE QUALITY %s (from %zu stones): examined %llu kept %llu win->draw %llu win->loss %llu draw->loss %llu unknown %llu\n",
                                m ? "PREV" : "NEW", solve_min_stones, (unsigned long long)r.quality[m][0], (unsigned long long)r.quality[m][1],
                                (unsigned long long)r.quality[m][2], (unsigned long long)r.quality[m][3], (unsigned long long)r.quality[m][4],
                                (unsigned long long)r.quality[m][5]);
            }
            // a long run moves to a new model id per accepted iteration: drop the slot nobody will read again
            e_.check(az_net_free(e_.raw(), (int32_t)(r.accepted ? model_id : model_id + 1)));
            if (r.accepted) ++model_id;
            if (rank_ == 0) {
                const std::string tmp = dir_ + "/coach.state.tmp";
                if (FILE* f = std::fopen(tmp.c_str(), "w")) {
                    std::fprintf(f, "%zu %zu\n", iteration, model_id);
                    std::fclose(f);
                    std::filesystem::rename(tmp, dir_ + "/coach.state");
                }
            }
            this->model_id = model_id;
            report.push_back(std::move(r));
        }
        return report;
    }

    std::deque<HistoryEntry> history;
    size_t start_iteration = 0, model_id = 0;
    size_t mcts_reserve_size = 0, temp_threshold = 0, max_history_length = 0, max_queue_length = 0, num_episode_threads = 0,
           num_arena_games = 0, num_iters = 0, num_eps = 0, num_sims = 0, max_depth = 0, num_sim_threads = 1;
    bool use_comm_at_world_1 = false;     // tests: run the gather / all-reduce path at world size 1
    // AZ_NET_CLASS_FP8: every iteration pins the playing model to fp8 before az_selfplay and both arena models to bf16 before
    // az_arena (the superseded id's class goes with az_net_free); training is untouched.  ENGINE (default): no class call at all
    az_net_class selfplay_class = AZ_NET_CLASS_ENGINE;
    // Dirichlet root noise of the episodes (Engine::set_root_noise): set before every az_selfplay and cleared behind it.  eps 0 (the
    // default): the engine is never asked
    double root_noise_eps = 0.0, root_noise_alpha = 1.0;
    // Playout cap randomization of the episodes (Engine::set_playout_cap): set before every az_selfplay and cleared behind it.  sims 0
    // (the default): the engine is never asked.  An iteration then yields the tuples of the full moves only
    int64_t playout_cap_sims = 0;
    double playout_cap_full = 0.25;
    // Forced playouts and policy target pruning of the episodes (Engine::set_forced_playouts): set before every az_selfplay and cleared
    // behind it.  k 0 (the default): the engine is never asked
    double forced_playouts_k = 0.0;
    bool policy_prune = false;
    // Gumbel root search with sequential halving of the episodes (Engine::set_gumbel): set before every az_selfplay and cleared behind it
    // (the engine refuses it together with forced playouts).  m 0 (the default): the engine is never asked
    int64_t gumbel_m = 0;
    double gumbel_c_visit = 50.0, gumbel_c_scale = 1.0;
    // Paired openings of the gate (Engine::set_arena_openings): set before the iteration's az_arena and cleared behind it.  0 (the
    // default): the engine is never asked
    int64_t arena_opening_plies = 0;
    // "eval_mirror" (Engine::set_eval_mirror): set ONCE at the start of learn() for the whole loop -- the episodes and the arena gate both
    // run under the mirror-canonical function, so the gate compares like with like.  false (the default): the engine is never asked
    bool eval_mirror = false;
    // The decided-move stop (az_host::set_search_stop; include/az_search_stop.h): set ONCE at the start of learn() for the whole loop -- the
    // episodes' temperature-0 moves and every move of the arena gate end once they can no longer change.  false (the default): the engine is
    // never asked
    bool search_stop = false;
    // Position averaging (az_samples_merge): every iteration's concatenated window is merged to one tuple per distinct position before
    // the shuffle, so the shuffle and NNet::train see the merged set; `history` and the <iter>.examples files stay raw.  merge_canonical
    // also merges a position with its mirror image: the window already holds both orientations (symmetries are expanded before it is merged)
    // and nothing expands them again, so the net then trains on the CANONICAL orientation of every position only -- half the set; meant to
    // go with eval_mirror, which evaluates on that orientation.  false (the default): the engine is never asked
    bool merge_positions = false, merge_canonical = false;
    // merge_weighted (requires merge_positions): the merge's multiplicities are kept, shuffled with their tuples, and NNet::train draws every
    // batch row in proportion to them (az_net_train_samples, from the merged STATES: no feature planes are made) -- the raw window's
    // distribution at the merged set's size and step count; under merge_canonical rows are mirrored at random (AZ_TRAIN_MIRROR), so the net
    // sees both orientations again.  Report::samples_weight is the sum of the multiplicities (= samples_raw).  Files on disk stay raw.
    // false (the default): the counts are dropped and az_net_train runs as before
    bool merge_weighted = false;
    // The optimiser rules of NNet::train (Engine::set_train_optim): decoupled weight decay, gradient-norm clipping, warm-up and decay of the
    // learning rate (lr_decay 0 none / 1 cosine / 2 linear, over the call's own steps) and an averaged shadow of the weights, set before
    // the iteration's one az_net_train and cleared behind it.  With ema_decay > 0 the candidate -- what the arena gates, what is saved as
    // <id>.aznet and what the next iteration trains from -- is the averaged model (az_net_train_ema).  All 0 (the default): the engine is
    // never asked
    double weight_decay = 0.0, clip_norm = 0.0;
    int64_t lr_warmup_steps = 0, lr_decay = 0;
    double lr_floor = 0.0, ema_decay = 0.0;
    // Move-quality report (az_move_quality): after every iteration's arena its games are replayed, every position with at least
    // solve_min_stones stones is solved exactly (budget solve_max_nodes per position and action) and the move played there classed; the
    // tally per model goes into Report::quality and one log line each.  It decides nothing: the gate, the checkpoints, the .examples files
    // and coach.state are those of a run without it.  0 (the default): the engine is never asked
    size_t solve_min_stones = 0;
    uint32_t solve_max_nodes = 1u << 20;
    // Search statistics as targets (az_samples_blend_z / az_samples_surprise; csrc/az_target.h).  Either one sets "selfplay_record_search"
    // before every az_selfplay and clears it behind it.  value_target_q (0 .. 1): right behind self-play the rank's own zs become
    // (1 - q) * z + q * R, R the root value of the tuple's search -- before any gather, so the result does not depend on the world size.
    // surprise_share (0 .. 1): the rank's own tuples are replaced by az_samples_surprise's resampling (seed = seed + iteration) -- before the
    // gather and the symmetry expansion; refused with a world above 1 (the normalisation would be per shard).  History, the .examples
    // files, the merge and the trainers see ordinary tuples; merge_positions + merge_weighted turn the duplicates back into draw weights.
    // Both 0 (the default): the engine is never asked
    double value_target_q = 0.0, surprise_share = 0.0;
    // Reanalyse (az_reanalyse; include/az_reanalyse.h).  reanalyse_sims > 0: every iteration, once the new window is
    // appended and the oldest dropped and BEFORE the .examples file is written, the pi of every tuple of every older history entry is
    // replaced by a fresh search of reanalyse_sims simulations with the current model (reanalyse_history above; temp 1, seed + iteration,
    // game ids reanalyse_first_game_id(iteration, entry) + tuple).  The file holds what was trained on, so a resumed run is byte-identical.
    // Report::reanalysed / t_reanalyse.  0 (the default): the engine is never asked and every file is what it was
    size_t reanalyse_sims = 0;
    // Held-out validation (az_samples_holdout / az_net_train_set_validation; csrc/az_score.h).  validation_share (0 .. 1): every iteration the
    // assembled window is split by the hold-out rule BEFORE merge and shuffle, with learn()'s constant seed -- a function of the position
    // alone, so a position (and its mirror image) is on the same side in every iteration; the rest is trained on, the held-out part is
    // registered raw and scored at the end of every epoch (Report::val_*, best_epoch).  keep_best stores the best epoch's weights, patience
    // > 0 stops after that many epochs without a new best.  History and the .examples files keep every tuple.  0 (the default): the engine
    // is never asked and reports and files are what they were
    double validation_share = 0.0;
    bool keep_best = false;
    size_t patience = 0;
    float update_threshold = 0.f;
    int32_t cpuct = 1;

  private:
    explicit Coach(Engine& e) : e_(e) {}
    Engine& e_;
    std::string dir_;
    int rank_ = 0, world_ = 1;
};

}  // namespace az_host
