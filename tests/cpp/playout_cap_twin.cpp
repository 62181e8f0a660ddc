// playout_cap_twin.cpp -- the CPU twin of playout cap randomization ("playout_cap_sims" / "playout_cap_full_e6", include/az_engine.h).
// TEST INFRASTRUCTURE ONLY.
//
// The oracle (oracle/az_oracle.hpp) has one simulation budget per AsyncMcts and records every ply; it stays as it is.  Everything in it is
// a public struct and AsyncMcts::num_sims is a plain field, so the feature is restated AROUND it: the episode loop of noise_twin.cpp
// (included for its helpers), which per move evaluates the predicate of csrc/az_playout.h (the g++ build of the text the kernels
// compile), sets the budget, searches with noise only when the move is full and eps > 0 (otherwise the oracle's plain get_action_prob,
// never a noisy call with eps = 0), and records full moves only.  Built by the tests with g++ -O2 -ffp-contract=off into a shared
// library driven through ctypes (tests/playout_cap_twin.py).
#include "noise_twin.cpp"
#include "az_playout.h"

namespace {

struct CapEpisode {
    std::vector<TrainingSample> samples;
    std::vector<uint8_t> moves;
    uint64_t full_mask = 0, sims = 0, budgets = 0;
};

// Coach::execute_episode (src/coach.rs:104-157) with a playout cap: n_full = num_sims, n_fast = playout_cap_sims
template <class G>
CapEpisode capped_episode(AsyncMcts<G>& mcts, const Noise& nz, size_t n_full, size_t n_fast, uint32_t thresh24, size_t temp_threshold, uint64_t seed,
                          uint64_t game_id) {
    struct Ex { std::vector<float> f; int8_t player; std::vector<float> pi; };
    std::vector<Ex> train_examples;
    CapEpisode out;
    G board = G::get_init_board();
    int8_t cur_player = 1;
    size_t episode_step = 0;
    for (;;) {
        episode_step += 1;
        G canonical = board.get_canonical_form(cur_player);
        const float temp = episode_step < temp_threshold ? 1.0f : 0.0f;
        const uint64_t ply = episode_step - 1;
        const bool full = az::playout_cap_full(seed, game_id, ply, thresh24);
        mcts.num_sims = full ? n_full : n_fast;
        out.budgets += mcts.num_sims;
        std::vector<float> pi = (full && nz.eps > 0.0f) ? noisy_get_action_prob(mcts, nz, canonical, temp, seed, game_id, ply)
                                                        : mcts.get_action_prob(canonical, temp, seed, game_id, ply);
        if (full) {
            out.full_mask |= 1ull << ply;
            for (auto& bp : canonical.get_symmetries(pi)) train_examples.push_back({bp.first.to_features(), cur_player, bp.second});
        }
        const uint64_t r64 = rng_draw(seed, game_id, ply, RNG_MOVE);
        const uint8_t action = (uint8_t)rng_choose_weighted(r64, pi.data(), (int)pi.size());
        out.moves.push_back(action);
        auto nx = board.get_next_state(cur_player, action);
        board = nx.first;
        cur_player = nx.second;
        const float r = board.get_game_ended(cur_player);
        if (r != 0.0f) {
            for (auto& ex : train_examples) out.samples.push_back({ex.f, ex.pi, r * (ex.player == cur_player ? 1.0f : -1.0f)});
            out.sims = mcts.stats.sims;
            return out;
        }
    }
}

}  // namespace

extern "C" {

// the host build of the predicate: out[i] = 1 when the move (seed, game_ids[i], plies[i]) is full at P = full_e6
void twin_playout_full(int64_t n, uint64_t seed, const uint64_t* game_ids, const uint64_t* plies, int64_t full_e6, uint8_t* out) {
    const uint32_t th = az::playout_cap_thresh24((uint64_t)full_e6);
    for (int64_t i = 0; i < n; ++i) out[i] = az::playout_cap_full(seed, game_ids[i], plies[i], th) ? 1 : 0;
}
uint32_t twin_playout_thresh24(int64_t full_e6) { return az::playout_cap_thresh24((uint64_t)full_e6); }

// Coach::execute_episode x n_games with a playout cap (and root noise on the full moves): twin_selfplay's outputs plus the full-ply masks
// [n_games] and sims_out[2] = {the oracle's simulation counter, the sum of the budgets}, both summed over the episodes
int64_t twin_capped_selfplay(int64_t n_games, uint64_t first_game_id, uint64_t sims, uint64_t cap_sims, int64_t full_e6, uint64_t temp_threshold, int cpuct,
                             uint64_t max_depth, uint64_t reserve, uint64_t seed, int net_kind, uint64_t salt, int game_kind, int sim_threads,
                             int64_t eps_e6, int64_t alpha_e6, float* boards, float* pis, float* zs, int64_t cap, int32_t* game_len, uint8_t* moves,
                             uint64_t* full_masks, uint64_t* sims_out, const int64_t* rec_off, const uint64_t* rec_states, const float* rec_pi,
                             const float* rec_v, int32_t* replay_bad) {
    const Noise nz(eps_e6, alpha_e6);
    const size_t ST = sim_threads > 0 ? (size_t)sim_threads : 1;
    const uint32_t th = az::playout_cap_thresh24((uint64_t)full_e6);
    int64_t n = 0;
    sims_out[0] = sims_out[1] = 0;
    try {
        for (int64_t g = 0; g < n_games; ++g) {
            Nets nets;
            nets.hash.salt = salt;
            if (net_kind == 2) {
                nets.replay.states = rec_states ? rec_states + 2 * rec_off[g] : nullptr;
                nets.replay.pis = rec_pi + 7 * rec_off[g];
                nets.replay.vs = rec_v + rec_off[g];
                nets.replay.n = (size_t)(rec_off[g + 1] - rec_off[g]);
            }
            CapEpisode ep;
            if (game_kind == 2) {
                AsyncMcts<C3Bits> m(reserve, sims, ST, max_depth, 0, cpuct, nets.get(net_kind), C4_W);
                ep = capped_episode<C3Bits>(m, nz, sims, cap_sims, th, temp_threshold, seed, first_game_id + (uint64_t)g);
            } else {
                AsyncMcts<C4Bits> m(reserve, sims, ST, max_depth, 0, cpuct, nets.get(net_kind), C4_W);
                ep = capped_episode<C4Bits>(m, nz, sims, cap_sims, th, temp_threshold, seed, first_game_id + (uint64_t)g);
            }
            if (replay_bad) replay_bad[g] = (net_kind == 2 && (nets.replay.mismatch || nets.replay.pos != nets.replay.n)) ? 1 : 0;
            game_len[g] = (int32_t)ep.moves.size();
            full_masks[g] = ep.full_mask;
            sims_out[0] += ep.sims;
            sims_out[1] += ep.budgets;
            for (size_t i = 0; i < ep.moves.size() && i < 42; ++i) moves[g * 42 + i] = ep.moves[i];
            for (auto& ts : ep.samples) {
                if (n >= cap) return -1;
                std::memcpy(boards + n * 84, ts.board.data(), 84 * sizeof(float));
                std::memcpy(pis + n * 7, ts.pi.data(), 7 * sizeof(float));
                zs[n] = ts.v;
                ++n;
            }
        }
    } catch (const std::exception&) { return -1; }
    return n;
}

}  // extern "C"
