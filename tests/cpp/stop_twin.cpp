// stop_twin.cpp -- the CPU twin of the decided-move stop (include/az_search_stop.h; csrc/az_stop.h).  TEST INFRASTRUCTURE ONLY.
//
// The oracle (oracle/az_oracle.hpp) has no such rule and keeps its behaviour.  The rule is restated AROUND it through its public pieces:
// root_of (the root with its prior), search with the plain field num_sims set to 1 (without root noise a persistent tree driven one
// simulation per call equals one call of as many simulations), policy_of (counts -> pi).  A move of budget B asks the g++ build of
// csrc/az_stop.h -- the text the kernels compile -- before every simulation and stops where it says so.  Around that: one tree (fresh or
// re-used roots), Coach::execute_episode with and without a playout cap, and the arena's play_game with per-game trees and a start board
// per game.  Built by the tests with g++ -O2 -ffp-contract=off into a shared library driven through ctypes (tests/stop_twin.py).
#include "az_oracle_games.hpp"
#include "az_playout.h"
#include "az_stop.h"

using namespace azo;

namespace {

struct Nets {
    StubNet stub;
    HashNet hash;
    NNet* get(int kind) { return kind == 0 ? (NNet*)&stub : (NNet*)&hash; }
};

// the root children's visit counts in slot order, as get_action_prob reads them (a link resolved to its canonical node)
template <class G>
bool root_decided(AsyncMcts<G>& m, size_t root, uint32_t left) {
    uint32_t n[16];
    int k = 0;
    for (size_t child_idx : m.nodes->get(root)->children) n[k++] = (uint32_t)m.nodes->get(child_idx)->get_n();
    return az::stop_decided_counts(n, k, left);
}

// AsyncMcts::get_action_prob with budget B under the rule.  ctr [SS_COUNT] is accumulated into for an eligible move; *ran = the simulations run
template <class G>
std::vector<float> stop_get_action_prob(AsyncMcts<G>& m, bool eligible, size_t B, const G& s, float temp, uint64_t seed, uint64_t game_id, uint64_t ply,
                                        uint64_t* ctr, uint16_t* counts_out = nullptr, float* q_out = nullptr, uint32_t* ran = nullptr) {
    const size_t root = m.root_of(s);
    const size_t keep = m.num_sims;
    size_t i = 0;
    bool stopped = false;
    m.num_sims = 1;
    for (; i < B; ++i) {
        if (eligible && root_decided(m, root, (uint32_t)(B - i))) { stopped = true; break; }
        m.search(root);
    }
    m.num_sims = keep;
    if (eligible && ctr) {
        ctr[az::SS_ELIGIBLE] += 1;
        ctr[az::SS_STOPPED] += stopped ? 1 : 0;
        ctr[az::SS_BUDGET] += B;
        ctr[az::SS_SKIPPED] += B - i;
    }
    if (ran) *ran = (uint32_t)i;
    Node<G>* root_node = m.nodes->get(root);
    std::vector<uint16_t> counts(m.action_size, 0);
    std::vector<float> qs(m.action_size, 0.0f);
    for (size_t child_idx : root_node->children) {
        Node<G>* child = m.nodes->get(child_idx);
        const uint8_t a = m.nodes->raw(child_idx)->a;
        counts[a] = child->get_n();
        qs[a] = child->compute_q();
    }
    if (counts_out) for (size_t a = 0; a < m.action_size; ++a) counts_out[a] = counts[a];
    if (q_out) for (size_t a = 0; a < m.action_size; ++a) q_out[a] = qs[a];
    return m.policy_of(counts, temp, seed, game_id, ply);
}

struct Episode {
    std::vector<TrainingSample> samples;
    std::vector<uint8_t> moves;
    uint64_t full_mask = 0, sims = 0;
};

// Coach::execute_episode (src/coach.rs:104-157) as oracle/az_oracle_games.hpp restates it, with a playout cap (cap_sims > 0: the fast moves'
// budget; they are played, not recorded) and the rule on the moves at temperature 0
template <class G>
Episode stop_episode(AsyncMcts<G>& mcts, bool on, size_t n_full, size_t cap_sims, uint32_t thresh24, size_t temp_threshold, uint64_t seed,
                     uint64_t game_id, uint64_t* ctr) {
    struct Ex { std::vector<float> f; int8_t player; std::vector<float> pi; };
    std::vector<Ex> train_examples;
    Episode out;
    G board = G::get_init_board();
    int8_t cur_player = 1;
    size_t episode_step = 0;
    for (;;) {
        episode_step += 1;
        G canonical = board.get_canonical_form(cur_player);
        const float temp = episode_step < temp_threshold ? 1.0f : 0.0f;
        const uint64_t ply = episode_step - 1;
        const bool full = cap_sims == 0 || az::playout_cap_full(seed, game_id, ply, thresh24);
        const bool eligible = on && az::stop_eligible((int32_t)ply, (int32_t)temp_threshold);
        std::vector<float> pi = stop_get_action_prob(mcts, eligible, full ? n_full : cap_sims, canonical, temp, seed, game_id, ply, ctr);
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

struct TreeBox {
    Nets n;
    std::unique_ptr<AsyncMcts<C4Bits>> m;
};

}  // namespace

extern "C" {

// ---- the host build of csrc/az_stop.h ----------------------------------------------------------------------------------------------------
int stop_twin_decided(const uint32_t* n, int nchild, uint32_t left) { return az::stop_decided_counts(n, nchild, left) ? 1 : 0; }
uint32_t stop_twin_word(uint32_t budget, int eligible) { return az::stop_word(budget, eligible != 0); }
uint32_t stop_twin_left(uint32_t word) { return az::stop_left(word); }
int stop_twin_eligible(int32_t ply, int32_t temp_threshold) { return az::stop_eligible(ply, temp_threshold) ? 1 : 0; }

// ---- one AsyncMcts under the rule (net_kind 0 stub, 1 hash) --------------------------------------------------------------------------------
void* stop_tree_new(uint64_t reserve, uint64_t sims, uint64_t max_depth, uint64_t model_id, int cpuct, int net_kind, uint64_t salt, const uint64_t* root) {
    try {
        auto* t = new TreeBox();
        t->n.hash.salt = salt;
        if (root) t->m.reset(new AsyncMcts<C4Bits>(C4Bits{root[0], root[1]}, reserve, sims, 1, max_depth, model_id, cpuct, t->n.get(net_kind), C4_W));
        else t->m.reset(new AsyncMcts<C4Bits>(reserve, sims, 1, max_depth, model_id, cpuct, t->n.get(net_kind), C4_W));
        return t;
    } catch (const std::exception&) { return nullptr; }
}
void stop_tree_free(void* t) { delete (TreeBox*)t; }
// one get_action_prob of budget `sims` (the tree's own when 0); on != 0 && temp == 0: the move is eligible.  ran_out: the simulations run
int stop_tree_get_action_prob(void* t, uint64_t mine, uint64_t theirs, float temp, uint64_t seed, uint64_t game_id, int on, uint64_t sims, float* pi,
                              uint16_t* counts, float* q, uint32_t* ran_out, uint64_t* ctr) {
    try {
        AsyncMcts<C4Bits>& m = *((TreeBox*)t)->m;
        const C4Bits s{mine, theirs};
        auto p = stop_get_action_prob(m, on != 0 && temp == 0.0f, sims ? (size_t)sims : m.num_sims, s, temp, seed, game_id,
                                      (uint64_t)__builtin_popcountll(mine | theirs), ctr, counts, q, ran_out);
        for (size_t i = 0; i < p.size(); ++i) pi[i] = p[i];
        return 0;
    } catch (const std::exception&) { return -1; }
}

// ---- Coach::execute_episode x n_games under the rule: the outputs of oracle_py.selfplay plus the full-ply masks [n_games], sims_out = the
// oracle's simulation counter summed over the episodes, and ctr [4] ------------------------------------------------------------------------------
int64_t stop_selfplay(int64_t n_games, uint64_t first_game_id, uint64_t sims, uint64_t cap_sims, int64_t full_e6, uint64_t temp_threshold, int cpuct,
                      uint64_t max_depth, uint64_t reserve, uint64_t seed, int net_kind, uint64_t salt, int on, float* boards, float* pis, float* zs,
                      int64_t cap, int32_t* game_len, uint8_t* moves, uint64_t* full_masks, uint64_t* sims_out, uint64_t* ctr) {
    const uint32_t th = az::playout_cap_thresh24((uint64_t)full_e6);
    int64_t n = 0;
    *sims_out = 0;
    for (int i = 0; i < az::SS_COUNT; ++i) ctr[i] = 0;
    try {
        for (int64_t g = 0; g < n_games; ++g) {
            Nets nets;
            nets.hash.salt = salt;
            AsyncMcts<C4Bits> m(reserve, sims, 1, max_depth, 0, cpuct, nets.get(net_kind), C4_W);
            const Episode ep = stop_episode<C4Bits>(m, on != 0, sims, cap_sims, th, temp_threshold, seed, first_game_id + (uint64_t)g, ctr);
            game_len[g] = (int32_t)ep.moves.size();
            full_masks[g] = ep.full_mask;
            *sims_out += ep.sims;
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

// ---- arena::play_game for games [0, n_games) of a `total`-game arena (game gi < total / 2 seats (new, old)), per-game trees, game gi starting
// from start[gi] = {first seat's stones, second seat's} (nullptr: the initial board); every move is eligible while on != 0.  results [n_games],
// moves [n_games][42], len [n_games], sims_out, ctr [4] -------------------------------------------------------------------------------------------
int stop_arena(uint64_t total, uint64_t n_games, uint64_t sims, int cpuct, uint64_t max_depth, uint64_t reserve, uint64_t seed, int net_kind, uint64_t salt,
               int new_model_id, int old_model_id, int on, const uint64_t* start, int8_t* results, uint8_t* moves, int32_t* len, uint64_t* sims_out,
               uint64_t* ctr) {
    *sims_out = 0;
    for (int i = 0; i < az::SS_COUNT; ++i) ctr[i] = 0;
    try {
        const uint64_t half = total / 2;
        for (uint64_t gi = 0; gi < n_games; ++gi) {
            const int first = gi < half ? 0 : 1;
            Nets nets[2];
            nets[0].hash.salt = nets[1].hash.salt = salt;
            AsyncMcts<C4Bits> trees[2] = {AsyncMcts<C4Bits>(reserve, sims, 1, max_depth, (size_t)new_model_id, cpuct, nets[0].get(net_kind), C4_W),
                                          AsyncMcts<C4Bits>(reserve, sims, 1, max_depth, (size_t)old_model_id, cpuct, nets[1].get(net_kind), C4_W)};
            int32_t k = 0;
            auto mk = [&](int slot) {
                return std::function<uint8_t(const C4Bits&)>([&, slot](const C4Bits& s) {
                    const uint64_t ply = (uint64_t)__builtin_popcountll(s.p1 | s.m1);
                    auto p = stop_get_action_prob(trees[slot], on != 0, (size_t)sims, s, 0.0f, seed, gi, ply, ctr);
                    size_t best = 0;
                    for (size_t i = 1; i < p.size(); ++i) if (!(p[best] > p[i])) best = i;       // argmax with max_by (last max), src/coach.rs:356-363
                    if (k < 42) moves[gi * 42 + k] = (uint8_t)best;
                    ++k;
                    return (uint8_t)best;
                });
            };
            std::function<uint8_t(const C4Bits&)> acts[2] = {mk(first), mk(1 - first)};
            std::optional<C4Bits> board0;
            if (start) board0 = C4Bits{start[2 * gi], start[2 * gi + 1]};
            results[gi] = play_game<C4Bits>(acts, board0);
            len[gi] = k;
            *sims_out += trees[0].stats.sims + trees[1].stats.sims;
        }
        return 0;
    } catch (const std::exception&) { return -1; }
}

}  // extern "C"
