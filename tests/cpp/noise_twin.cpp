// noise_twin.cpp -- the CPU twin of the Dirichlet root noise ("root_noise_eps_e6", include/az_engine.h).  TEST INFRASTRUCTURE ONLY.
//
// The oracle (oracle/az_oracle.hpp) has no root noise and stays as it is.  Everything in it is a public struct, and its get_action_prob
// skips the root's evaluation when the root already has a prior, so the feature's semantics are restated AROUND it:
//     get_action_prob with noise = look the root up (or create it, S10), make sure it has its prior (S1), mix eta into that prior
//                                  (csrc/az_noise.h, the g++ build of the header the kernels compile), call the oracle's get_action_prob.
// The episode loop of Coach::execute_episode (oracle/az_oracle_games.hpp) is restated around that.  Built by the tests with
// g++ -O2 -ffp-contract=off into a shared library driven through ctypes (tests/noise_twin.py).
#include "az_oracle_games.hpp"
#include "az_noise.h"

using namespace azo;

namespace {

struct Noise {
    float eps = 0.0f, alpha = 1.0f;
    Noise(int64_t eps_e6, int64_t alpha_e6) : eps((float)((double)eps_e6 / 1e6)), alpha((float)((double)alpha_e6 / 1e6)) {}
};

template <class G>
uint32_t valid_mask_of(const std::vector<uint8_t>& v) {
    uint32_t m = 0;
    for (size_t a = 0; a < v.size(); ++a) if (v[a]) m |= 1u << a;
    return m;
}

// the root of get_action_prob(s), with its prior: src/async_mcts.rs:81 + S10 + S1, exactly as AsyncMcts::get_action_prob does it
template <class G>
size_t ensure_root(AsyncMcts<G>& m, const G& s) {
    size_t root;
    auto found = m.nodes->lookup_state_id(s);
    if (found) {
        root = *found;
    } else {
        root = m.nodes->push(Node<G>(WIN_SCALE));
        m.nodes->upgrade(root, s);
        m.stats.expansions++;
    }
    Node<G>* rn = m.nodes->get(root);
    if (rn->e != 0.0f) throw std::runtime_error("get_action_prob: terminal root state");
    if (!rn->p) {
        auto pv = m.evaluate(*rn->s, *rn->v);
        m.nodes->set_policy_unlocked(root, std::move(pv.first));
    }
    return root;
}

// once per get_action_prob, before the first selection: p[a] <- (1 - eps) * p[a] + eps * eta[a] for the valid actions, in place
template <class G>
std::vector<float> noisy_get_action_prob(AsyncMcts<G>& m, const Noise& nz, const G& s, float temp, uint64_t seed, uint64_t game_id, uint64_t ply,
                                         uint16_t* counts = nullptr, float* q = nullptr) {
    const size_t root = ensure_root(m, s);
    Node<G>* rn = m.nodes->get(root);
    const uint32_t vm = valid_mask_of<G>(*rn->v);
    float eta[8];
    az::noise_eta(seed, game_id, ply, nz.alpha, vm, (int)m.action_size, eta);
    std::vector<float>& p = *rn->p;
    for (size_t a = 0; a < m.action_size; ++a)
        if ((vm >> a) & 1u) p[a] = az::noise_mix(nz.eps, p[a], eta[a]);
    return m.get_action_prob(s, temp, seed, game_id, ply, counts, q);
}

// Coach::execute_episode (src/coach.rs:104-157) as oracle/az_oracle_games.hpp restates it, with the noisy get_action_prob
template <class G>
std::vector<TrainingSample> noisy_episode(AsyncMcts<G>& mcts, const Noise& nz, size_t temp_threshold, uint64_t seed, uint64_t game_id,
                                          std::vector<uint8_t>* moves_out) {
    struct Ex { std::vector<float> f; int8_t player; std::vector<float> pi; };
    std::vector<Ex> train_examples;
    G board = G::get_init_board();
    int8_t cur_player = 1;
    size_t episode_step = 0;
    for (;;) {
        episode_step += 1;
        G canonical = board.get_canonical_form(cur_player);
        float temp = episode_step < temp_threshold ? 1.0f : 0.0f;
        uint64_t ply = episode_step - 1;
        std::vector<float> pi = noisy_get_action_prob(mcts, nz, canonical, temp, seed, game_id, ply);
        for (auto& bp : canonical.get_symmetries(pi)) train_examples.push_back({bp.first.to_features(), cur_player, bp.second});
        uint64_t r64 = rng_draw(seed, game_id, ply, RNG_MOVE);
        uint8_t action = (uint8_t)rng_choose_weighted(r64, pi.data(), (int)pi.size());
        if (moves_out) moves_out->push_back(action);
        auto nx = board.get_next_state(cur_player, action);
        board = nx.first;
        cur_player = nx.second;
        float r = board.get_game_ended(cur_player);
        if (r != 0.0f) {
            std::vector<TrainingSample> out;
            for (auto& ex : train_examples) out.push_back({ex.f, ex.pi, r * (ex.player == cur_player ? 1.0f : -1.0f)});
            return out;
        }
    }
}

struct Nets {
    StubNet stub;
    HashNet hash;
    ReplayNet replay;
    NNet* get(int kind) { return kind == 0 ? (NNet*)&stub : kind == 1 ? (NNet*)&hash : (NNet*)&replay; }
};

struct TwinBase {
    virtual ~TwinBase() = default;
    virtual int get_action_prob(uint64_t mine, uint64_t theirs, float temp, uint64_t seed, uint64_t game_id, int64_t eps_e6, int64_t alpha_e6,
                                float* pi, uint16_t* counts, float* q) = 0;
    virtual int root_priors(uint64_t mine, uint64_t theirs, float* out7) = 0;
    virtual Nets& nets() = 0;
};
template <class G>
struct Twin : TwinBase {
    Nets n;
    std::unique_ptr<AsyncMcts<G>> m;
    int get_action_prob(uint64_t mine, uint64_t theirs, float temp, uint64_t seed, uint64_t game_id, int64_t eps_e6, int64_t alpha_e6, float* pi,
                        uint16_t* counts, float* q) override {
        try {
            const G s{mine, theirs};
            auto p = noisy_get_action_prob(*m, Noise(eps_e6, alpha_e6), s, temp, seed, game_id, (uint64_t)__builtin_popcountll(mine | theirs), counts, q);
            for (size_t i = 0; i < p.size(); ++i) pi[i] = p[i];
            return 0;
        } catch (const std::exception&) { return -1; }
    }
    int root_priors(uint64_t mine, uint64_t theirs, float* out7) override {
        auto found = m->nodes->lookup_state_id(G{mine, theirs});
        if (!found || !m->nodes->get(*found)->p) return -1;
        const std::vector<float>& p = *m->nodes->get(*found)->p;
        for (size_t a = 0; a < p.size(); ++a) out7[a] = p[a];
        return 0;
    }
    Nets& nets() override { return n; }
};
template <class G>
TwinBase* make_twin(uint64_t reserve, uint64_t sims, uint64_t threads, uint64_t max_depth, uint64_t model_id, int cpuct, int net_kind, uint64_t salt) {
    auto* t = new Twin<G>();
    t->n.hash.salt = salt;
    t->m.reset(new AsyncMcts<G>(reserve, sims, threads, max_depth, model_id, cpuct, t->n.get(net_kind), C4_W));
    return t;
}

}  // namespace

extern "C" {

// ---- the host build of csrc/az_noise.h ------------------------------------------------------------------------------------------------
// eta_out [n,7] for root states [n,2] on the streams (seed, game_ids[i], stones): what az_root_noise_eta returns from the device
void twin_noise_eta(int64_t n, uint64_t seed, const uint64_t* game_ids, const uint64_t* states, int64_t alpha_e6, float* eta_out) {
    const float alpha = (float)((double)alpha_e6 / 1e6);
    for (int64_t i = 0; i < n; ++i) {
        const C4Bits s{states[2 * i], states[2 * i + 1]};
        az::noise_eta(seed, game_ids[i], (uint64_t)__builtin_popcountll(s.p1 | s.m1), alpha, valid_mask_of<C4Bits>(s.get_valid_moves(1)), C4_W, eta_out + 7 * i);
    }
}
void twin_noise_log2(int64_t n, const float* x, float* out) { for (int64_t i = 0; i < n; ++i) out[i] = az::noise_log2(x[i]); }
void twin_noise_exp2(int64_t n, const float* x, float* out) { for (int64_t i = 0; i < n; ++i) out[i] = az::noise_exp2(x[i]); }

// ---- AsyncMcts with root noise ---------------------------------------------------------------------------------------------------------
// game_kind 0 = Connect Four, 2 = Connect Three (oracle_py.GAME_BITS / GAME_CONNECT3); net_kind 0 stub, 1 hash, 2 replay
void* twin_tree_new(int game_kind, uint64_t reserve, uint64_t sims, uint64_t threads, uint64_t max_depth, uint64_t model_id, int cpuct, int net_kind,
                    uint64_t salt) {
    try {
        if (game_kind == 2) return make_twin<C3Bits>(reserve, sims, threads, max_depth, model_id, cpuct, net_kind, salt);
        return make_twin<C4Bits>(reserve, sims, threads, max_depth, model_id, cpuct, net_kind, salt);
    } catch (const std::exception&) { return nullptr; }
}
void twin_tree_free(void* t) { delete (TwinBase*)t; }
int twin_tree_get_action_prob(void* t, uint64_t mine, uint64_t theirs, float temp, uint64_t seed, uint64_t game_id, int64_t eps_e6, int64_t alpha_e6,
                              float* pi, uint16_t* counts, float* q) {
    return ((TwinBase*)t)->get_action_prob(mine, theirs, temp, seed, game_id, eps_e6, alpha_e6, pi, counts, q);
}
int twin_tree_root_priors(void* t, uint64_t mine, uint64_t theirs, float* out7) { return ((TwinBase*)t)->root_priors(mine, theirs, out7); }
void twin_tree_set_replay(void* t, const uint64_t* states, const float* pis, const float* vs, uint64_t n) {
    ReplayNet& r = ((TwinBase*)t)->nets().replay;
    r.states = states; r.pis = pis; r.vs = vs; r.n = (size_t)n; r.pos = 0; r.mismatch = false;
}
int twin_tree_replay_bad(void* t) { const ReplayNet& r = ((TwinBase*)t)->nets().replay; return (r.mismatch || r.pos != r.n) ? 1 : 0; }

// ---- Coach::execute_episode x n_games with root noise: the outputs of oracle_py.selfplay (azo_selfplay) ------------------------------------
int64_t twin_selfplay(int64_t n_games, uint64_t first_game_id, uint64_t sims, uint64_t temp_threshold, int cpuct, uint64_t max_depth, uint64_t reserve,
                      uint64_t seed, int net_kind, uint64_t salt, int game_kind, int sim_threads, int64_t eps_e6, int64_t alpha_e6, float* boards,
                      float* pis, float* zs, int64_t cap, int32_t* game_len, uint8_t* moves, const int64_t* rec_off, const uint64_t* rec_states,
                      const float* rec_pi, const float* rec_v, int32_t* replay_bad) {
    const Noise nz(eps_e6, alpha_e6);
    const size_t ST = sim_threads > 0 ? (size_t)sim_threads : 1;
    int64_t n = 0;
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
            std::vector<TrainingSample> smp;
            std::vector<uint8_t> mv;
            if (game_kind == 2) {
                AsyncMcts<C3Bits> m(reserve, sims, ST, max_depth, 0, cpuct, nets.get(net_kind), C4_W);
                smp = noisy_episode<C3Bits>(m, nz, temp_threshold, seed, first_game_id + (uint64_t)g, &mv);
            } else {
                AsyncMcts<C4Bits> m(reserve, sims, ST, max_depth, 0, cpuct, nets.get(net_kind), C4_W);
                smp = noisy_episode<C4Bits>(m, nz, temp_threshold, seed, first_game_id + (uint64_t)g, &mv);
            }
            if (replay_bad) replay_bad[g] = (net_kind == 2 && (nets.replay.mismatch || nets.replay.pos != nets.replay.n)) ? 1 : 0;
            game_len[g] = (int32_t)mv.size();
            for (size_t i = 0; i < mv.size() && i < 42; ++i) moves[g * 42 + i] = mv[i];
            for (auto& ts : smp) {
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
