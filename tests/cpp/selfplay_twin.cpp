// selfplay_twin.cpp -- the CPU twin of the self-play options the engine has beyond the reference (include/az_engine.h): Dirichlet root
// noise ("root_noise_eps_e6"), playout cap randomization ("playout_cap_sims" / "playout_cap_full_e6"), forced playouts at the root and
// policy target pruning ("forced_playouts_k_e6" / "policy_prune").  TEST INFRASTRUCTURE ONLY.
//
// The oracle (oracle/az_oracle.hpp) has none of them and keeps its behaviour.  The options are restated AROUND it, through its public
// pieces: root_of (the root with its prior), search, policy_of (counts -> pi), the plain field num_sims, and the root_select seam, which
// replaces best_child for the first selection of a simulation.  A FULL move is: root_of, noise mixed into the root's prior when eps > 0,
// search with forced_best_child at the root, counts -> (pruned counts) -> policy_of; it is recorded.  A fast move is the oracle's plain
// get_action_prob at the capped budget; it is only played.  The predicates are the g++ build of csrc/az_noise.h, az_playout.h and
// az_forced.h, the text the kernels compile.  Built by the tests with g++ -O2 -ffp-contract=off into a shared library driven through
// ctypes (tests/selfplay_twin.py).
#include "az_oracle_games.hpp"
#include "az_noise.h"
#include "az_playout.h"
#include "az_forced.h"

#include <limits>

using namespace azo;

namespace {

// what the twin COUNTS: the parity tests assert on these so that they cannot pass vacuously
enum { FC_ROOT_SEL = 0, FC_ROOT_FORCED, FC_ROOT_FORCED_INFLIGHT, FC_MOVES, FC_MOVES_PRUNED, FC_TO_ZERO, FC_VISITS, FC_VISITS_PRUNED, FC_COUNT };

struct Rules {
    float eps = 0.0f, alpha = 1.0f;      // root noise
    size_t cap_sims = 0;                 // playout cap: the fast moves' budget; 0 = every move is full
    uint32_t thresh24 = 0;
    float k = 0.0f;                      // forced playouts
    bool prune = false;
    uint64_t c[FC_COUNT] = {0, 0, 0, 0, 0, 0, 0, 0};
    Rules(int64_t eps_e6, int64_t alpha_e6, uint64_t cap_sims_, int64_t full_e6, int64_t k_e6, int prune_)
        : eps((float)((double)eps_e6 / 1e6)), alpha((float)((double)alpha_e6 / 1e6)), cap_sims((size_t)cap_sims_),
          thresh24(az::playout_cap_thresh24((uint64_t)full_e6)), k(az::forced_k_of(k_e6)), prune(prune_ != 0) {}
};

template <class G>
uint32_t valid_mask_of(const std::vector<uint8_t>& v) {
    uint32_t m = 0;
    for (size_t a = 0; a < v.size(); ++a) if (v[a]) m |= 1u << a;
    return m;
}

// NodeStore::best_child (src/node.rs:343-370) at the root of a forced move: a child with n > 0 && (float)n < nf gets u = +inf
template <class G>
size_t forced_best_child(const NodeStore<G>& ns, size_t idx, int32_t cpuct, bool filter, float k, bool* winner_forced) {
    const Node<G>* node = ns.get(idx);
    const uint16_t parent_n = node->get_n();
    uint32_t S = 0;
    for (size_t child_idx : node->children) S += (uint32_t)ns.get(child_idx)->get_n();
    bool have = false, best_forced = false;
    size_t best = 0;
    float best_u = 0.0f;
    for (size_t child_idx : node->children) {
        const Node<G>* child = ns.get(child_idx);
        const uint8_t ea = ns.raw(child_idx)->a;
        const float p = (*node->p)[ea];
        float u = child->compute_q() + (((float)cpuct * p) * std::sqrt((float)parent_n + EPS)) / (float)(uint16_t)(1 + child->get_n());
        const bool f = az::forced_child(k, p, S, (uint32_t)child->get_n());
        if (f) u = std::numeric_limits<float>::infinity();
        if (filter && ns.state(child_idx) == std::optional<NodeState>(NodeState::Locked)) continue;
        if (!have) { have = true; best = child_idx; best_u = u; best_forced = f; continue; }
        if (!(best_u > u)) { best = child_idx; best_u = u; best_forced = f; }
    }
    if (!have) throw std::runtime_error("best_child: no children");
    *winner_forced = best_forced;
    return best;
}

// AsyncMcts::get_action_prob under the rules.  counts_out / q_out stay raw.
template <class G>
std::vector<float> twin_get_action_prob(AsyncMcts<G>& m, Rules& R, bool full, const G& s, float temp, uint64_t seed, uint64_t game_id, uint64_t ply,
                                        uint16_t* counts_out = nullptr, float* q_out = nullptr) {
    if (!full) return m.get_action_prob(s, temp, seed, game_id, ply, counts_out, q_out);
    const size_t A = m.action_size;
    const size_t root = m.root_of(s);
    if (R.eps > 0.0f) {      // once per call, before the first selection: p[a] <- (1 - eps) * p[a] + eps * eta[a] for the valid actions, in place
        Node<G>* rn = m.nodes->get(root);
        const uint32_t vm = valid_mask_of<G>(*rn->v);
        float eta[8];
        az::noise_eta(seed, game_id, ply, R.alpha, vm, (int)A, eta);
        std::vector<float>& p = *rn->p;
        for (size_t a = 0; a < A; ++a)
            if ((vm >> a) & 1u) p[a] = az::noise_mix(R.eps, p[a], eta[a]);
    }
    {
        struct Unhook { AsyncMcts<G>& m; ~Unhook() { m.root_select = nullptr; } } unhook{m};
        // a root selection STANDS unless its winner is Locked: select_phase then retries it filtered, or abandons the simulation (S11)
        m.root_select = [&](size_t idx, bool filter, size_t thread) {
            bool wf = false;
            const size_t c = forced_best_child(*m.nodes, idx, m.cpuct, filter, R.k, &wf);
            if (!filter) R.c[FC_ROOT_SEL]++;
            if (wf && m.nodes->state(c) != std::optional<NodeState>(NodeState::Locked)) {
                R.c[FC_ROOT_FORCED]++;
                if (thread > 0) R.c[FC_ROOT_FORCED_INFLIGHT]++;      // earlier simulations of this step are still in flight
            }
            return c;
        };
        m.search(root);
    }
    Node<G>* root_node = m.nodes->get(root);
    std::vector<uint16_t> counts(A, 0);
    std::vector<float> qs(A, 0.0f);
    const size_t nchild = root_node->children.size();
    std::vector<uint32_t> n_j(nchild);
    std::vector<float> q_j(nchild), p_j(nchild);
    std::vector<uint8_t> a_j(nchild);
    uint32_t S = 0;
    for (size_t j = 0; j < nchild; ++j) {
        const size_t child_idx = root_node->children[j];
        Node<G>* child = m.nodes->get(child_idx);
        a_j[j] = m.nodes->raw(child_idx)->a;
        n_j[j] = child->get_n();
        q_j[j] = child->compute_q();
        p_j[j] = (*root_node->p)[a_j[j]];
        S += n_j[j];
        counts[a_j[j]] = (uint16_t)n_j[j];
        qs[a_j[j]] = q_j[j];
    }
    if (counts_out) for (size_t i = 0; i < A; ++i) counts_out[i] = counts[i];
    if (q_out) for (size_t i = 0; i < A; ++i) q_out[i] = qs[i];
    std::vector<uint16_t> pruned = counts;
    if (R.prune && R.k > 0.0f) {
        size_t b = 0;
        for (size_t j = 0; j < nchild; ++j) if (n_j[j] >= n_j[b]) b = j;       // the most visited slot, the highest among equals
        const float sq = az::forced_sqrt_parent((uint32_t)root_node->get_n());
        const float u_star = az::forced_puct(q_j[b], n_j[b], p_j[b], sq, (float)m.cpuct);
        bool changed = false;
        for (size_t j = 0; j < nchild; ++j) {
            if (j == b || n_j[j] == 0) continue;
            const uint32_t mj = az::forced_prune(R.k, p_j[j], S, n_j[j], q_j[j], sq, (float)m.cpuct, u_star);
            pruned[a_j[j]] = (uint16_t)mj;
            if (mj != n_j[j]) changed = true;
            if (mj == 0 && n_j[j] >= 2 && az::forced_prune_loop(R.k, p_j[j], S, n_j[j], q_j[j], sq, (float)m.cpuct, u_star) == 1) R.c[FC_TO_ZERO]++;   // the single-playout rule
            R.c[FC_VISITS_PRUNED] += n_j[j] - mj;
        }
        if (changed) R.c[FC_MOVES_PRUNED]++;
    }
    R.c[FC_MOVES]++;
    R.c[FC_VISITS] += S;
    return m.policy_of(pruned, temp, seed, game_id, ply);
}

struct Episode {
    std::vector<TrainingSample> samples;
    std::vector<uint8_t> moves;
    uint64_t full_mask = 0, sims = 0, budgets = 0;
};

// Coach::execute_episode (src/coach.rs:104-157) as oracle/az_oracle_games.hpp restates it, under the rules: n_full = num_sims,
// n_fast = playout_cap_sims; full moves are searched by twin_get_action_prob and recorded, fast moves are only played
template <class G>
Episode twin_episode(AsyncMcts<G>& mcts, Rules& R, size_t n_full, size_t temp_threshold, uint64_t seed, uint64_t game_id) {
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
        const bool full = R.cap_sims == 0 || az::playout_cap_full(seed, game_id, ply, R.thresh24);
        mcts.num_sims = full ? n_full : R.cap_sims;
        out.budgets += mcts.num_sims;
        std::vector<float> pi = twin_get_action_prob(mcts, R, full, canonical, temp, seed, game_id, ply);
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

struct Nets {
    StubNet stub;
    HashNet hash;
    ReplayNet replay;
    NNet* get(int kind) { return kind == 0 ? (NNet*)&stub : kind == 1 ? (NNet*)&hash : (NNet*)&replay; }
    bool replay_bad() const { return replay.mismatch || replay.pos != replay.n; }
};

template <class G>
Episode play_episode(Nets& nets, Rules& R, uint64_t reserve, uint64_t sims, size_t threads, uint64_t max_depth, int cpuct, int net_kind,
                     uint64_t temp_threshold, uint64_t seed, uint64_t game_id) {
    AsyncMcts<G> m(reserve, sims, threads, max_depth, 0, cpuct, nets.get(net_kind), C4_W);
    return twin_episode<G>(m, R, sims, temp_threshold, seed, game_id);
}

struct TreeBase {
    Nets n;
    virtual ~TreeBase() = default;
    virtual int get_action_prob(uint64_t mine, uint64_t theirs, float temp, uint64_t seed, uint64_t game_id, Rules& R, float* pi, uint16_t* counts,
                                float* q) = 0;
    virtual int root_priors(uint64_t mine, uint64_t theirs, float* out7) = 0;
};
template <class G>
struct Tree : TreeBase {
    std::unique_ptr<AsyncMcts<G>> m;
    int get_action_prob(uint64_t mine, uint64_t theirs, float temp, uint64_t seed, uint64_t game_id, Rules& R, float* pi, uint16_t* counts,
                        float* q) override {
        try {
            auto p = twin_get_action_prob(*m, R, true, G{mine, theirs}, temp, seed, game_id, (uint64_t)__builtin_popcountll(mine | theirs), counts, q);
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
};
template <class G>
TreeBase* make_tree(uint64_t reserve, uint64_t sims, uint64_t threads, uint64_t max_depth, uint64_t model_id, int cpuct, int net_kind, uint64_t salt) {
    auto* t = new Tree<G>();
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

// ---- the host build of csrc/az_playout.h: out[i] = 1 when the move (seed, game_ids[i], plies[i]) is full at P = full_e6 ---------------------
void twin_playout_full(int64_t n, uint64_t seed, const uint64_t* game_ids, const uint64_t* plies, int64_t full_e6, uint8_t* out) {
    const uint32_t th = az::playout_cap_thresh24((uint64_t)full_e6);
    for (int64_t i = 0; i < n; ++i) out[i] = az::playout_cap_full(seed, game_ids[i], plies[i], th) ? 1 : 0;
}
uint32_t twin_playout_thresh24(int64_t full_e6) { return az::playout_cap_thresh24((uint64_t)full_e6); }

// ---- the host build of csrc/az_forced.h, element by element: nf, the forced predicate and the pruned count of one slot ----------------------
int twin_forced_counters() { return FC_COUNT; }
void twin_forced_eval(int64_t n, const int64_t* k_e6, const float* p, const uint32_t* S, const uint32_t* nn, const float* q, const uint32_t* n_root,
                      float cpuct, const float* u_star, float* nf_out, uint8_t* forced_out, uint32_t* m_out, float* sq_out) {
    for (int64_t i = 0; i < n; ++i) {
        const float k = az::forced_k_of(k_e6[i]);
        nf_out[i] = az::forced_nf(k, p[i], S[i]);
        forced_out[i] = az::forced_child(k, p[i], S[i], nn[i]) ? 1 : 0;
        const float sq = az::forced_sqrt_parent(n_root[i]);
        sq_out[i] = sq;
        m_out[i] = az::forced_prune(k, p[i], S[i], nn[i], q[i], sq, cpuct, u_star[i]);
    }
}
// u = q + ((cpuct * p) * sq) / (float)(u16)(n + 1): the PUCT value as the header restates it
void twin_forced_puct(int64_t n, const float* q, const uint32_t* nn, const float* p, const uint32_t* n_root, float cpuct, float* out) {
    for (int64_t i = 0; i < n; ++i) out[i] = az::forced_puct(q[i], nn[i], p[i], az::forced_sqrt_parent(n_root[i]), cpuct);
}

// ---- one AsyncMcts under the rules: every get_action_prob is a full move -----------------------------------------------------------------------
// game_kind 0 = Connect Four, 2 = Connect Three (oracle_py.GAME_BITS / GAME_CONNECT3); net_kind 0 stub, 1 hash, 2 replay
void* twin_tree_new(int game_kind, uint64_t reserve, uint64_t sims, uint64_t threads, uint64_t max_depth, uint64_t model_id, int cpuct, int net_kind,
                    uint64_t salt) {
    try {
        if (game_kind == 2) return make_tree<C3Bits>(reserve, sims, threads, max_depth, model_id, cpuct, net_kind, salt);
        return make_tree<C4Bits>(reserve, sims, threads, max_depth, model_id, cpuct, net_kind, salt);
    } catch (const std::exception&) { return nullptr; }
}
void twin_tree_free(void* t) { delete (TreeBase*)t; }
// ctr [FC_COUNT] is ACCUMULATED into
int twin_tree_get_action_prob(void* t, uint64_t mine, uint64_t theirs, float temp, uint64_t seed, uint64_t game_id, int64_t eps_e6, int64_t alpha_e6,
                              int64_t k_e6, int prune, float* pi, uint16_t* counts, float* q, uint64_t* ctr) {
    Rules R(eps_e6, alpha_e6, 0, 0, k_e6, prune);
    const int rc = ((TreeBase*)t)->get_action_prob(mine, theirs, temp, seed, game_id, R, pi, counts, q);
    if (rc == 0) for (int i = 0; i < FC_COUNT; ++i) ctr[i] += R.c[i];
    return rc;
}
int twin_tree_root_priors(void* t, uint64_t mine, uint64_t theirs, float* out7) { return ((TreeBase*)t)->root_priors(mine, theirs, out7); }
void twin_tree_set_replay(void* t, const uint64_t* states, const float* pis, const float* vs, uint64_t n) {
    ReplayNet& r = ((TreeBase*)t)->n.replay;
    r.states = states; r.pis = pis; r.vs = vs; r.n = (size_t)n; r.pos = 0; r.mismatch = false;
}
int twin_tree_replay_bad(void* t) { return ((TreeBase*)t)->n.replay_bad() ? 1 : 0; }

// ---- Coach::execute_episode x n_games under the rules: the outputs of oracle_py.selfplay (azo_selfplay) plus the full-ply masks [n_games],
// sims_out[2] = {the oracle's simulation counter, the sum of the budgets}, both summed over the episodes, and ctr [FC_COUNT] ------------------
int64_t twin_selfplay(int64_t n_games, uint64_t first_game_id, uint64_t sims, uint64_t cap_sims, int64_t full_e6, uint64_t temp_threshold, int cpuct,
                      uint64_t max_depth, uint64_t reserve, uint64_t seed, int net_kind, uint64_t salt, int game_kind, int sim_threads, int64_t eps_e6,
                      int64_t alpha_e6, int64_t k_e6, int prune, float* boards, float* pis, float* zs, int64_t cap, int32_t* game_len, uint8_t* moves,
                      uint64_t* full_masks, uint64_t* sims_out, uint64_t* ctr, const int64_t* rec_off, const uint64_t* rec_states, const float* rec_pi,
                      const float* rec_v, int32_t* replay_bad) {
    Rules R(eps_e6, alpha_e6, cap_sims, full_e6, k_e6, prune);
    const size_t ST = sim_threads > 0 ? (size_t)sim_threads : 1;
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
            const uint64_t game_id = first_game_id + (uint64_t)g;
            const Episode ep = game_kind == 2 ? play_episode<C3Bits>(nets, R, reserve, sims, ST, max_depth, cpuct, net_kind, temp_threshold, seed, game_id)
                                              : play_episode<C4Bits>(nets, R, reserve, sims, ST, max_depth, cpuct, net_kind, temp_threshold, seed, game_id);
            replay_bad[g] = (net_kind == 2 && nets.replay_bad()) ? 1 : 0;
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
    for (int i = 0; i < FC_COUNT; ++i) ctr[i] = R.c[i];
    return n;
}

}  // extern "C"
