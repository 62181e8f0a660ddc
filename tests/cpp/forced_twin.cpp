// forced_twin.cpp -- the CPU twin of forced playouts and policy target pruning ("forced_playouts_k_e6" / "policy_prune",
// include/az_engine.h).  TEST INFRASTRUCTURE ONLY.
//
// The oracle (oracle/az_oracle.hpp) has neither and stays as it is.  Everything in it is a public struct, so the feature is restated
// AROUND it: copies of search_iteration / select_phase / search_lockstep that differ from the oracle's ONLY in calling forced_best_child
// where the oracle calls best_child on the loop's first pass (the node is the call's root), and a get_action_prob that prunes the counts
// before pi is formed.  The predicates are the g++ build of csrc/az_forced.h, the text the kernels compile.  The episode loop is that of
// playout_cap_twin.cpp (included for its helpers: root noise, playout cap, replay net), so the three features compose: a FORCED MOVE is a
// full move; a fast move is the oracle's plain get_action_prob.  Built by the tests with g++ -O2 -ffp-contract=off into a shared library
// driven through ctypes (tests/forced_twin.py).
#include "playout_cap_twin.cpp"
#include "az_forced.h"

#include <limits>

namespace {

// what the twin COUNTS: the parity tests assert on these so that they cannot pass vacuously
enum { FC_ROOT_SEL = 0, FC_ROOT_FORCED, FC_ROOT_FORCED_INFLIGHT, FC_MOVES, FC_MOVES_PRUNED, FC_TO_ZERO, FC_VISITS, FC_VISITS_PRUNED, FC_COUNT };
struct Forced {
    float k = 0.0f;
    bool prune = false;
    uint64_t c[FC_COUNT] = {0, 0, 0, 0, 0, 0, 0, 0};
    Forced(int64_t k_e6, int prune_) : k(az::forced_k_of(k_e6)), prune(prune_ != 0) {}
};

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

// AsyncMcts::search_iteration with the forced root
template <class G>
void f_search_iteration(AsyncMcts<G>& m, size_t root_idx, Forced& F) {
    auto& nodes = m.nodes;
    m.stats.sims++;
    size_t cur = root_idx;
    std::vector<size_t> node_path;
    node_path.reserve(64);
    size_t depth = 0;
    float v;
    bool at_root = true;
    for (;;) {
        Node<G>* head = nodes->get(cur);
        head->visit();
        if (depth > m.max_depth) { v = head->s->eval_heuristic(); break; }
        if (head->e != 0.0f) { v = head->e; m.stats.terminal_hits++; break; }
        size_t c;
        if (at_root) {
            bool wf = false;
            c = forced_best_child(*nodes, cur, m.cpuct, false, F.k, &wf);
            F.c[FC_ROOT_SEL]++;
            if (wf) F.c[FC_ROOT_FORCED]++;
            at_root = false;
        } else {
            c = nodes->best_child(cur, m.cpuct, false);
        }
        m.stats.depth_sum++;
        auto st = nodes->state(c);
        if (st == std::optional<NodeState>(NodeState::PlaceHolder)) {
            nodes->lock(c);
            node_path.push_back(cur);
            size_t parent = cur;
            cur = c;
            Node<G>* node_p = nodes->get(parent);
            uint8_t act = m.quirks.b1_parent_action ? node_p->a : nodes->raw(c)->a;
            auto nx = node_p->s->get_next_state(1, act);
            G s2 = nx.first.get_canonical_form(nx.second);
            auto up = nodes->upgrade(c, s2);
            if (!*up) {
                m.stats.link_hits++;
                cur = *nodes->resolve(c);
                continue;
            }
            m.stats.expansions++;
            Node<G>* leaf = nodes->get(c);
            leaf->visit();
            if (leaf->e != 0.0f) {
                nodes->unlock(c);
                v = leaf->e;
                break;
            }
            auto pv = m.evaluate(*leaf->s, *leaf->v);
            nodes->set_policy(c, std::move(pv.first));
            nodes->unlock(c);
            v = -pv.second;
            break;
        } else {
            node_path.push_back(cur);
            cur = *nodes->resolve(c);
            depth += 1;
        }
    }
    float x = v;
    nodes->get(cur)->unvisit(x);
    while (!node_path.empty()) {
        cur = node_path.back();
        node_path.pop_back();
        if (!m.quirks.b2_same_sign_backup) x = -x;
        nodes->get(cur)->unvisit(x);
    }
}

// AsyncMcts::select_phase with the forced root; thread = the simulation's index within its lock-step step
template <class G>
typename AsyncMcts<G>::Pending f_select_phase(AsyncMcts<G>& m, size_t root_idx, Forced& F, size_t thread) {
    auto& nodes = m.nodes;
    m.stats.sims++;
    typename AsyncMcts<G>::Pending pd;
    pd.cur = root_idx;
    pd.node_path.reserve(64);
    size_t depth = 0;
    bool cur_visited = false, at_root = true;
    auto abandon = [&]() {
        for (size_t idx : pd.node_path) nodes->get(idx)->revert_visit();
        if (cur_visited) nodes->get(pd.cur)->revert_visit();
        pd.kind = 2;
        m.stats.abandoned++;
    };
    for (;;) {
        size_t cur = pd.cur;
        cur_visited = false;
        if (nodes->state(cur) == std::optional<NodeState>(NodeState::Locked)) { abandon(); return pd; }
        Node<G>* head = nodes->get(cur);
        head->visit();
        cur_visited = true;
        if (depth > m.max_depth) { pd.v = head->s->eval_heuristic(); return pd; }
        if (head->e != 0.0f) { pd.v = head->e; m.stats.terminal_hits++; return pd; }
        const bool root_pass = at_root;
        at_root = false;
        bool wf = false;
        size_t c = root_pass ? forced_best_child(*nodes, cur, m.cpuct, false, F.k, &wf) : nodes->best_child(cur, m.cpuct, false);
        m.stats.depth_sum++;
        if (root_pass) F.c[FC_ROOT_SEL]++;
        if (nodes->state(c) == std::optional<NodeState>(NodeState::Locked)) {
            if (nodes->all_children_locked(cur)) { abandon(); return pd; }
            c = root_pass ? forced_best_child(*nodes, cur, m.cpuct, true, F.k, &wf) : nodes->best_child(cur, m.cpuct, true);
        }
        if (root_pass && wf) {
            F.c[FC_ROOT_FORCED]++;
            if (thread > 0) F.c[FC_ROOT_FORCED_INFLIGHT]++;      // earlier simulations of this step are still in flight
        }
        auto st = nodes->state(c);
        if (st == std::optional<NodeState>(NodeState::PlaceHolder)) {
            nodes->lock(c);
            pd.node_path.push_back(cur);
            size_t parent = cur;
            pd.cur = c;
            Node<G>* node_p = nodes->get(parent);
            uint8_t act = m.quirks.b1_parent_action ? node_p->a : nodes->raw(c)->a;
            auto nx = node_p->s->get_next_state(1, act);
            G s2 = nx.first.get_canonical_form(nx.second);
            auto up = nodes->upgrade(c, s2);
            if (!*up) {
                m.stats.link_hits++;
                pd.cur = *nodes->resolve(c);
                continue;
            }
            m.stats.expansions++;
            Node<G>* leaf = nodes->get(c);
            leaf->visit();
            if (leaf->e != 0.0f) {
                nodes->unlock(c);
                pd.v = leaf->e;
                return pd;
            }
            pd.kind = 1;
            return pd;
        } else {
            pd.node_path.push_back(cur);
            pd.cur = *nodes->resolve(c);
            depth += 1;
        }
    }
}

// AsyncMcts::search_lockstep / search over the forced select phase
template <class G>
void f_search(AsyncMcts<G>& m, size_t root_idx, Forced& F) {
    auto& nodes = m.nodes;
    if (m.num_sims % m.num_threads != 0) throw std::runtime_error("num_sims % num_threads != 0");
    if (m.num_threads == 1 && !m.force_lockstep) {
        for (size_t i = 0; i < m.num_sims; ++i) f_search_iteration(m, root_idx, F);
        return;
    }
    const size_t steps = m.num_sims / m.num_threads;
    for (size_t step = 0; step < steps; ++step) {
        std::vector<typename AsyncMcts<G>::Pending> pend;
        pend.reserve(m.num_threads);
        for (size_t t = 0; t < m.num_threads; ++t) pend.push_back(f_select_phase(m, root_idx, F, t));
        for (auto& pd : pend) {
            if (pd.kind != 1) continue;
            Node<G>* leaf = nodes->get(pd.cur);
            auto pv = m.evaluate(*leaf->s, *leaf->v);
            nodes->set_policy(pd.cur, std::move(pv.first));
            nodes->unlock(pd.cur);
            pd.v = -pv.second;
        }
        for (auto& pd : pend) {
            if (pd.kind == 2) continue;
            float x = pd.v;
            nodes->get(pd.cur)->unvisit(x);
            while (!pd.node_path.empty()) {
                size_t cur = pd.node_path.back();
                pd.node_path.pop_back();
                if (!m.quirks.b2_same_sign_backup) x = -x;
                nodes->get(cur)->unvisit(x);
            }
        }
    }
}

// AsyncMcts::get_action_prob of a FORCED MOVE: root (+ noise when nz.eps > 0), the forced search, counts -> (pruned counts) -> pi.
// counts_out / q_out stay raw.
template <class G>
std::vector<float> forced_get_action_prob(AsyncMcts<G>& m, Forced& F, const Noise& nz, const G& s, float temp, uint64_t seed, uint64_t game_id,
                                          uint64_t ply, uint16_t* counts_out = nullptr, float* q_out = nullptr) {
    const size_t A = m.action_size;
    const size_t root = ensure_root(m, s);
    if (nz.eps > 0.0f) {
        Node<G>* rn = m.nodes->get(root);
        const uint32_t vm = valid_mask_of<G>(*rn->v);
        float eta[8];
        az::noise_eta(seed, game_id, ply, nz.alpha, vm, (int)A, eta);
        std::vector<float>& p = *rn->p;
        for (size_t a = 0; a < A; ++a)
            if ((vm >> a) & 1u) p[a] = az::noise_mix(nz.eps, p[a], eta[a]);
    }
    f_search(m, root, F);
    Node<G>* root_node = m.nodes->get(root);
    std::vector<uint16_t> counts(A, 0), pruned(A, 0);
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
    pruned = counts;
    if (F.prune && F.k > 0.0f) {
        size_t b = 0;
        for (size_t j = 0; j < nchild; ++j) if (n_j[j] >= n_j[b]) b = j;       // the most visited slot, the highest among equals
        const float sq = az::forced_sqrt_parent((uint32_t)root_node->get_n());
        const float u_star = az::forced_puct(q_j[b], n_j[b], p_j[b], sq, (float)m.cpuct);
        bool changed = false;
        for (size_t j = 0; j < nchild; ++j) {
            if (j == b || n_j[j] == 0) continue;
            const uint32_t mj = az::forced_prune(F.k, p_j[j], S, n_j[j], q_j[j], sq, (float)m.cpuct, u_star);
            pruned[a_j[j]] = (uint16_t)mj;
            if (mj != n_j[j]) changed = true;
            if (mj == 0 && n_j[j] >= 2 && az::forced_prune_loop(F.k, p_j[j], S, n_j[j], q_j[j], sq, (float)m.cpuct, u_star) == 1) F.c[FC_TO_ZERO]++;   // the single-playout rule
            F.c[FC_VISITS_PRUNED] += n_j[j] - mj;
        }
        if (changed) F.c[FC_MOVES_PRUNED]++;
    }
    F.c[FC_MOVES]++;
    F.c[FC_VISITS] += S;
    std::vector<float> probs(A, 0.0f);
    if (temp == 0.0f) {
        uint16_t max_val = 0;
        for (auto c : pruned) if (c > max_val) max_val = c;
        std::vector<size_t> best;
        for (size_t i = 0; i < A; ++i) if (pruned[i] == max_val) best.push_back(i);
        uint64_t r = rng_draw(seed, game_id, ply, RNG_TIEBREAK);
        probs[best[rng_choose(r, (uint32_t)best.size())]] = 1.0f;
        return probs;
    }
    float inv_t = 1.0f / temp;
    std::vector<float> x(A);
    for (size_t i = 0; i < A; ++i) x[i] = (inv_t == 1.0f) ? (float)pruned[i] : std::pow((float)pruned[i], inv_t);
    float sum = 0.0f;
    for (size_t i = 0; i < A; ++i) sum = sum + x[i];
    for (size_t i = 0; i < A; ++i) probs[i] = x[i] / sum;
    return probs;
}

// capped_episode of playout_cap_twin.cpp with the forced moves; n_fast == 0: no playout cap, every move is a full one
template <class G>
CapEpisode forced_episode(AsyncMcts<G>& mcts, Forced& F, const Noise& nz, size_t n_full, size_t n_fast, uint32_t thresh24, size_t temp_threshold,
                          uint64_t seed, uint64_t game_id) {
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
        const bool full = n_fast == 0 || az::playout_cap_full(seed, game_id, ply, thresh24);
        mcts.num_sims = full ? n_full : n_fast;
        out.budgets += mcts.num_sims;
        std::vector<float> pi = full ? forced_get_action_prob(mcts, F, nz, canonical, temp, seed, game_id, ply)
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

struct ForcedTreeBase {
    virtual ~ForcedTreeBase() = default;
    virtual int get_action_prob(uint64_t mine, uint64_t theirs, float temp, uint64_t seed, uint64_t game_id, int64_t eps_e6, int64_t alpha_e6,
                                int64_t k_e6, int prune, float* pi, uint16_t* counts, float* q, uint64_t* ctr) = 0;
    virtual Nets& nets() = 0;
};
template <class G>
struct ForcedTree : ForcedTreeBase {
    Nets n;
    std::unique_ptr<AsyncMcts<G>> m;
    int get_action_prob(uint64_t mine, uint64_t theirs, float temp, uint64_t seed, uint64_t game_id, int64_t eps_e6, int64_t alpha_e6, int64_t k_e6,
                        int prune, float* pi, uint16_t* counts, float* q, uint64_t* ctr) override {
        try {
            const G s{mine, theirs};
            Forced F(k_e6, prune);
            auto p = forced_get_action_prob(*m, F, Noise(eps_e6, alpha_e6), s, temp, seed, game_id, (uint64_t)__builtin_popcountll(mine | theirs), counts, q);
            for (size_t i = 0; i < p.size(); ++i) pi[i] = p[i];
            if (ctr) for (int i = 0; i < FC_COUNT; ++i) ctr[i] += F.c[i];
            return 0;
        } catch (const std::exception&) { return -1; }
    }
    Nets& nets() override { return n; }
};
template <class G>
ForcedTreeBase* make_forced_tree(uint64_t reserve, uint64_t sims, uint64_t threads, uint64_t max_depth, int cpuct, int net_kind, uint64_t salt) {
    auto* t = new ForcedTree<G>();
    t->n.hash.salt = salt;
    t->m.reset(new AsyncMcts<G>(reserve, sims, threads, max_depth, 0, cpuct, t->n.get(net_kind), C4_W));
    return t;
}

}  // namespace

extern "C" {

int twin_forced_counters() { return FC_COUNT; }

// the host build of csrc/az_forced.h, element by element: nf, the forced predicate and the pruned count of one slot
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

void* twin_forced_tree_new(int game_kind, uint64_t reserve, uint64_t sims, uint64_t threads, uint64_t max_depth, int cpuct, int net_kind, uint64_t salt) {
    try {
        if (game_kind == 2) return make_forced_tree<C3Bits>(reserve, sims, threads, max_depth, cpuct, net_kind, salt);
        return make_forced_tree<C4Bits>(reserve, sims, threads, max_depth, cpuct, net_kind, salt);
    } catch (const std::exception&) { return nullptr; }
}
void twin_forced_tree_free(void* t) { delete (ForcedTreeBase*)t; }
// ctr [FC_COUNT] is ACCUMULATED into
int twin_forced_tree_get_action_prob(void* t, uint64_t mine, uint64_t theirs, float temp, uint64_t seed, uint64_t game_id, int64_t eps_e6,
                                     int64_t alpha_e6, int64_t k_e6, int prune, float* pi, uint16_t* counts, float* q, uint64_t* ctr) {
    return ((ForcedTreeBase*)t)->get_action_prob(mine, theirs, temp, seed, game_id, eps_e6, alpha_e6, k_e6, prune, pi, counts, q, ctr);
}

// twin_capped_selfplay with forced playouts and pruning on the full moves (cap_sims == 0: no playout cap); ctr [FC_COUNT] is written
int64_t twin_forced_selfplay(int64_t n_games, uint64_t first_game_id, uint64_t sims, uint64_t cap_sims, int64_t full_e6, uint64_t temp_threshold, int cpuct,
                             uint64_t max_depth, uint64_t reserve, uint64_t seed, int net_kind, uint64_t salt, int game_kind, int sim_threads,
                             int64_t eps_e6, int64_t alpha_e6, int64_t k_e6, int prune, float* boards, float* pis, float* zs, int64_t cap,
                             int32_t* game_len, uint8_t* moves, uint64_t* full_masks, uint64_t* sims_out, uint64_t* ctr, const int64_t* rec_off,
                             const uint64_t* rec_states, const float* rec_pi, const float* rec_v, int32_t* replay_bad) {
    const Noise nz(eps_e6, alpha_e6);
    Forced F(k_e6, prune);
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
                ep = forced_episode<C3Bits>(m, F, nz, sims, cap_sims, th, temp_threshold, seed, first_game_id + (uint64_t)g);
            } else {
                AsyncMcts<C4Bits> m(reserve, sims, ST, max_depth, 0, cpuct, nets.get(net_kind), C4_W);
                ep = forced_episode<C4Bits>(m, F, nz, sims, cap_sims, th, temp_threshold, seed, first_game_id + (uint64_t)g);
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
    for (int i = 0; i < FC_COUNT; ++i) ctr[i] = F.c[i];
    return n;
}

}  // extern "C"
