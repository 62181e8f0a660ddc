// gumbel_twin.cpp -- the CPU twin of Gumbel root search with sequential halving ("gumbel_m" / "gumbel_c_visit_e6" / "gumbel_c_scale_e6",
// include/az_engine.h), alone and combined with Dirichlet root noise and playout cap randomization.  TEST INFRASTRUCTURE ONLY.
//
// The oracle (oracle/az_oracle.hpp) has none of it and keeps its behaviour.  A Gumbel move is restated AROUND it, through its public
// pieces: root_of (the root with its prior), the root_select seam, which replaces best_child for the first selection of a simulation, and
// search.  A GUMBEL move is: root_of, noise mixed into the root's prior when eps > 0, the baseline and the variates taken, search with
// az::gumbel_select at the root, then az::gumbel_result on the final counters: the improved policy is recorded and the selected action is
// played.  A fast move (playout cap) is the oracle's plain get_action_prob at the capped budget; it is only played.  The rule is the g++
// build of csrc/az_gumbel.h, the text the kernels compile.  Built by the tests with g++ -O2 -ffp-contract=off into a shared library driven
// through ctypes (tests/gumbel_twin.py).
#include "az_oracle_games.hpp"
#include "az_gumbel.h"
#include "az_noise.h"
#include "az_playout.h"

using namespace azo;

namespace {

// what the twin COUNTS: the parity tests assert on these so that they cannot pass vacuously
enum { GC_ROOT_SEL = 0, GC_ROOT_NOT_PUCT, GC_MOVES, GC_MOVES_NOT_MOST_VISITED, GC_MOVES_REUSED, GC_NO_CONSIDERED, GC_BAD_SCHEDULE, GC_MOVES_G_ZERO, GC_MOVES_RELINKED, GC_COUNT };

struct Rules {
    uint32_t m = 0;                      // gumbel_m
    float c_visit = 50.0f, c_scale = 1.0f;
    float eps = 0.0f, alpha = 1.0f;      // root noise
    size_t cap_sims = 0;                 // playout cap: the fast moves' budget; 0 = every move is a Gumbel move
    uint32_t thresh24 = 0;
    uint64_t c[GC_COUNT] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    Rules(int m_, int64_t cv_e6, int64_t cs_e6, int64_t eps_e6, int64_t alpha_e6, uint64_t cap_sims_, int64_t full_e6)
        : m((uint32_t)m_), c_visit(az::gumbel_of_e6(cv_e6)), c_scale(az::gumbel_of_e6(cs_e6)), eps((float)((double)eps_e6 / 1e6)),
          alpha((float)((double)alpha_e6 / 1e6)), cap_sims((size_t)cap_sims_), thresh24(az::playout_cap_thresh24((uint64_t)full_e6)) {}
};

template <class G>
uint32_t valid_mask_of(const std::vector<uint8_t>& v) {
    uint32_t m = 0;
    for (size_t a = 0; a < v.size(); ++a) if (v[a]) m |= 1u << a;
    return m;
}

// the d vector sequential halving prescribes for m_eff considered actions and n simulations, largest first: in the phase with k
// considered actions the k leading slots get one visit per round
std::vector<uint32_t> prescribed_d(uint32_t m_eff, uint32_t n, uint32_t nchild) {
    std::vector<uint32_t> d(nchild, 0u);
    if (m_eff <= 1u) { if (nchild) d[0] = n; return d; }
    uint32_t L = 0;
    while ((1u << L) < m_eff) ++L;
    uint32_t k = m_eff, left = n;
    while (left > 0) {
        const uint32_t extra = std::max<uint32_t>(1u, n / (L * k));
        const uint32_t take = std::min(left, extra * k);
        for (uint32_t j = 0; j < k; ++j) d[j] += take / k + (j < take % k ? 1u : 0u);
        left -= take;
        k = std::max<uint32_t>(2u, k / 2u);
    }
    return d;
}

// the root's slots as az_gumbel.h takes them, from the oracle's nodes.  d[j] = the simulations of this move the root's selection sent to slot j,
// counted by the twin itself; the baseline the header subtracts is then n_j - d_j.  (At the move's start that is the slot's resolved visit
// count; a placeholder slot that its first visit turns into a link to a node an earlier move built takes that node's earlier count.)
template <class G>
az::GumbelRoot root_view(const AsyncMcts<G>& m, size_t root, const uint32_t* d, const float* g) {
    const Node<G>* rn = m.nodes->get(root);
    az::GumbelRoot r{};
    r.nchild = (uint32_t)rn->children.size();
    for (uint32_t j = 0; j < r.nchild; ++j) {
        const size_t ci = rn->children[j];
        const Node<G>* child = m.nodes->get(ci);
        r.p[j] = (*rn->p)[m.nodes->raw(ci)->a];
        r.q[j] = child->compute_q();
        r.n[j] = child->get_n();
        r.base[j] = (r.n[j] - d[j]) & 0xFFFFu;
        r.g[j] = g[j];
    }
    return r;
}

// AsyncMcts::get_action_prob as a Gumbel move (gumbel = false: the oracle's own).  counts_out / q_out stay raw; *selected = the action played;
// d_out [7] (may be null) = the slots' visits in this call
template <class G>
std::vector<float> twin_get_action_prob(AsyncMcts<G>& m, Rules& R, bool gumbel, const G& s, float temp, uint64_t seed, uint64_t game_id, uint64_t ply,
                                        int* selected, uint16_t* counts_out = nullptr, float* q_out = nullptr, uint32_t* d_out = nullptr) {
    *selected = -1;
    if (!gumbel) return m.get_action_prob(s, temp, seed, game_id, ply, counts_out, q_out);
    const size_t A = m.action_size;
    const size_t root = m.root_of(s);
    Node<G>* rn = m.nodes->get(root);
    if (R.eps > 0.0f) {      // root noise, as tests/cpp/selfplay_twin.cpp mixes it
        const uint32_t vm = valid_mask_of<G>(*rn->v);
        float eta[8];
        az::noise_eta(seed, game_id, ply, R.alpha, vm, (int)A, eta);
        std::vector<float>& p = *rn->p;
        for (size_t a = 0; a < A; ++a)
            if ((vm >> a) & 1u) p[a] = az::noise_mix(R.eps, p[a], eta[a]);
    }
    const uint32_t nchild = (uint32_t)rn->children.size();
    uint32_t base[az::GUMBEL_SLOTS] = {0, 0, 0, 0, 0, 0, 0}, dm[az::GUMBEL_SLOTS] = {0, 0, 0, 0, 0, 0, 0};
    float g[az::GUMBEL_SLOTS] = {0, 0, 0, 0, 0, 0, 0};
    uint8_t a_j[az::GUMBEL_SLOTS] = {0, 0, 0, 0, 0, 0, 0};
    bool reused = false;
    for (uint32_t j = 0; j < nchild; ++j) {
        const size_t ci = rn->children[j];
        a_j[j] = m.nodes->raw(ci)->a;
        base[j] = m.nodes->get(ci)->get_n();
        g[j] = az::gumbel_variate(seed, game_id, ply, a_j[j], temp == 0.0f);
        reused = reused || base[j] != 0;
    }
    const uint32_t budget = (uint32_t)m.num_sims;
    {
        struct Unhook { AsyncMcts<G>& m; ~Unhook() { m.root_select = nullptr; } } unhook{m};
        m.root_select = [&](size_t idx, bool, size_t) {
            const az::GumbelRoot r = root_view(m, idx, dm, g);
            bool found = false;
            const uint32_t j = az::gumbel_select(r, R.m, budget, R.c_visit, R.c_scale, &found);
            dm[j] += 1;
            const size_t c = m.nodes->get(idx)->children[j];
            R.c[GC_ROOT_SEL]++;
            if (!found) R.c[GC_NO_CONSIDERED]++;
            if (c != m.nodes->best_child(idx, m.cpuct, false)) R.c[GC_ROOT_NOT_PUCT]++;
            return c;
        };
        m.search(root);
    }
    const az::GumbelRoot r = root_view(m, root, dm, g);
    float pi_slot[az::GUMBEL_SLOTS];
    const uint32_t sel = az::gumbel_result(r, R.c_visit, R.c_scale, pi_slot);
    std::vector<float> pi(A, 0.0f);
    uint32_t max_n = 0;
    std::vector<uint32_t> d(nchild);
    for (uint32_t j = 0; j < nchild; ++j) {
        pi[a_j[j]] = pi_slot[j];
        if (counts_out) counts_out[a_j[j]] = (uint16_t)r.n[j];
        if (q_out) q_out[a_j[j]] = r.q[j];
        max_n = std::max(max_n, r.n[j]);
        d[j] = az::gumbel_d(r, j);
        if (d_out) d_out[j] = d[j];
    }
    *selected = a_j[sel];
    // the schedule: the selected slot has the most visits of this call, and the sorted d vector is the prescribed one
    const uint32_t d_sel = d[sel];
    std::sort(d.begin(), d.end(), std::greater<uint32_t>());
    if (d != prescribed_d(std::min(R.m, nchild), budget, nchild) || d_sel != d[0]) R.c[GC_BAD_SCHEDULE]++;
    R.c[GC_MOVES]++;
    if (r.n[sel] != max_n) R.c[GC_MOVES_NOT_MOST_VISITED]++;
    if (reused) R.c[GC_MOVES_REUSED]++;
    if (temp == 0.0f) R.c[GC_MOVES_G_ZERO]++;
    bool relinked = false;       // a placeholder slot became a link to an older node: its baseline is that node's earlier count, not the 0 taken at the start
    for (uint32_t j = 0; j < nchild; ++j) relinked = relinked || r.base[j] != base[j];
    if (relinked) R.c[GC_MOVES_RELINKED]++;
    return pi;
}

struct Episode {
    std::vector<TrainingSample> samples;
    std::vector<uint8_t> moves;
    uint64_t full_mask = 0, sims = 0, budgets = 0;
};

// Coach::execute_episode (src/coach.rs:104-157) as oracle/az_oracle_games.hpp restates it, with Gumbel moves: n_full = num_sims,
// n_fast = playout_cap_sims; full moves are Gumbel moves and recorded, fast moves are the oracle's and only played
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
        int selected = -1;
        std::vector<float> pi = twin_get_action_prob(mcts, R, full, canonical, temp, seed, game_id, ply, &selected);
        if (full) {
            out.full_mask |= 1ull << ply;
            for (auto& bp : canonical.get_symmetries(pi)) train_examples.push_back({bp.first.to_features(), cur_player, bp.second});
        }
        uint8_t action;
        if (full) {
            action = (uint8_t)selected;              // the move draw is not used
        } else {
            const uint64_t r64 = rng_draw(seed, game_id, ply, RNG_MOVE);
            action = (uint8_t)rng_choose_weighted(r64, pi.data(), (int)pi.size());
        }
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
Episode play_episode(Nets& nets, Rules& R, uint64_t reserve, uint64_t sims, uint64_t max_depth, int cpuct, int net_kind, uint64_t temp_threshold,
                     uint64_t seed, uint64_t game_id) {
    AsyncMcts<G> m(reserve, sims, 1, max_depth, 0, cpuct, nets.get(net_kind), C4_W);
    return twin_episode<G>(m, R, sims, temp_threshold, seed, game_id);
}

struct TreeBase {
    Nets n;
    virtual ~TreeBase() = default;
    virtual int get_action_prob(uint64_t mine, uint64_t theirs, float temp, uint64_t seed, uint64_t game_id, Rules& R, float* pi, uint16_t* counts,
                                float* q, int* selected, uint32_t* d) = 0;
};
template <class G>
struct Tree : TreeBase {
    std::unique_ptr<AsyncMcts<G>> m;
    int get_action_prob(uint64_t mine, uint64_t theirs, float temp, uint64_t seed, uint64_t game_id, Rules& R, float* pi, uint16_t* counts,
                        float* q, int* selected, uint32_t* d) override {
        try {
            auto p = twin_get_action_prob(*m, R, R.m != 0, G{mine, theirs}, temp, seed, game_id, (uint64_t)__builtin_popcountll(mine | theirs), selected,
                                          counts, q, d);
            for (size_t i = 0; i < p.size(); ++i) pi[i] = p[i];
            return 0;
        } catch (const std::exception&) { return -1; }
    }
};
template <class G>
TreeBase* make_tree(uint64_t reserve, uint64_t sims, uint64_t max_depth, uint64_t model_id, int cpuct, int net_kind, uint64_t salt) {
    auto* t = new Tree<G>();
    t->n.hash.salt = salt;
    t->m.reset(new AsyncMcts<G>(reserve, sims, 1, max_depth, model_id, cpuct, t->n.get(net_kind), C4_W));
    return t;
}

}  // namespace

extern "C" {

int gtwin_counters() { return GC_COUNT; }

// ---- the host build of csrc/az_gumbel.h, element by element ---------------------------------------------------------------------------------
void gtwin_considered(uint32_t m_eff, uint32_t n, int64_t count, uint32_t* out) { for (int64_t t = 0; t < count; ++t) out[t] = az::gumbel_considered_visit(m_eff, n, (uint32_t)t); }
void gtwin_prescribed_d(uint32_t m_eff, uint32_t n, uint32_t nchild, uint32_t* out) {
    const std::vector<uint32_t> d = prescribed_d(m_eff, n, nchild);
    for (uint32_t j = 0; j < nchild; ++j) out[j] = d[j];
}
void gtwin_uniform(int64_t n, const uint64_t* r, float* out) { for (int64_t i = 0; i < n; ++i) out[i] = az::gumbel_uniform(r[i]); }
void gtwin_of_uniform(int64_t n, const float* u, float* out) { for (int64_t i = 0; i < n; ++i) out[i] = az::gumbel_of_uniform(u[i]); }
void gtwin_logit(int64_t n, const float* p, float* out) { for (int64_t i = 0; i < n; ++i) out[i] = az::gumbel_logit(p[i]); }
// g_out [n,7] for root states [n,2] on the streams (seed, game_ids[i], stones): what az_gumbel_values returns from the device
void gtwin_values(int64_t n, uint64_t seed, const uint64_t* game_ids, const uint64_t* states, int temp_is_zero, float* g_out) {
    for (int64_t i = 0; i < n; ++i) {
        const C4Bits s{states[2 * i], states[2 * i + 1]};
        const uint32_t vm = valid_mask_of<C4Bits>(s.get_valid_moves(1));
        const uint64_t ply = (uint64_t)__builtin_popcountll(s.p1 | s.m1);
        for (int a = 0; a < C4_W; ++a) g_out[7 * i + a] = ((vm >> a) & 1u) ? az::gumbel_variate(seed, game_ids[i], ply, (uint32_t)a, temp_is_zero != 0) : 0.0f;
    }
}
// one root: the slot a simulation goes to (sel_out[0], found in sel_out[1]), the move's result on the same counters (sel_out[2]), sigma and pi by slot
void gtwin_root(uint32_t nchild, const float* p, const float* q, const float* g, const uint32_t* n, const uint32_t* base, uint32_t m, uint32_t budget,
                int64_t cv_e6, int64_t cs_e6, uint32_t* sel_out, float* sigma_out, float* pi_out) {
    az::GumbelRoot r{};
    r.nchild = nchild;
    for (uint32_t j = 0; j < nchild; ++j) { r.p[j] = p[j]; r.q[j] = q[j]; r.g[j] = g[j]; r.n[j] = n[j]; r.base[j] = base[j]; }
    const float cv = az::gumbel_of_e6(cv_e6), cs = az::gumbel_of_e6(cs_e6);
    bool found = false;
    sel_out[0] = az::gumbel_select(r, m, budget, cv, cs, &found);
    sel_out[1] = found ? 1u : 0u;
    az::gumbel_sigmas(r, cv, cs, sigma_out);
    sel_out[2] = az::gumbel_result(r, cv, cs, pi_out);
}

// ---- one AsyncMcts whose get_action_prob is a Gumbel move (m > 0) -----------------------------------------------------------------------------
// game_kind 0 = Connect Four, 2 = Connect Three; net_kind 0 stub, 1 hash, 2 replay
void* gtwin_tree_new(int game_kind, uint64_t reserve, uint64_t sims, uint64_t max_depth, uint64_t model_id, int cpuct, int net_kind, uint64_t salt) {
    try {
        if (game_kind == 2) return make_tree<C3Bits>(reserve, sims, max_depth, model_id, cpuct, net_kind, salt);
        return make_tree<C4Bits>(reserve, sims, max_depth, model_id, cpuct, net_kind, salt);
    } catch (const std::exception&) { return nullptr; }
}
void gtwin_tree_free(void* t) { delete (TreeBase*)t; }
// ctr [GC_COUNT] is ACCUMULATED into
int gtwin_tree_get_action_prob(void* t, uint64_t mine, uint64_t theirs, float temp, uint64_t seed, uint64_t game_id, int m, int64_t cv_e6, int64_t cs_e6,
                               int64_t eps_e6, int64_t alpha_e6, float* pi, uint16_t* counts, float* q, int32_t* selected, uint32_t* d, uint64_t* ctr) {
    Rules R(m, cv_e6, cs_e6, eps_e6, alpha_e6, 0, 0);
    int sel = -1;
    const int rc = ((TreeBase*)t)->get_action_prob(mine, theirs, temp, seed, game_id, R, pi, counts, q, &sel, d);
    *selected = sel;
    if (rc == 0) for (int i = 0; i < GC_COUNT; ++i) ctr[i] += R.c[i];
    return rc;
}

// ---- Coach::execute_episode x n_games with Gumbel moves: the outputs of oracle_py.selfplay (azo_selfplay) plus the full-ply masks [n_games],
// sims_out[2] = {the oracle's simulation counter, the sum of the budgets}, both summed over the episodes, and ctr [GC_COUNT] ---------------------
int64_t gtwin_selfplay(int64_t n_games, uint64_t first_game_id, uint64_t sims, uint64_t cap_sims, int64_t full_e6, uint64_t temp_threshold, int cpuct,
                       uint64_t max_depth, uint64_t reserve, uint64_t seed, int net_kind, uint64_t salt, int game_kind, int m, int64_t cv_e6, int64_t cs_e6,
                       int64_t eps_e6, int64_t alpha_e6, float* boards, float* pis, float* zs, int64_t cap, int32_t* game_len, uint8_t* moves,
                       uint64_t* full_masks, uint64_t* sims_out, uint64_t* ctr, const int64_t* rec_off, const uint64_t* rec_states, const float* rec_pi,
                       const float* rec_v, int32_t* replay_bad) {
    Rules R(m, cv_e6, cs_e6, eps_e6, alpha_e6, cap_sims, full_e6);
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
            const Episode ep = game_kind == 2 ? play_episode<C3Bits>(nets, R, reserve, sims, max_depth, cpuct, net_kind, temp_threshold, seed, game_id)
                                              : play_episode<C4Bits>(nets, R, reserve, sims, max_depth, cpuct, net_kind, temp_threshold, seed, game_id);
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
    for (int i = 0; i < GC_COUNT; ++i) ctr[i] = R.c[i];
    return n;
}

}  // extern "C"
