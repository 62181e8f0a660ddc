// az_tree.hip -- MCTS tree kernels for gfx950 (select / expand / leaf request / backup / root policy / self-play move),
// templates over the Game policy of az_game.h.  GROUP (8) lanes serve one game: lane j evaluates child j of the node
// being selected, so a node's child block (8 x 32-byte records, 256-byte aligned) is two coalesced 128-byte lines and
// the PUCT arg-max is an in-register fold over lane shuffles.  One simulation is in flight per tree (the reference's
// deterministic mode, num_sim_threads = 1), so every counter update is a plain read-modify-write by one lane:
// integer, order-free, bit-reproducible.
//
// Reference restated: src/async_mcts.rs:74-115, :219-371; src/node.rs:272-370;
// src/coach.rs:104-157; with the repairs of SURVEY.md section 0.2 (tagged S#/B#).
#include "az_tree.h"
#include "az_noise.h"
#include "az_gumbel.h"
#include "az_target.h"

namespace az {
static_assert(NOISE_PURPOSE == RNG_NOISE, "az_noise.h restates the purpose word of az_common.h");
static_assert(GUMBEL_PURPOSE == RNG_GUMBEL, "az_gumbel.h restates the purpose word of az_common.h");
// THE ROOT RULE of a search: one template axis with three values (forced playouts and Gumbel exclude each other, az_engine.hip), so the
// kernels that carry it exist three times, not four
enum RootRule : int { RR_NONE = 0, RR_FORCED = 1, RR_GUMBEL = 2 };
// THE COUNTDOWN of a move in TreeHead.active, the PC axis of k_backup_select and k_search_fixture: none / the playout cap's budget / a budget
// plus the decided-move stop (az_stop.h).  The kernels that only carry the cap (k_step_mt, k_async_step, k_selfplay_move) keep a bool.
enum Countdown : int { PC_NONE = 0, PC_BUDGET = 1, PC_STOP = 2 };

// ---- lane-group primitives (GW = Game::GROUP lanes per tree) ------------------------------------------------------
template <int GW> AZ_D uint32_t gshfl(uint32_t v, int src) { return (uint32_t)__shfl((int)v, src, GW); }
template <int GW> AZ_D float gshflf(float v, int src) { return __shfl(v, src, GW); }
template <int GW> AZ_D uint64_t gshfl64(uint64_t v, int src) {
    return ((uint64_t)gshfl<GW>((uint32_t)(v >> 32), src) << 32) | gshfl<GW>((uint32_t)v, src);
}
template <int GW> AZ_D uint32_t gballot(bool p) {
    unsigned long long m = __ballot(p);
    int lane = threadIdx.x & 63;
    return (uint32_t)(m >> (lane & ~(GW - 1))) & ((1u << GW) - 1u);
}
template <int NA> AZ_D uint32_t nth_set_bit(uint32_t mask, uint32_t n) {
    uint32_t a = 0;
#pragma unroll
    for (int c = 0; c < NA; ++c) {
        bool set = (mask >> c) & 1u;
        if (set && n == 0) a = (uint32_t)c;
        if (set) --n;
    }
    return a;
}

// ---- node record access (layout: az_tree.h) ---------------------------------------------------------------------------
// The 16-byte record {ctr, prior, word}: word = a | nchild << 3 | ecode << 6 | has_prior << 8 | locked << 9 | kind << 10 | payload << 12,
// kind 0 = placeholder, 1 = link (payload = the canonical node's slot), 2 = expanded (payload = child block index).  NodeRec keeps the
// meta bits of az_common.h (EXPANDED = kind 2) so the search code reads as before; the packed state of an expanded node lives in t.key.
struct NodeRec {
    uint64_t ctr;
    uint32_t prior, meta, link, child_base;
};
AZ_HD uint32_t node_word(uint32_t meta, uint32_t link, uint32_t child_base) {
    const uint32_t kind = link != NONE ? 1u : ((meta & META_EXPANDED) ? 2u : 0u);
    const uint32_t payload = kind == 1u ? link : (kind == 2u ? child_base / (uint32_t)BLOCK_SLOTS : 0u);
    return (meta & 0x3Fu) | (((meta >> META_ECODE_SHIFT) & 0xFu) << 6) | (kind << 10) | (payload << 12);
}
AZ_D uint4* node_ptr(const TreeDev& t, size_t base, uint32_t slot) { return t.node + (base + slot); }
AZ_D NodeRec node_load(const uint4* p) {
    const uint4 a = p[0];
    const uint32_t w = a.w, kind = (w >> 10) & 3u, payload = w >> 12;
    NodeRec r;
    r.ctr = ((uint64_t)a.y << 32) | a.x;
    r.prior = a.z;
    r.meta = (w & 0x3Fu) | (((w >> 6) & 0xFu) << META_ECODE_SHIFT) | (kind == 2u ? META_EXPANDED : 0u);
    r.link = kind == 1u ? payload : NONE;
    r.child_base = kind == 2u ? payload * (uint32_t)BLOCK_SLOTS : 0u;
    return r;
}
AZ_D void node_store(const TreeDev& t, size_t base, uint32_t slot, uint64_t ctr, uint64_t key, uint32_t prior, uint32_t meta, uint32_t link,
                     uint32_t child_base) {
    t.node[base + slot] = make_uint4((uint32_t)ctr, (uint32_t)(ctr >> 32), prior, node_word(meta, link, child_base));
    if (meta & META_EXPANDED) t.key[base + slot] = key;           // only expanded nodes have a state (and only they are looked up by it)
}
AZ_D uint64_t node_ctr(const uint4* p) { return *(const unsigned long long*)p; }
AZ_D void node_set_ctr(uint4* p, uint64_t v) { *(unsigned long long*)p = v; }
AZ_D uint64_t node_key(const TreeDev& t, size_t base, uint32_t slot) { return t.key[base + slot]; }
AZ_D void node_set_prior(uint4* p, uint32_t bits) { ((uint32_t*)p)[2] = bits; }
// rewrite the word of a record whose fields the caller holds (meta changes, or a placeholder becoming a link)
AZ_D void node_set_word(uint4* p, uint32_t meta, uint32_t link, uint32_t child_base) { ((uint32_t*)p)[3] = node_word(meta, link, child_base); }

// `seen.get(&s)` (src/node.rs:282): GW-wide linear probe.  found = node slot or NONE;
// ins = first empty position (where `seen.insert` will go, src/node.rs:320).
template <class G>
AZ_D void hash_find(const TreeDev& t, int g, size_t base, typename G::State s, int sub, uint32_t* found, uint32_t* ins) {
    constexpr int GW = G::GROUP;
    const uint32_t mask = t.H - 1;
    const uint32_t h = G::hash(s) & mask;
    const uint64_t key = G::pack(s);
    const uint32_t* tab = t.hash + (size_t)g * t.H;
    for (uint32_t probe = 0; probe < t.H; probe += GW) {
        uint32_t pos = (h + probe + (uint32_t)sub) & mask;
        uint32_t idx = tab[pos];
        bool empty = idx == NONE;
        bool match = false;
        if (!empty) match = node_key(t, base, idx) == key;
        uint32_t em = gballot<GW>(empty), mm = gballot<GW>(match);
        int fe = em ? (__ffs((int)em) - 1) : GW;
        uint32_t before = mm & ((1u << fe) - 1u);
        if (before) {
            *found = gshfl<GW>(idx, __ffs((int)before) - 1);
            *ins = NONE;
            return;
        }
        if (em) {
            *found = NONE;
            *ins = (h + probe + (uint32_t)fe) & mask;
            return;
        }
    }
    *found = NONE;
    *ins = NONE;
}

// NodeStore::upgrade, `None` arm (src/node.rs:290-323): store s, e = -ended(s), push one placeholder per valid move in
// ascending action order into a fresh child block, insert into `seen`.  extra = nodes pushed besides the placeholders
// (1 when the upgraded node itself is new: a root).  Returns false when the arena is exhausted (assert!, src/node.rs:237).
template <class G>
AZ_D bool node_upgrade(const TreeDev& t, TreeHead& h, int g, size_t base, uint32_t slot, typename G::State s, uint32_t prior_bits,
                       uint32_t a, uint32_t ins_pos, uint64_t ctr_value, uint32_t cbase, uint32_t extra, int sub, uint32_t* ecode_out,
                       uint32_t lock_if_live = 0u /*META_LOCKED: the slot stays Locked until its prior is stored (src/node.rs:322, src/async_mcts.rs:351)*/) {
    uint32_t ec = G::ended_code(s);
    uint32_t vm = ec ? 0u : G::valid_mask(s);
    uint32_t nv = (uint32_t)__popc(vm);
    if (cbase + BLOCK_SLOTS > t.R || h.count + extra + nv > t.reserve_nodes || ins_pos == NONE) {
        if (sub == 0) atomicOr(&t.err[ins_pos == NONE ? ERR_HASH_FULL : ERR_CAPACITY], 1u);
        return false;
    }
    h.len = cbase + BLOCK_SLOTS;
    h.count += extra + nv;
    if (sub == 0) {
        node_store(t, base, slot, ctr_value, G::pack(s), prior_bits,
                   a | (nv << META_NCHILD_SHIFT) | META_EXPANDED | (ec << META_ECODE_SHIFT) | (ec == E_NONE ? lock_if_live : 0u), NONE, cbase);
        t.hash[(size_t)g * t.H + ins_pos] = slot;
    }
    if ((uint32_t)sub < nv)
        node_store(t, base, cbase + sub, CTR_INIT, 0ull, 0u, nth_set_bit<G::ACTIONS>(vm, (uint32_t)sub), NONE, 0u);
    *ecode_out = ec;
    return true;
}

// lane `sub`'s two inline node_path entries (j = sub and sub + 8)
struct PathRegs { uint32_t lo, hi; };
AZ_D PathRegs path_load(const TreeDev& t, int g, int sub) { return PathRegs{t.head[g].path16[sub], t.head[g].path16[8 + sub]}; }
AZ_D void path_store(const TreeDev& t, int g, int sub, const PathRegs& p) { t.head[g].path16[sub] = p.lo; t.head[g].path16[8 + sub] = p.hi; }

AZ_D TreeHead head_load(const TreeDev& t, int g) {
    const uint4* p = (const uint4*)(t.head + g);
    const uint4 a = p[0], b = p[1], c = p[2], d = p[3];
    TreeHead h;
    h.len = a.x; h.count = a.y; h.root = a.z; h.active = a.w;
    h.leaf = b.x; h.leaf_kind = b.y; h.leaf_val = __uint_as_float(b.z); h.src = b.w;
    h.path_len = c.x; h.log_len = c.y; h.stat[0] = c.z; h.stat[1] = c.w;
    h.stat[2] = d.x; h.stat[3] = d.y; h.stat[4] = d.z; h.stat[5] = d.w;
    return h;
}
AZ_D void head_store(const TreeDev& t, int g, const TreeHead& h) {
    uint4* p = (uint4*)(t.head + g);
    p[0] = make_uint4(h.len, h.count, h.root, h.active);
    p[1] = make_uint4(h.leaf, h.leaf_kind, __float_as_uint(h.leaf_val), h.src);
    p[2] = make_uint4(h.path_len, h.log_len, h.stat[0], h.stat[1]);
    p[3] = make_uint4(h.stat[2], h.stat[3], h.stat[4], h.stat[5]);
}

__global__ void k_init_heads(TreeDev t) {
    int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= t.G) return;
    TreeHead h{};
    h.active = 1;
    head_store(t, g, h);
}
__global__ void k_set_active(TreeDev t, uint32_t value) {
    int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g < t.G) t.head[g].head.active = value;
}

// ---- NodeStore::new (src/node.rs:156-166): clear `seen`, push + upgrade the initial board ----
template <class G>
__global__ __launch_bounds__(256) void k_reset_trees(TreeDev t, const uint8_t* flags, uint8_t* clear_flags,
                                                     const ulonglong2* roots /*nullptr = initial board*/) {
    constexpr int GW = G::GROUP;
    int g = blockIdx.x;
    if (flags && !flags[g]) return;
    uint32_t* tab = t.hash + (size_t)g * t.H;
    for (uint32_t i = threadIdx.x; i < t.H; i += blockDim.x) tab[i] = NONE;
    __syncthreads();
    if (threadIdx.x < GW) {
        int sub = threadIdx.x;
        size_t base = (size_t)g * t.R;
        TreeHead h = head_load(t, g);
        h.len = 0;
        h.count = 0;
        uint32_t ec;
        const typename G::State rs = roots ? roots[g] : G::init();          // NodeStore::from_root, src/node.rs:168-177
        uint32_t ins = G::hash(rs) & (t.H - 1);
        // the root takes slot 0 of block 0, its children block 1
        node_upgrade<G>(t, h, g, base, 0u, rs, 0u, 0u, ins, CTR_INIT, BLOCK_SLOTS, 1u, sub, &ec);
        h.root = 0;
        h.log_len = 0;
        h.leaf_kind = LEAF_NONE;
        if (sub == 0) {
            head_store(t, g, h);
            if (clear_flags) clear_flags[g] = 0;
        }
    }
}

// ---- leaf request: inference batch assembly (src/async_mcts.rs:137-151 restated) + de-duplication ---------------------
// A tree whose leaf goes to the net (want) gets a SOURCE for its (pi, v):
//   1. the evaluation cache: the state's bucket is one 64-byte line of 8 keys, lane j checks way j;
//   2. the batch's election table: the first tree to CAS its key in wins a row, later ones point at the winner's slot;
//   3. a row of the batch: one atomicAdd per wave (8 trees), rows in lane order inside the wave.
// Without de-duplication every requesting tree goes straight to 3.  All lanes of the wave that are still alive call
// this together (the ballots are wave-wide); lanes of trees with nothing to evaluate pass want = false.
// MIR ("eval_mirror", EvalBatch.mirror): everything here -- the cache probe, the election and the row -- is about c(s), the canonical
// orientation; the backup recomputes whether its tree's own s was the mirrored one.  Only the MIR instantiations contain any of it.
template <class G, bool MIR = false>
AZ_D uint32_t leaf_request(const EvalBatch& eb, const EvalCache& ec, bool want, typename G::State s, int sub) {
    constexpr int GW = G::GROUP;
    const int lane = (int)(threadIdx.x & 63);
    if constexpr (MIR) { uint32_t m; s = G::canonical(s, &m); }
    uint32_t src = 0;
    bool hit = false, dup = false, take = want;
    uint32_t tpos = 0;
    if (eb.dedup) {
        const unsigned long long key = (unsigned long long)G::pack(s);
        // the election table's first probe is fetched together with the cache's key line (one round trip, not two)
        const uint32_t pos0 = (uint32_t)(mix64(key) >> 24) & eb.tmask;
        unsigned long long cur0 = 0ull;
        if (want && sub == 0) cur0 = eb.tkey[pos0];
        if (ec.key) {
            const unsigned long long ck = key | ec.tag;
            const uint32_t bucket = (uint32_t)(mix64(ck) >> 20) & ec.bmask;
            const uint32_t ways = gballot<GW>(want && ec.key[(size_t)bucket * 8 + sub] == ck);
            if (want && ways) { hit = true; take = false; src = SRC_CACHE | (bucket * 8u + (uint32_t)__ffs((int)ways) - 1u); }
        }
        if (take && sub == 0) {
            const unsigned long long mine = key;                           // never 0 (Game::pack)
            uint32_t pos = pos0;
            unsigned long long cur = cur0;
            for (;; cur = eb.tkey[pos]) {
                if (cur == 0ull) {                                         // empty: try to take it
                    const unsigned long long prev = atomicCAS(&eb.tkey[pos], 0ull, mine);
                    if (prev == 0ull) break;                               // won the slot
                    cur = prev;                                            // somebody else took it first
                }
                if (cur == mine) { dup = true; break; }
                pos = (pos + 1u) & eb.tmask;
            }
            tpos = pos;
        }
        dup = gshfl<GW>(dup ? 1u : 0u, 0) != 0u;
        tpos = gshfl<GW>(tpos, 0);
        if (take && dup) { take = false; src = SRC_TABLE | tpos; }
    }
    // rows of the batch: one atomicAdd per wave
    const unsigned long long wm = __ballot(take && sub == 0);
    uint32_t base = 0;
    if (blockDim.x > 64) {
        // four waves per workgroup (k_backup_select): ONE atomicAdd on the batch's row counter per workgroup -- the counter is a single
        // hot address for the ~1000 waves of a launch.  Every wave of the workgroup gets here exactly once.
        __shared__ uint32_t s_cnt[4], s_base;
        const int w = (int)(threadIdx.x >> 6);
        if (lane == 0) s_cnt[w] = (uint32_t)__popcll(wm);
        __syncthreads();
        if (threadIdx.x == 0) {
            const uint32_t total = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
            s_base = total ? atomicAdd(eb.n, total) : 0u;
        }
        __syncthreads();
        base = s_base;
        for (int i = 0; i < w; ++i) base += s_cnt[i];
    } else if (wm) {
        const int leader = __ffsll((long long)wm) - 1;
        if (lane == leader) base = atomicAdd(eb.n, (uint32_t)__popcll(wm));
        base = (uint32_t)__shfl((int)base, leader, 64);
    }
    if (wm) {
        if (take) {
            const int lane0 = lane & ~(GW - 1);
            const uint32_t row = base + (uint32_t)__popcll(wm & ((1ull << lane0) - 1ull));
            if (sub == 0) {
                eb.state[row] = s;
                if (eb.dedup) eb.tuniq[tpos] = row;
            }
            src = row;
        }
    }
    if (ec.stat && eb.dedup) {
        const unsigned long long am = __ballot(want && sub == 0), hm = __ballot(hit && sub == 0), dm = __ballot(dup && want && sub == 0);
        if (am && lane == __ffsll((long long)am) - 1) {
            unsigned long long* st = ec.stat + (size_t)(blockIdx.x % DD_REPLICAS) * DD_STRIDE;
            atomicAdd(&st[DD_REQUESTED], (unsigned long long)__popcll(am));
            if (wm) atomicAdd(&st[DD_EXECUTED], (unsigned long long)__popcll(wm));
            if (hm) atomicAdd(&st[DD_CACHE_HITS], (unsigned long long)__popcll(hm));
            if (dm) atomicAdd(&st[DD_BATCH_DUPS], (unsigned long long)__popcll(dm));
        }
    }
    return src;
}

// ---- Dirichlet root noise (az_noise.h; only the NZ instantiations of the kernels contain it) ---------------------------------------
// The root's 8 lanes together: lane sub < nchild draws the Gamma variate of its own child's action `myact` (an action's draws are a
// sub-stream of their own, so the lanes' rejection counts do not matter), the sum runs over the children in slot order = ascending
// action order (group shuffles), and the lane gets its child's eta.
template <class G>
AZ_D float root_noise_eta_lane(uint64_t stream, float alpha, uint32_t nchild, uint32_t myact, int sub) {
    constexpr int GW = G::GROUP;
    const float gm = (uint32_t)sub < nchild ? noise_gamma(stream, myact, alpha) : 0.0f;
    float sum = 0.0f;
#pragma unroll
    for (int j = 0; j < G::ACTIONS; ++j) {
        const float gj = gshflf<GW>(gm, j);
        if ((uint32_t)j < nchild) sum = __fadd_rn(sum, gj);
    }
    return noise_normalise(gm, sum, nchild);
}
// (seed, game_id) of tree g's root-move stream (az_tree.h RootStream): what the root noise and the Gumbel variates of its move are drawn on
AZ_D ulonglong2 root_stream_of(const TreeDev& t, int g) {
    const RootStream& r = t.move.stream;
    uint64_t seed = r.seed, game_id;
    if (r.stream) { const ulonglong2 st = r.stream[g]; seed = st.x; game_id = st.y; }
    else game_id = r.first_game_id + (uint64_t)(r.row ? r.row[g] : g);
    return make_ulonglong2(seed, game_id);
}
// the prior of lane sub's root child after the mix: (1 - eps) * prior + eps * eta[myact]; s = the root's state
template <class G>
AZ_D float root_noise_mix(const TreeDev& t, int g, typename G::State s, uint32_t nchild, uint32_t myact, float prior, int sub) {
    const ulonglong2 rs = root_stream_of(t, g);
    const uint64_t stream = noise_stream(rs.x, rs.y, (uint64_t)G::stones(s));
    return noise_mix(t.move.noise.eps, prior, root_noise_eta_lane<G>(stream, t.move.noise.alpha, nchild, myact, sub));
}

// Playout cap (az_tree.h PlayoutCap): a slot's fast moves get no noise, no forced playouts and no Gumbel rule; without a cap every move
// does.  Only NZ / RR != RR_NONE code reads this.
AZ_D bool move_noisy(const TreeDev& t, int g) { return !t.move.cap.word || (t.move.cap.word[g] & PLAYOUT_FULL_BIT) != 0u; }

// ---- Gumbel root search (az_gumbel.h; only the RR_GUMBEL / GZ instantiations of the kernels contain it) ------------------------------------
// A GUMBEL MOVE is every move that can carry root noise (move_noisy).  Its BASELINE is taken where the noise is mixed in -- once per move,
// after the root has its prior and before the first selection: lane sub < nchild stores the resolved visit count of its root child and the
// child's Gumbel variate (16 + 32 bytes per tree).  s = the root's state, cb = its child block.
template <class G>
AZ_D void gumbel_capture(const TreeDev& t, int g, size_t base, typename G::State s, uint32_t nchild, uint32_t cb, int sub) {
    uint32_t n = 0u;
    float gv = 0.0f;
    if ((uint32_t)sub < nchild) {
        const NodeRec cr = node_load(node_ptr(t, base, cb + (uint32_t)sub));
        const uint64_t cc = cr.link != NONE ? node_ctr(node_ptr(t, base, cr.link)) : cr.ctr;
        n = ctr_n(cc);
        const ulonglong2 rs = root_stream_of(t, g);
        const uint32_t ply = G::stones(s);
        gv = gumbel_variate(rs.x, rs.y, (uint64_t)ply, cr.meta & META_A_MASK, (int32_t)ply + 1 >= t.move.gumbel.temp_threshold);
    }
    ((uint16_t*)t.move.gumbel.base)[(size_t)g * BLOCK_SLOTS + sub] = (uint16_t)n;
    t.move.gumbel.g[(size_t)g * BLOCK_SLOTS + sub] = gv;
}
// what lane sub of a Gumbel move's root holds besides its child's counters: the slot's visits in this move and its variate
struct GumbelLane { uint32_t d; float g; };
AZ_D GumbelLane gumbel_lane(const TreeDev& t, int g, uint32_t nchild, uint32_t n, int sub) {
    GumbelLane r{0u, 0.0f};
    if ((uint32_t)sub < nchild) {
        r.d = (n - (uint32_t)((const uint16_t*)t.move.gumbel.base)[(size_t)g * BLOCK_SLOTS + sub]) & 0xFFFFu;
        r.g = t.move.gumbel.g[(size_t)g * BLOCK_SLOTS + sub];
    }
    return r;
}
// sigma of lane sub's slot: v_mix and max n over the slots in ascending order (group shuffles); *sum_d = t, *max_d = the largest d
template <class G>
AZ_D float gumbel_sigma_lane(const TreeDev& t, uint32_t nchild, uint32_t n, float q, float p, uint32_t d, uint32_t* sum_d, uint32_t* max_d) {
    constexpr int GW = G::GROUP;
    GumbelMix mx{0.0f, 0.0f};
    uint32_t max_n = 0u, sd = 0u, md = 0u;
#pragma unroll
    for (int j = 0; j < G::ACTIONS; ++j) {
        const uint32_t nj = gshfl<GW>(n, j), dj = gshfl<GW>(d, j);
        const float pj = gshflf<GW>(p, j), qj = gshflf<GW>(q, j);
        if ((uint32_t)j < nchild) {
            gumbel_mix_add(mx, pj, qj, nj);
            max_n = nj > max_n ? nj : max_n;
            sd += dj;
            md = dj > md ? dj : md;
        }
    }
    *sum_d = sd;
    *max_d = md;
    return gumbel_sigma(t.move.gumbel.c_visit, t.move.gumbel.c_scale, max_n, n, q, gumbel_vmix(mx));
}

// ---- get_action_prob prologue: root lookup (src/async_mcts.rs:81) + S10 + S1 -------------
// NZ: root noise is on.  A root that already has its prior gets the noise here; one that is evaluated first (LEAF_ROOT) gets it in its
// backup, right after the prior is stored -- once per get_action_prob either way, before the call's first selection.
// noisy (read by the NZ instantiations only): this tree's move gets the noise (false: a fast move under a playout cap)
// GZ (Gumbel root search): the move's baseline is taken here too, on the same moves (`noisy`)
template <class G, bool NZ = false, bool GZ = false>
AZ_D typename G::State root_prepare_body(const TreeDev& t, TreeHead& h, const ulonglong2* root_states, int g, int sub, bool noisy = true) {
    const bool act = h.active != 0;
    size_t base = (size_t)g * t.R;
    typename G::State s = act ? root_states[g] : G::init();
    uint32_t kind = LEAF_NONE;
    if (act) {
        uint32_t found, ins;
        hash_find<G>(t, g, base, s, sub, &found, &ins);
        uint32_t root = found;
        uint32_t n_exp = 0;
        if (found == NONE) {
            // S10 (A11): unseen root -> push + upgrade a fresh node, as NodeStore::from_root (src/node.rs:168-177):
            // the root takes slot 0 of a new block, its children the next block
            uint32_t idx = h.len;
            uint32_t ec_;
            if (idx + BLOCK_SLOTS > t.R) {
                if (sub == 0) atomicOr(&t.err[ERR_CAPACITY], 1u);
            } else if (node_upgrade<G>(t, h, g, base, idx, s, 0u, 0u, ins, CTR_INIT, idx + BLOCK_SLOTS, 1u, sub, &ec_)) {
                root = idx;
                n_exp = 1;
            }
        }
        if (root != NONE) {
            uint32_t meta = (found == NONE) ? 0u : node_load(node_ptr(t, base, root)).meta;
            uint32_t ec_ = (found == NONE) ? G::ended_code(s) : ((meta >> META_ECODE_SHIFT) & 3u);
            if (ec_ != E_NONE) {
                // terminal root: the reference panics at root.mu.p.unwrap() (src/async_mcts.rs:85)
                if (sub == 0) atomicOr(&t.err[ERR_TERMINAL_ROOT], 1u);
            } else if (!(meta & META_HAS_PRIOR)) {
                kind = LEAF_ROOT;  // S1 (A1): evaluate the root once so best_child has a prior (not a simulation: nothing is backed up)
            } else if ((NZ || GZ) && noisy) {
                const NodeRec rr = node_load(node_ptr(t, base, root));
                const uint32_t nchild = (rr.meta >> META_NCHILD_SHIFT) & 7u;
                if constexpr (NZ) {
                    uint4* cp = node_ptr(t, base, rr.child_base + ((uint32_t)sub < nchild ? (uint32_t)sub : 0u));
                    const NodeRec cr = node_load(cp);
                    const float mixed = root_noise_mix<G>(t, g, s, nchild, cr.meta & META_A_MASK, __uint_as_float(cr.prior), sub);
                    if ((uint32_t)sub < nchild) node_set_prior(cp, __float_as_uint(mixed));
                }
                if constexpr (GZ) gumbel_capture<G>(t, g, base, s, nchild, rr.child_base, sub);
            }
        }
        h.root = (root == NONE) ? 0u : root;
        h.leaf = h.root;
        h.path_len = 0;
        if (root == NONE) h.active = 0;       // a failed root deactivates the tree for this search
        h.stat[ST_EXPANSIONS] += n_exp;
    }
    h.leaf_kind = kind;
    return s;
}

template <class G, bool NZ, bool MIR, bool GZ>
__global__ __launch_bounds__(64) void k_root_prepare(TreeDev t, EvalBatch eb, EvalCache ec, const ulonglong2* root_states) {
    constexpr int GW = G::GROUP;
    int tid = blockIdx.x * 64 + threadIdx.x;
    int g = tid / GW, sub = tid % GW;
    if (g >= t.G) return;
    TreeHead h = head_load(t, g);
    bool noisy = true;
    if constexpr (NZ || GZ) noisy = move_noisy(t, g);
    const typename G::State s = root_prepare_body<G, NZ, GZ>(t, h, root_states, g, sub, noisy);
    const uint32_t src = leaf_request<G, MIR>(eb, ec, h.leaf_kind == LEAF_ROOT, s, sub);
    if (h.leaf_kind == LEAF_ROOT) h.src = src;
    if (sub == 0) head_store(t, g, h);
}

// ---- search_iteration: select + expand (src/async_mcts.rs:226-299, Appendix A of SURVEY.md) ----
// MT (several simulations in flight per tree, src/async_mcts.rs:191-217 as a lock-step schedule): the thread sees the Locked slots
// earlier threads of the step hold.  C8 (src/async_mcts.rs:253-258, :275; src/node.rs:359-365): if the arg-max over all children is
// Locked, the retry excludes Locked children.  Two sites where the reference panics have no legal continuation and are repaired by
// ABANDONING the simulation (its visits are reverted exactly, it counts toward num_sims; *abandoned = 1):
//   S11  every child is Locked: `max_by` on an empty iterator -> `unwrap()` (src/node.rs:366-367)
//   S12  a link leads to a node that is Locked, i.e. expanded by an earlier thread of this step and still without its prior:
//        `p.as_ref().unwrap()` (src/node.rs:354)
// go = false (playout cap only): the tree's move has had its budget -- nothing is selected, the tree asks for no leaf
// FP (forced playouts, az_forced.h): at the FIRST level of the simulation -- the node is the call's root -- a child that has been visited and
// is still short of nf = sqrt(k * p * S) gets u = +inf; the arg-max, the Locked filter (C8), S11 and S12 then run on the u as written.
// forced (read by the RR != RR_NONE instantiations only): this tree's move is a forced / Gumbel move (false: a fast move under a playout cap)
// RR_GUMBEL (az_gumbel.h): at the first level the children's u is s_j = (g_j + l_j) + sigma_j for the slots whose visits in this move equal
// the considered visit count c(t), -inf for the others; PUCT does not decide there.  Every level below the root is unchanged.
template <class G, bool MT = false, int RR = RR_NONE>
AZ_D typename G::State select_body(const TreeDev& t, TreeHead& h, PathRegs& pth, const SearchParams& sp, int g, int sub, uint32_t* path,
                                   uint32_t* abandoned = nullptr, bool go = true, bool forced = true) {
    constexpr int GW = G::GROUP;
    constexpr int NA = G::ACTIONS;
    const bool act = h.active != 0 && go;
    const size_t base = (size_t)g * t.R;
    bool give_up = false, cur_visited = false;
    uint32_t cur = h.root;
    uint32_t depth = 0, plen = 0, kind = LEAF_NONE;
    float val = 0.0f;
    uint32_t n_exp = 0, n_link = 0, n_term = 0, n_depth = 0;
    typename G::State leaf_s = G::init();
    // The record of an expanded child chosen at one level IS the parent of the next level and is already in the registers of
    // the lane that evaluated it: it is handed down by shuffles, so a level costs one dependent fetch (the child block), not
    // two.  Only the root and link targets (canonical nodes living elsewhere) are fetched by slot.
    NodeRec pr{};
    bool have_pr = false;
    bool at_root = true;                                        // RR only: the loop's first pass
    uint32_t gz_relink = NONE;                                  // RR_GUMBEL only: the root slot whose placeholder this simulation just turned into a link
    while (act) {
        uint4* pp = node_ptr(t, base, cur);
        if (!have_pr) pr = node_load(pp);
        have_pr = false;
        if constexpr (RR == RR_GUMBEL) {
            // the slot's visits before this move are those of the node it now resolves to, not the placeholder's 0 the baseline took
            if (gz_relink != NONE) {
                if ((uint32_t)sub == gz_relink) ((uint16_t*)t.move.gumbel.base)[(size_t)g * BLOCK_SLOTS + sub] = (uint16_t)ctr_n(pr.ctr);
                gz_relink = NONE;
            }
        }
        if constexpr (MT) { if (pr.meta & META_LOCKED) { give_up = true; cur_visited = false; break; } }   // S12
        const uint64_t pc = pr.ctr + CTR_VISIT;                 // visit(), src/node.rs:77-80; S5: before the checks
        if (sub == 0) node_set_ctr(pp, pc);
        const uint32_t ecd = (pr.meta >> META_ECODE_SHIFT) & 3u;
        if (depth > sp.max_depth) { val = 0.0f; kind = LEAF_VALUE; break; }   // src/async_mcts.rs:241-244 (B10)
        if (ecd != E_NONE) { val = ecode_value(ecd); kind = LEAF_VALUE; ++n_term; break; }  // :246-249
        // best_child, src/node.rs:343-370
        const uint32_t nchild = (pr.meta >> META_NCHILD_SHIFT) & 7u, cb = pr.child_base;
        const float sq = puct_sqrt_parent(ctr_n(pc));
        NodeRec cr{0ull, 0u, 0u, NONE, 0u};
        float u = 0.0f;
        uint32_t fn = 0u;                                       // RR only: this lane's n_j (0 beyond nchild)
        float fq = 0.0f;                                        // RR_GUMBEL only: this lane's q_j
        if ((uint32_t)sub < nchild) {
            // the child's record carries its own counter; only a link slot needs the second, dependent fetch of the
            // canonical node's counter (resolve(), src/node.rs:179-193)
            cr = node_load(node_ptr(t, base, cb + sub));
            uint64_t cc = cr.ctr;
            if (cr.link != NONE) cc = node_ctr(node_ptr(t, base, cr.link));
            u = puct(cc, __uint_as_float(cr.prior), sq, sp.cpuct_f);
            if constexpr (RR != RR_NONE) fn = ctr_n(cc);
            if constexpr (RR == RR_GUMBEL) fq = ctr_q(cc);
        }
        if constexpr (RR == RR_GUMBEL) {
            if (at_root && forced) {
                const GumbelLane gl = gumbel_lane(t, g, nchild, fn, sub);
                const float p = __uint_as_float(cr.prior);
                uint32_t tt, md;
                const float sigma = gumbel_sigma_lane<G>(t, nchild, fn, fq, p, gl.d, &tt, &md);
                const uint32_t m_eff = t.move.gumbel.m < nchild ? t.move.gumbel.m : nchild;
                const uint32_t want = gumbel_considered_visit(m_eff, t.move.gumbel.num_sims, tt);
                u = ((uint32_t)sub < nchild && gl.d == want) ? gumbel_score(gl.g, gumbel_logit(p), sigma) : -__builtin_inff();
            }
            at_root = false;
        }
        if constexpr (RR == RR_FORCED) {
            if (at_root && forced) {
                uint32_t S = 0u;
#pragma unroll
                for (int j = 0; j < NA; ++j) S += gshfl<GW>(fn, j);
                if ((uint32_t)sub < nchild && forced_child(t.move.forced.k, __uint_as_float(cr.prior), S, fn)) u = __builtin_inff();
            }
            at_root = false;
        }
        uint32_t best = 0;
        float bu = gshflf<GW>(u, 0);
#pragma unroll
        for (int j = 1; j < NA; ++j) {                          // max_by: later element wins unless earlier is Greater (C7)
            float uj = gshflf<GW>(u, j);
            if ((uint32_t)j < nchild && !(bu > uj)) { best = (uint32_t)j; bu = uj; }
        }
        ++n_depth;
        if constexpr (MT) {
            const uint32_t lockm = gballot<GW>((uint32_t)sub < nchild && (cr.meta & META_LOCKED)) & ((1u << NA) - 1u);
            if ((lockm >> best) & 1u) {                         // C8: the winner is Locked -> retry without the Locked children
                bool have = false;
#pragma unroll
                for (int j = 0; j < NA; ++j) {
                    const float uj = gshflf<GW>(u, j);
                    if ((uint32_t)j >= nchild || ((lockm >> j) & 1u)) continue;
                    if (!have || !(bu > uj)) { best = (uint32_t)j; bu = uj; have = true; }
                }
                if (!have) { give_up = true; cur_visited = true; break; }       // S11
            }
        }
        const uint32_t clink = gshfl<GW>(cr.link, (int)best), cmeta = gshfl<GW>(cr.meta, (int)best), cprior = gshfl<GW>(cr.prior, (int)best);
        const uint32_t cslot = cb + best;
        if (plen >= (uint32_t)PATH_CAP) {
            if (sub == 0) atomicOr(&t.err[ERR_PATH], 1u);
            kind = LEAF_NONE;
            break;
        }
        if (plen < (uint32_t)PATH_INLINE) {                      // node_path.push, S3 / :270: lane plen & 7 keeps it
            if ((uint32_t)sub == (plen & 7u)) { if (plen < 8u) pth.lo = cur; else pth.hi = cur; }
        } else if (sub == 0) {
            path[plen] = cur;
        }
        ++plen;
        if (clink != NONE) { cur = clink; ++depth; continue; }  // Exists(false): follow the link (S2: one level per iteration)
        if (cmeta & META_EXPANDED) {                             // Exists(true)
            pr.ctr = gshfl64<GW>(cr.ctr, (int)best);
            pr.meta = cmeta;
            pr.child_base = gshfl<GW>(cr.child_base, (int)best);
            have_pr = true;
            cur = cslot;
            ++depth;
            continue;
        }
        // PlaceHolder (:261-268, S3): expand it.  B1: play the child's own action.
        // the parent's state: the one fetch of a simulation that goes to the key array (the levels above only read 16-byte records)
        const typename G::State s2 = G::play(G::unpack(node_key(t, base, cur)), (int)(cmeta & META_A_MASK));       // :284-287 (B5)
        uint32_t found, ins;
        hash_find<G>(t, g, base, s2, sub, &found, &ins);
        if (found != NONE) {                                    // upgrade -> Some(false): become a link (src/node.rs:285-289)
            if (sub == 0) node_set_word(node_ptr(t, base, cslot), cmeta, found, 0u);
            if constexpr (RR == RR_GUMBEL) { if (plen == 1u && forced) gz_relink = best; }      // (plen == 1: still the first pass, the node is the root)
            cur = found;
            ++n_link;
            continue;                                           // :297-298
        }
        uint32_t ec2;
        // the placeholder is visited right after the upgrade (:309): its counter becomes INIT + VISIT
        if (!node_upgrade<G>(t, h, g, base, cslot, s2, cprior, cmeta & META_A_MASK, ins, CTR_INIT + CTR_VISIT, h.len, 0u, sub, &ec2,
                             MT ? META_LOCKED : 0u)) {
            kind = LEAF_NONE;
            break;
        }
        ++n_exp;
        cur = cslot;
        if (ec2 != E_NONE) { val = ecode_value(ec2); kind = LEAF_VALUE; break; }   // S4 (A5)
        kind = LEAF_EVAL;                                       // :303-315: goes to the net
        leaf_s = s2;
        break;
    }
    if constexpr (MT) {
        if (give_up) {
            // revert this simulation's visits exactly (N - 1, vloss - 1): node_path[0 .. plen) and, if it was visited, cur.
            // Lane sub holds node_path entries sub and sub + 8; a line never repeats a node, so the lanes touch distinct counters.
            const uint32_t total = plen + (cur_visited ? 1u : 0u);
            for (uint32_t r = 0; r < total; r += GW) {
                const uint32_t i = r + (uint32_t)sub;
                if (i < total) {
                    const uint32_t node = i < plen ? (i < 8u ? pth.lo : (i < (uint32_t)PATH_INLINE ? pth.hi : path[i])) : cur;
                    uint4* np = node_ptr(t, base, node);
                    node_set_ctr(np, node_ctr(np) - CTR_VISIT);
                }
            }
            kind = LEAF_NONE;
            if (abandoned) *abandoned = 1u;
        }
    }
    if (act) {
        h.leaf = cur;
        h.leaf_val = val;
        h.path_len = plen;
        h.stat[ST_SIMS] += 1;
        h.stat[ST_EXPANSIONS] += n_exp;
        h.stat[ST_LINK_HITS] += n_link;
        h.stat[ST_TERMINAL_HITS] += n_term;
        h.stat[ST_DEPTH_SUM] += n_depth;
    }
    h.leaf_kind = kind;
    return leaf_s;
}

// `seen`-style sharing of evaluations across trees: a tree whose row was really evaluated publishes (pi, v) under its
// state's key.  Bucket = one 64-byte line of 8 keys.  The claim (a CAS of an empty way, starting at a way picked by the key's
// hash) is ISSUED as soon as the leaf's key is known and CHECKED at the end of the backup, so its round trip overlaps the
// prior / counter updates; a way taken by another key costs one more attempt on the next way (at most three).
struct CacheClaim {
    unsigned long long key, prev;
    uint32_t slot;
    bool open;
};
template <class G>
AZ_D CacheClaim cache_claim_begin(const EvalCache& ec, typename G::State s, int sub) {
    CacheClaim c{0ull, 0ull, 0u, false};
    if (G::stones(s) > ec.max_stones) return c;
    c.key = (unsigned long long)G::pack(s) | ec.tag;
    const unsigned long long hsh = mix64(c.key);
    c.slot = ((uint32_t)(hsh >> 20) & ec.bmask) * 8u + ((uint32_t)(hsh >> 50) & 7u);
    c.open = true;
    if (sub == 0) c.prev = atomicCAS(&ec.key[c.slot], 0ull, c.key);
    return c;
}
template <class G>
AZ_D void cache_claim_finish(const EvalCache& ec, CacheClaim c, float pv, int sub) {
    constexpr int GW = G::GROUP;
    bool inserted = false;
    if (c.open) {
        unsigned long long prev = gshfl64<GW>(c.prev, 0);
        for (int attempt = 0; prev != 0ull && prev != c.key && attempt < 2; ++attempt) {
            c.slot = (c.slot & ~7u) | ((c.slot + 1u) & 7u);
            if (sub == 0) prev = atomicCAS(&ec.key[c.slot], 0ull, c.key);
            prev = gshfl64<GW>(prev, 0);
        }
        if (prev == 0ull) {                               // claimed (prev == key: already published; else: bucket busy, not cached)
            ec.pv[(size_t)c.slot * 8 + sub] = pv;
            inserted = true;
        }
    }
    const unsigned long long im = __ballot(inserted && sub == 0);
    if (ec.stat && im && (int)(threadIdx.x & 63) == __ffsll((long long)im) - 1)
        atomicAdd(&ec.stat[(size_t)(blockIdx.x % DD_REPLICAS) * DD_STRIDE + DD_INSERTS], (unsigned long long)__popcll(im));
}

// ---- mask/renormalise/store the prior (src/async_mcts.rs:317-353) + backup (:361-370) ----
// INLINE_PV: the leaf's (pi, v) row is handed over in a register (pv_in: lane a < ACTIONS holds pi[a], lane ACTIONS holds v)
// instead of being read through TreeHead.src -- the fused search of the fixture nets.
// GZ (Gumbel root search): the root's own evaluation is also where the move's baseline is taken (gumbel_capture), on the same moves
template <class G, bool INLINE_PV = false, bool NZ = false, bool MIR = false, bool GZ = false>
AZ_D void backup_body(const TreeDev& t, TreeHead& h, const PathRegs& pth, const EvalBatch& eb, const EvalCache& ec, int g,
                      int sub, const uint32_t* path, float pv_in = 0.0f, bool noisy = true /*NZ only: see root_prepare_body*/) {
    constexpr int GW = G::GROUP;
    constexpr int NA = G::ACTIONS;
    const uint32_t kind = h.leaf_kind;
    if (kind == LEAF_NONE) return;
    const size_t base = (size_t)g * t.R;
    const uint32_t leaf = h.leaf;
    float val;
    float pv = 0.0f;                                // lanes 0..NA-1: pi[sub], lane NA: v
    CacheClaim claim{0ull, 0ull, 0u, false};
    bool publish = false;
    const bool apply_only = kind == LEAF_ROOT;            // the root's own evaluation: store the prior, back nothing up
    if (kind == LEAF_EVAL || kind == LEAF_ROOT) {
        uint4* lp = node_ptr(t, base, leaf);
        const NodeRec lr = node_load(lp);
        const typename G::Packed lkey = node_key(t, base, leaf);
        const typename G::State s = G::unpack(lkey);
        const uint32_t src = h.src;
        // "eval_mirror": the row behind src is the raw N(c(s)); whether this tree's s is the mirrored one is recomputed from the leaf's own
        // key, which the backup loads anyway (TreeHead.src has no free bit: SRC_INDEX is used up at 2^30 cache entries)
        bool mir = false;
        if constexpr (MIR) mir = G::mirrored_key(lkey);
        if constexpr (INLINE_PV) {
            pv = pv_in;
        } else if (src & SRC_CACHE) {
            pv = ec.pv[(size_t)(src & SRC_INDEX) * 8 + sub];
        } else {
            const uint32_t row = (src & SRC_TABLE) ? eb.tuniq[src & SRC_INDEX] : src;
            pv = eb.pi[(size_t)row * 8 + sub];
            publish = !(src & SRC_TABLE) && eb.dedup && ec.key;
            if (publish) claim = cache_claim_begin<G>(ec, mir ? G::mirror(s) : s, sub);       // under the key of c(s), with the raw row
        }
        float p = sub < NA ? pv : 0.0f;
        const float v = gshflf<GW>(pv, NA);
        if constexpr (MIR) {                                        // F(s).pi[a] = N(c(s)).pi[mirror_action(a)]; pv stays raw for the cache
            const float pm = gshflf<GW>(pv, G::mirror_action(sub < NA ? sub : 0));
            if (mir && sub < NA) p = pm;
        }
        if (t.log_cap > 0) {
            uint32_t n = h.log_len;
            if (n < (uint32_t)t.log_cap) {
                size_t li = (size_t)(t.log_row ? t.log_row[g] : g) * t.log_cap + n;
                if (sub < NA) t.log_pi[li * NA + sub] = p;
                if (sub == 0) { t.log_v[li] = v; t.log_state[li] = s; }
            }
            h.log_len = n + 1;
        }
        const uint32_t vm = G::valid_mask(s);
        const bool valid = sub < NA && ((vm >> sub) & 1u);
        if (!valid) p = 0.0f;                                       // :322-326
        float sum = 0.0f;
#pragma unroll
        for (int a = 0; a < NA; ++a) sum = __fadd_rn(sum, gshflf<GW>(p, a));   // :328 (sequential, C10)
        if (sum > 0.0f) {
            p = __fdiv_rn(p, sum);                                  // :331
        } else {
            p = __fadd_rn(p, valid ? 1.0f : 0.0f);                  // :340-342
            float s2 = 0.0f;
#pragma unroll
            for (int a = 0; a < NA; ++a) s2 = __fadd_rn(s2, gshflf<GW>(p, a));
            p = __fdiv_rn(p, s2);                                   // :344
        }
        const uint32_t nchild = (lr.meta >> META_NCHILD_SHIFT) & 7u, cb = lr.child_base;
        const uint32_t myact = (uint32_t)sub < nchild ? nth_set_bit<NA>(vm, (uint32_t)sub) : 0u;
        float pa = gshflf<GW>(p, (int)myact);
        if constexpr (NZ) { if (apply_only && noisy) pa = root_noise_mix<G>(t, g, s, nchild, myact, pa, sub); }      // the root's own evaluation: mix the noise in
        if ((uint32_t)sub < nchild) node_set_prior(node_ptr(t, base, cb + sub), __float_as_uint(pa));   // set_policy, :348
        if (sub == 0) node_set_word(lp, (lr.meta | META_HAS_PRIOR) & ~META_LOCKED, lr.link, lr.child_base);      // set_policy + unlock, :348-351
        if constexpr (GZ) { if (apply_only && noisy) gumbel_capture<G>(t, g, base, s, nchild, cb, sub); }
        h.stat[ST_LEAF_EVALS] += 1;
        val = -v;                                                   // :353 (C9)
    } else {
        val = h.leaf_val;
    }
    if (!apply_only) {
        // unvisit() leaf -> root along node_path; B2: the sign alternates toward the root.
        // A Connect Four line never repeats a node, so the lanes update distinct counters.
        const uint32_t plen = h.path_len;
        for (uint32_t r = 0; r <= plen; r += GW) {                      // round r: lane sub takes step i = r + sub (group-uniform trips)
            const uint32_t i = r + (uint32_t)sub;
            const uint32_t j = i >= 1u && i <= plen ? plen - i : 0u;    // node_path index of step i >= 1
            const uint32_t lo = gshfl<GW>(pth.lo, (int)(j & 7u)), hi = gshfl<GW>(pth.hi, (int)(j & 7u));
            if (i <= plen) {
                uint32_t node = i == 0 ? leaf : (j < 8u ? lo : (j < (uint32_t)PATH_INLINE ? hi : path[j]));
                float x = (i & 1u) ? -val : val;
                uint4* np = node_ptr(t, base, node);
                node_set_ctr(np, node_ctr(np) - ctr_unvisit_delta(x));  // src/node.rs:83-92
            }
        }
    }
    if constexpr (!INLINE_PV) { if (publish) cache_claim_finish<G>(ec, claim, pv, sub); }
}

// ---- get_action_prob epilogue (src/async_mcts.rs:84-114): counts -> pi ----------------------
struct RootPolicy {
    float pi;        // this lane's action (sub < ACTIONS)
    uint32_t count;
    float q;
    int32_t sel;     // RR_GUMBEL on a Gumbel move: the selected action (the same in every lane); else -1
};
// RR_FORCED && forced && t.move.forced.prune (policy target pruning, az_forced.h): pi is formed from the PRUNED counts; count and q stay raw
// RR_GUMBEL && forced (az_gumbel.h): pi = softmax(l + sigma) over the root's slots and sel = the selected action; count and q stay raw,
// temp and the tie-break stream are not used
template <class G, int RR = RR_NONE>
AZ_D RootPolicy root_policy(const TreeDev& t, uint32_t root, int g, int sub, float temp, uint64_t seed, uint64_t game_id, uint64_t ply,
                            bool forced = true) {
    constexpr int GW = G::GROUP;
    constexpr int NA = G::ACTIONS;
    const size_t base = (size_t)g * t.R;
    const NodeRec pr = node_load(node_ptr(t, base, root));
    const uint32_t nchild = (pr.meta >> META_NCHILD_SHIFT) & 7u, cb = pr.child_base;
    uint32_t ca = 0, cn = 0;
    float cq = 0.0f, cp = 0.0f;                                     // cp (FP only): the slot's stored prior
    if ((uint32_t)sub < nchild) {
        const NodeRec cr = node_load(node_ptr(t, base, cb + sub));
        const uint64_t cc = cr.link != NONE ? node_ctr(node_ptr(t, base, cr.link)) : cr.ctr;
        ca = cr.meta & META_A_MASK;                                 // B3: the slot's own action
        cn = ctr_n(cc);
        cq = ctr_q(cc);
        if constexpr (RR != RR_NONE) cp = __uint_as_float(cr.prior);
    }
    RootPolicy out{0.0f, 0u, 0.0f, -1};
#pragma unroll
    for (int j = 0; j < NA; ++j) {                                  // counts[a] = n, :88-94
        uint32_t aj = gshfl<GW>(ca, j), nj = gshfl<GW>(cn, j);
        float qj = gshflf<GW>(cq, j);
        if ((uint32_t)j < nchild && aj == (uint32_t)sub) { out.count = nj; out.q = qj; }
    }
    if constexpr (RR == RR_GUMBEL) {
        if (forced) {
            const bool in = (uint32_t)sub < nchild;
            const GumbelLane gl = gumbel_lane(t, g, nchild, cn, sub);
            uint32_t tt, md;
            const float sigma = gumbel_sigma_lane<G>(t, nchild, cn, cq, cp, gl.d, &tt, &md);
            const float l = gumbel_logit(cp);
            const float x = gumbel_x(l, sigma);
            const float u = (in && gl.d == md) ? gumbel_score(gl.g, l, sigma) : -__builtin_inff();
            float max_x = gshflf<GW>(x, 0);
            uint32_t best = 0;
            float bu = gshflf<GW>(u, 0);
#pragma unroll
            for (int j = 1; j < NA; ++j) {
                const float xj = gshflf<GW>(x, j), uj = gshflf<GW>(u, j);
                if ((uint32_t)j < nchild && xj > max_x) max_x = xj;
                if ((uint32_t)j < nchild && !(bu > uj)) { best = (uint32_t)j; bu = uj; }
            }
            const float e = in ? gumbel_softmax_term(x, max_x) : 0.0f;
            float sum = 0.0f;
#pragma unroll
            for (int j = 0; j < NA; ++j) {
                const float ej = gshflf<GW>(e, j);
                if ((uint32_t)j < nchild) sum = __fadd_rn(sum, ej);
            }
            const float ps = __fdiv_rn(e, sum);
#pragma unroll
            for (int j = 0; j < NA; ++j) {
                const uint32_t aj = gshfl<GW>(ca, j);
                const float pj = gshflf<GW>(ps, j);
                if ((uint32_t)j < nchild && aj == (uint32_t)sub) out.pi = pj;
            }
            out.sel = (int32_t)gshfl<GW>(ca, (int)best);
            return out;
        }
    }
    uint32_t pcount = out.count;                                    // what pi is formed from: the raw count, or ...
    if constexpr (RR == RR_FORCED) {
        if (forced && t.move.forced.prune) {                             // ... the pruned one
            uint32_t S = 0u, b = 0u, bn = 0u;
#pragma unroll
            for (int j = 0; j < NA; ++j) {
                const uint32_t nj = gshfl<GW>(cn, j);               // (0 beyond nchild)
                S += nj;
                if ((uint32_t)j < nchild && nj >= bn) { b = (uint32_t)j; bn = nj; }      // the most visited slot, the highest among equals
            }
            const float sq = forced_sqrt_parent(ctr_n(pr.ctr));
            const float u_star = forced_puct(gshflf<GW>(cq, (int)b), bn, gshflf<GW>(cp, (int)b), sq, t.move.forced.cpuct_f);
            uint32_t cm = cn;
            if ((uint32_t)sub < nchild && (uint32_t)sub != b && cn > 0u) cm = forced_prune(t.move.forced.k, cp, S, cn, cq, sq, t.move.forced.cpuct_f, u_star);
            pcount = 0u;
#pragma unroll
            for (int j = 0; j < NA; ++j) {
                const uint32_t aj = gshfl<GW>(ca, j), mj = gshfl<GW>(cm, j);
                if ((uint32_t)j < nchild && aj == (uint32_t)sub) pcount = mj;
            }
        }
    }
    if (temp == 0.0f) {                                             // :97-107
        uint32_t mx = 0;
#pragma unroll
        for (int a = 0; a < NA; ++a) { uint32_t ca2 = gshfl<GW>(pcount, a); mx = ca2 > mx ? ca2 : mx; }
        uint32_t ties = gballot<GW>(sub < NA && pcount == mx) & ((1u << NA) - 1u);
        uint64_t r = rng_draw(seed, game_id, ply, RNG_TIEBREAK);
        uint32_t pick = nth_set_bit<NA>(ties, rng_choose(r, (uint32_t)__popc(ties)));
        out.pi = ((uint32_t)sub == pick) ? 1.0f : 0.0f;
    } else {                                                        // S6 (A7): counts^(1/temp) / sum
        float inv_t = __fdiv_rn(1.0f, temp);
        float x = (inv_t == 1.0f) ? (float)pcount : powf((float)pcount, inv_t);   // :109
        if (sub >= NA) x = 0.0f;
        float sum = 0.0f;
#pragma unroll
        for (int a = 0; a < NA; ++a) sum = __fadd_rn(sum, gshflf<GW>(x, a));           // :110
        out.pi = __fdiv_rn(x, sum);
    }
    return out;
}

// ---- the decided-move stop (az_stop.h; only the PC_STOP instantiations contain it) ---------------------------------------------------------
// The decision of one tree's 8 lanes: lane j reads root child j's visit count as root_policy reads it (a link slot resolved to its canonical
// node, the raw u16), the two largest are taken over the slots by group shuffles.  It reads the root record and its child block, the two
// lines the selection loads next.  The caller has made the backup's counter stores visible (the wave fence).
template <class G>
AZ_D bool stop_root_decided(const TreeDev& t, uint32_t root, int g, int sub, uint32_t left) {
    constexpr int GW = G::GROUP;
    const size_t base = (size_t)g * t.R;
    const NodeRec pr = node_load(node_ptr(t, base, root));
    const uint32_t nchild = (pr.meta >> META_NCHILD_SHIFT) & 7u, cb = pr.child_base;
    uint32_t n = 0u;
    if ((uint32_t)sub < nchild) {
        const NodeRec cr = node_load(node_ptr(t, base, cb + sub));
        n = ctr_n(cr.link != NONE ? node_ctr(node_ptr(t, base, cr.link)) : cr.ctr);
    }
    uint32_t n1 = 0u, n2 = 0u;
#pragma unroll
    for (int j = 0; j < G::ACTIONS; ++j) {
        const uint32_t nj = gshfl<GW>(n, j);
        if ((uint32_t)j < nchild) stop_top2(n1, n2, nj);
    }
    return stop_decided(n1, n2, left);
}

// the batch a launch consumes gets its election table cleared (nothing reads the keys any more: the backups read tuniq)
AZ_D void clear_election_keys(const EvalBatch& eb) {
    if (!eb.dedup) return;
    const uint32_t total = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i <= eb.tmask; i += total) eb.tkey[i] = 0ull;
}
template <class G, bool NZ, bool MIR, bool GZ>
__global__ __launch_bounds__(64) void k_backup(TreeDev t, EvalBatch eb, EvalCache ec) {
    constexpr int GW = G::GROUP;
    const int tid = blockIdx.x * 64 + threadIdx.x;
    const int g = tid / GW, sub = tid % GW;
    if (tid == 0) { if (eb.max_n && *eb.n > *eb.max_n) *eb.max_n = *eb.n; *eb.n = 0; }   // the batch has been consumed (nothing in this kernel reads the count)
    clear_election_keys(eb);
    if (g >= t.G) return;
    TreeHead h = head_load(t, g);
    const PathRegs pth = path_load(t, g, sub);
    bool noisy = true;
    if constexpr (NZ || GZ) noisy = move_noisy(t, g);
    backup_body<G, false, NZ, MIR, GZ>(t, h, pth, eb, ec, g, sub, t.path + (size_t)g * PATH_CAP, 0.0f, noisy);
    h.leaf_kind = LEAF_NONE;
    if (sub == 0) head_store(t, g, h);
}

// backup of simulation i and select of simulation i+1 in one launch: both belong to the same 8 lanes of the same tree and
// nothing else touches that tree in between.  The leaf of i+1 goes into the OTHER eval batch (eb_next; its count was
// zeroed by the previous launch, this one zeroes eb_prev's), so the two ping-pong.
// PC (playout cap): TreeHead.active carries the simulations the tree's move has left (1 | left << 1); a tree with none left selects nothing
// and requests no leaf for the rest of the round -- its last backup above still runs, and its lanes still go through leaf_request's
// workgroup-wide row claim as an inactive tree's do.  So a replayed graph chunk in which some trees are done is correct as it is.
// PC_STOP (the decided-move stop): TreeHead.active is a stop_word (az_stop.h).  Between the backup and the selection an eligible tree that
// still has simulations left takes the decision; a decided tree keeps its `left`, sets STOP_DECIDED_BIT and from then on is a tree with none
// left: it selects nothing, requests no leaf and goes through leaf_request's claim as an inactive tree does.
// RR (the root rule): select_body's forced / Gumbel branch at the root, on the tree's forced / Gumbel moves
template <class G, bool STAMP, bool NZ, bool MIR, int PC, int RR>     // STAMP: diagnostic build, per-wave s_memtime stamps of the kernel's phases into dbg[wave][8]
__global__ __launch_bounds__(256) void k_backup_select(TreeDev t, EvalBatch eb_prev, EvalBatch eb_next, EvalCache ec,
                                                       SearchParams sp, unsigned long long* dbg) {
    static_assert(PC != PC_STOP || RR == RR_NONE, "the decided-move stop is stated for the PUCT root: no such instantiation (RR_OF_PC)");
    constexpr int GW = G::GROUP;
    const int tid = blockIdx.x * blockDim.x + threadIdx.x;      // 64 or 256 threads (256 only when every wave of the grid holds trees)
    const int g = tid / GW, sub = tid % GW;
    unsigned long long ts[7] = {0, 0, 0, 0, 0, 0, 0};
#define AZ_TSTAMP(i_) if constexpr (STAMP) { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); ts[i_] = __builtin_amdgcn_s_memtime(); }
    AZ_TSTAMP(0);
    if (tid == 0) { if (eb_prev.max_n && *eb_prev.n > *eb_prev.max_n) *eb_prev.max_n = *eb_prev.n; *eb_prev.n = 0; }
    clear_election_keys(eb_prev);
    if (g >= t.G) return;
    TreeHead h = head_load(t, g);
    PathRegs pth = path_load(t, g, sub);
    AZ_TSTAMP(1);
    constexpr bool GZ = RR == RR_GUMBEL;
    bool noisy = true;
    if constexpr (NZ || GZ) noisy = move_noisy(t, g);
    backup_body<G, false, NZ, MIR, GZ>(t, h, pth, eb_prev, ec, g, sub, t.path + (size_t)g * PATH_CAP, 0.0f, noisy);
    AZ_TSTAMP(2);
    // the counters this tree's other lanes just wrote are read by the selection below
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    AZ_TSTAMP(3);
    bool go = true;
    if constexpr (PC == PC_BUDGET) go = (h.active >> 1) != 0u;
    if constexpr (PC == PC_STOP) {
        go = (h.active & 1u) != 0u && stop_left(h.active) != 0u && !(h.active & STOP_DECIDED_BIT);
        if (go && (h.active & STOP_ELIGIBLE_BIT)) {
            if (stop_root_decided<G>(t, h.root, g, sub, stop_left(h.active))) { h.active |= STOP_DECIDED_BIT; go = false; }
        }
    }
    bool forced = true;
    if constexpr (RR != RR_NONE) forced = move_noisy(t, g);
    const typename G::State leaf_s = select_body<G, false, RR>(t, h, pth, sp, g, sub, t.path + (size_t)g * PATH_CAP, nullptr, go, forced);
    if constexpr (PC != PC_NONE) { if (go) h.active -= 2u; }
    AZ_TSTAMP(4);
    const uint32_t src = leaf_request<G, MIR>(eb_next, ec, h.leaf_kind == LEAF_EVAL, leaf_s, sub);
    AZ_TSTAMP(5);
    if (h.leaf_kind == LEAF_EVAL) h.src = src;
    if (sub == 0) head_store(t, g, h);
    path_store(t, g, sub, pth);
    AZ_TSTAMP(6);
#undef AZ_TSTAMP
    if constexpr (STAMP) {
        if (dbg && (threadIdx.x & 63) == 0 && h.active && h.leaf_kind == LEAF_EVAL) {      // a wave whose first tree searched and asked for a row
            unsigned long long* o = dbg + (size_t)(tid >> 6) * 8;
            for (int i = 0; i < 6; ++i) o[i] = ts[i + 1] - ts[i];
            o[6] = ts[6] - ts[0];
        }
    }
}

AZ_D void group_memory_sync() {
    // what one lane of the group stored (node records, node_path, counters) is read by its other lanes next
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- several simulations in flight per tree: ONE lock-step step (src/async_mcts.rs:191-217 as a deterministic schedule) ----------
// The T threads of a tree are served by the tree's 8 lanes one after the other.  Backups of the previous step's leaves in thread
// order (mask/renorm/store the prior, unlock, unvisit along the thread's own node_path), then T selections in thread order: thread
// tt sees the N + 1 / vloss + 1 of the threads before it (visit(), src/node.rs:77-80; Q = (W - vloss) / N, :51-58) and their Locked
// leaves (C8).  Each thread's leaf request goes into the step's batch, so a step evaluates up to T rows per tree together.
// The per-thread part of the search state lives in t.thr[g*T + tt]; t.head[g] keeps what the threads share.
struct ThreadRegs { uint32_t leaf, leaf_kind; float leaf_val; uint32_t src, path_len; };
AZ_D void thread_to_head(TreeHead& h, const ThreadRegs& r) { h.leaf = r.leaf; h.leaf_kind = r.leaf_kind; h.leaf_val = r.leaf_val; h.src = r.src; h.path_len = r.path_len; }
AZ_D ThreadRegs head_to_thread(const TreeHead& h) { return ThreadRegs{h.leaf, h.leaf_kind, h.leaf_val, h.src, h.path_len}; }
// PC (playout cap): as in k_backup_select; a step takes T simulations off what the tree's move has left (budgets are multiples of T)
template <class G, bool NZ, bool MIR, bool PC, int RR>
__global__ __launch_bounds__(64) void k_step_mt(TreeDev t, EvalBatch eb_prev, EvalBatch eb_next, EvalCache ec, SearchParams sp, int first, int last) {
    static_assert(RR != RR_GUMBEL, "never launched with Gumbel on: no such instantiation (AZ_FOR_RR)");
    constexpr int GW = G::GROUP;
    const int tid = blockIdx.x * 64 + threadIdx.x;
    const int g = tid / GW, sub = tid % GW;
    if (tid == 0) { if (eb_prev.max_n && *eb_prev.n > *eb_prev.max_n) *eb_prev.max_n = *eb_prev.n; *eb_prev.n = 0; }
    clear_election_keys(eb_prev);
    if (g >= t.G) return;
    TreeHead h = head_load(t, g);
    const ThreadRegs root_req = head_to_thread(h);          // first: k_root_prepare left the root's evaluation request in the head (S1)
    const int T = t.T;
    int tt0 = 0;
    if constexpr (NZ) {
        // the root's own evaluation (the only backup of a first step) is where the noise goes in: peeled out of the thread loop, which
        // then runs the noise-free body
        if (first) {
            PathRegs pth{0u, 0u};
            thread_to_head(h, root_req);
            backup_body<G, false, true, MIR>(t, h, pth, eb_prev, ec, g, sub, t.path + (size_t)g * T * PATH_CAP, 0.0f, move_noisy(t, g));
            tt0 = T;
        }
    }
    for (int tt = tt0; tt < T; ++tt) {                      // backups in thread order
        TreeLine* tl = t.thr + (size_t)g * T + tt;
        ThreadRegs r{0u, LEAF_NONE, 0.0f, 0u, 0u};
        PathRegs pth{0u, 0u};
        if (first) { if (tt == 0) r = root_req; }
        else {
            const uint4 a = ((const uint4*)tl)[1];
            r = ThreadRegs{a.x, a.y, __uint_as_float(a.z), a.w, tl->head.path_len};
            pth = PathRegs{tl->path16[sub], tl->path16[8 + sub]};
        }
        thread_to_head(h, r);
        backup_body<G, false, false, MIR>(t, h, pth, eb_prev, ec, g, sub, t.path + ((size_t)g * T + tt) * PATH_CAP);
    }
    h.leaf_kind = LEAF_NONE;
    bool go = !last;
    if constexpr (PC) go = go && (h.active >> 1) >= (uint32_t)T;
    bool forced = true;
    if constexpr (RR != RR_NONE) forced = move_noisy(t, g);
    for (int tt = 0; tt < T; ++tt) {                        // selections in thread order
        group_memory_sync();                                // counters, priors, locks and links written so far are read next
        TreeLine* tl = t.thr + (size_t)g * T + tt;
        ThreadRegs r{0u, LEAF_NONE, 0.0f, 0u, 0u};
        PathRegs pth{0u, 0u};
        uint32_t abandoned = 0u;
        bool want = false;
        typename G::State leaf_s = G::init();
        if (go) {
            leaf_s = select_body<G, true, RR>(t, h, pth, sp, g, sub, t.path + ((size_t)g * T + tt) * PATH_CAP, &abandoned, true, forced);
            want = h.leaf_kind == LEAF_EVAL;
        }
        const uint32_t src = leaf_request<G, MIR>(eb_next, ec, want, leaf_s, sub);      // every wave calls it T times (wave-wide ballots inside)
        if (want) h.src = src;
        r = head_to_thread(h);
        if (last) r.leaf_kind = LEAF_NONE;
        if (sub == 0) {
            ((uint4*)tl)[1] = make_uint4(r.leaf, r.leaf_kind, __float_as_uint(r.leaf_val), r.src);
            tl->head.path_len = r.path_len;
            if (abandoned) tl->head.stat[0] += 1u;
        }
        tl->path16[sub] = pth.lo;
        tl->path16[8 + sub] = pth.hi;
        h.leaf_kind = LEAF_NONE;
    }
    if constexpr (PC) { if (go) h.active -= 2u * (uint32_t)T; }
    if (sub == 0) head_store(t, g, h);
}

// ---- the whole get_action_prob search in ONE launch, for nets that are a pure function of the state on the device ----
// (DumbConnectFourNnet, examples/connect_four.rs:12-43, and the hash fixture): root prepare, then num_sims x {select,
// evaluate in registers, backup} per tree with no kernel boundary and no leaf batch -- the trees never wait for each other.
// Same operations per tree in the same order as the launch-per-step path: bit-identical.
template <class G>
AZ_D float fixture_row(typename G::State s, int kind, uint64_t salt, int sub) {
    float pi[G::ACTIONS], v;
    if (kind == 0) {
#pragma unroll
        for (int a = 0; a < G::ACTIONS; ++a) pi[a] = __fdiv_rn(1.0f, (float)G::ACTIONS);   // examples/connect_four.rs:34-41 (S9)
        v = 1.0f;
    } else {
        hashnet_eval(s.x, s.y, salt, pi, &v);
    }
    float out = v;
#pragma unroll
    for (int a = 0; a < G::ACTIONS; ++a) out = sub == a ? pi[a] : out;
    return out;
}
// PC_BUDGET (playout cap): tree g runs the budget of its own move, t.move.cap.word[g], instead of num_sims
// PC_STOP (the decided-move stop): the budget is the one the tree's stop_word was armed with; an eligible tree takes the decision before every
// selection and leaves with what it skipped in its word, as k_backup_select does
template <class G, bool NZ, int PC, int RR>
__global__ __launch_bounds__(64) void k_search_fixture(TreeDev t, const ulonglong2* root_states, SearchParams sp, int num_sims, int kind,
                                                       uint64_t salt) {
    constexpr int GW = G::GROUP;
    const int tid = blockIdx.x * 64 + threadIdx.x;
    const int g = tid / GW, sub = tid % GW;
    if (g >= t.G) return;
    const EvalBatch no_eb{};
    const EvalCache no_ec{};
    TreeHead h = head_load(t, g);
    PathRegs pth{0u, 0u};
    constexpr bool GZ = RR == RR_GUMBEL;
    bool noisy = true;
    if constexpr (NZ || GZ) noisy = move_noisy(t, g);
    if constexpr (PC == PC_BUDGET) num_sims = (int)(t.move.cap.word[g] & ~PLAYOUT_FULL_BIT);
    bool eligible = false, decided = false;
    if constexpr (PC == PC_STOP) { num_sims = (int)stop_left(h.active); eligible = (h.active & STOP_ELIGIBLE_BIT) != 0u; }
    bool forced = true;
    if constexpr (RR != RR_NONE) forced = move_noisy(t, g);
    typename G::State ls = root_prepare_body<G, NZ, GZ>(t, h, root_states, g, sub, noisy);
    if constexpr (PC == PC_STOP) { if (h.active == 0u) eligible = false; }      // a failed root: the tree is out of this search
    for (int i = 0; i <= num_sims; ++i) {
        group_memory_sync();
        // backup of the previous leaf (i == 0: the root's priors only, S1), then the next selection
        const float pv = (h.leaf_kind == LEAF_EVAL || h.leaf_kind == LEAF_ROOT) ? fixture_row<G>(ls, kind, salt, sub) : 0.0f;
        backup_body<G, true, NZ, false, GZ>(t, h, pth, no_eb, no_ec, g, sub, t.path + (size_t)g * PATH_CAP, pv, noisy);
        if (i == num_sims) break;
        group_memory_sync();
        if constexpr (PC == PC_STOP) {
            if (eligible && stop_root_decided<G>(t, h.root, g, sub, (uint32_t)(num_sims - i))) {
                h.active = stop_word((uint32_t)(num_sims - i), true) | STOP_DECIDED_BIT;
                decided = true;
                break;
            }
        }
        ls = select_body<G, false, RR>(t, h, pth, sp, g, sub, t.path + (size_t)g * PATH_CAP, nullptr, true, forced);
    }
    if constexpr (PC == PC_STOP) { if (h.active != 0u && !decided) h.active = stop_word(0u, eligible); }
    h.leaf_kind = LEAF_NONE;
    if (sub == 0) head_store(t, g, h);
}

template <class G, int RR>
__global__ __launch_bounds__(64) void k_root_policy(TreeDev t, float temp, uint64_t seed, uint64_t first_game_id,
                                                    float* pi, uint16_t* counts, float* q) {
    constexpr int GW = G::GROUP;
    constexpr int NA = G::ACTIONS;
    int tid = blockIdx.x * 64 + threadIdx.x;
    int g = tid / GW, sub = tid % GW;
    if (g >= t.G) return;
    const TreeHead h = head_load(t, g);
    if (!h.active) return;
    const typename G::State s = G::unpack(node_key(t, (size_t)g * t.R, h.root));
    RootPolicy rp = root_policy<G, RR>(t, h.root, g, sub, temp, seed, first_game_id + (uint64_t)g, (uint64_t)G::stones(s));
    if constexpr (RR == RR_GUMBEL) { if (sub == 0) t.move.gumbel.selected[g] = rp.sel; }      // az_tree_get_selected
    if (sub < NA) {
        pi[(size_t)g * NA + sub] = rp.pi;
        if (counts) counts[(size_t)g * NA + sub] = (uint16_t)rp.count;
        if (q) q[(size_t)g * NA + sub] = rp.q;
    }
}

// ---- shared tree batch (az_tree_share) ----------------------------------------------------------------------------------------
// One workgroup: first every slot goes inactive (and loses its reset flag), then -- after the barrier, so the two phases' stores to
// one head never race -- the requested slots are armed.  A batch of any size leaves every other tree exactly as it was.
__global__ __launch_bounds__(1024) void k_slot_arm(TreeDev t, const SlotReq* __restrict__ req, int n, ulonglong2* roots, uint8_t* reset_flags,
                                                   ulonglong2* streams) {
    for (int g = threadIdx.x; g < t.G; g += blockDim.x) {
        t.head[g].head.active = 0u;
        reset_flags[g] = 0;
    }
    if (threadIdx.x < ERR_COUNT) t.err[threadIdx.x] = 0u;
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const SlotReq r = req[i];
        if (r.slot < 0 || r.slot >= t.G) continue;
        t.head[r.slot].head.active = 1u;
        roots[r.slot] = r.state;
        reset_flags[r.slot] = r.reset ? 1 : 0;
        if (streams) streams[r.slot] = make_ulonglong2(r.seed, r.game_id);      // the slot's root-noise stream
    }
}
__global__ void k_noise_streams(ulonglong2* streams, int n, uint64_t seed, uint64_t first_game_id) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g < n) streams[g] = make_ulonglong2(seed, first_game_id + (uint64_t)g);
}
// az_root_noise_eta: the sampler alone, 8 lanes per root exactly as a search runs it (the root's children = its valid moves in ascending
// order); lane a then holds eta[a] (0 for an invalid action)
template <class G>
__global__ __launch_bounds__(64) void k_root_noise_eta(int n, uint64_t seed, const uint64_t* __restrict__ game_ids, const ulonglong2* __restrict__ states,
                                                       float alpha, float* __restrict__ eta_out) {
    constexpr int GW = G::GROUP;
    constexpr int NA = G::ACTIONS;
    const int tid = blockIdx.x * 64 + threadIdx.x;
    const int i = tid / GW, sub = tid % GW;
    if (i >= n) return;
    const typename G::State s = states[i];
    const uint32_t vm = G::valid_mask(s) & ((1u << NA) - 1u), nchild = (uint32_t)__popc(vm);
    const uint32_t myact = (uint32_t)sub < nchild ? nth_set_bit<NA>(vm, (uint32_t)sub) : 0u;
    const float eta = root_noise_eta_lane<G>(noise_stream(seed, game_ids[i], (uint64_t)G::stones(s)), alpha, nchild, myact, sub);
    float mine = 0.0f;
#pragma unroll
    for (int j = 0; j < NA; ++j) {
        const float ej = gshflf<GW>(eta, j);
        const uint32_t aj = gshfl<GW>(myact, j);
        if ((uint32_t)j < nchild && aj == (uint32_t)sub) mine = ej;
    }
    if (sub < NA) eta_out[(size_t)i * NA + sub] = mine;
}

// az_gumbel_values: the variates alone, lane a of a root's 8 lanes holds action a
template <class G>
__global__ __launch_bounds__(64) void k_gumbel_values(int n, uint64_t seed, const uint64_t* __restrict__ game_ids, const ulonglong2* __restrict__ states,
                                                      bool temp_is_zero, float* __restrict__ g_out) {
    constexpr int GW = G::GROUP;
    constexpr int NA = G::ACTIONS;
    const int tid = blockIdx.x * 64 + threadIdx.x;
    const int i = tid / GW, sub = tid % GW;
    if (i >= n || sub >= NA) return;
    const typename G::State s = states[i];
    const bool valid = (G::valid_mask(s) >> sub) & 1u;
    g_out[(size_t)i * NA + sub] = valid ? gumbel_variate(seed, game_ids[i], (uint64_t)G::stones(s), (uint32_t)sub, temp_is_zero) : 0.0f;
}

// k_root_policy per REQUEST: request i's tree is req[i].slot, its temperature and RNG stream are its own, its answer goes to out[i].
// status: a failed root (the search left the tree inactive: arena exhausted at the root) or a terminal root is this request's own
// error; a capacity error raised during the search (t.err) is blamed on every tree of the batch that is that close to full (a tree
// whose push failed always is: node_upgrade refuses exactly when len + 8 > R or count + 8 > reserve could be exceeded).
template <class G, int RR>
__global__ __launch_bounds__(64) void k_slot_root_policy(TreeDev t, const SlotReq* __restrict__ req, int n, SlotOut* out) {
    static_assert(RR != RR_GUMBEL, "never launched with Gumbel on: no such instantiation (AZ_FOR_RR)");
    constexpr int GW = G::GROUP;
    constexpr int NA = G::ACTIONS;
    const int tid = blockIdx.x * 64 + threadIdx.x;
    const int i = tid / GW, sub = tid % GW;
    if (i >= n) return;
    const SlotReq r = req[i];
    if (r.slot < 0 || r.slot >= t.G) return;
    const int g = r.slot;
    const size_t base = (size_t)g * t.R;
    const TreeHead h = head_load(t, g);
    uint32_t status = 0u;
    RootPolicy rp{0.0f, 0u, 0.0f};
    if (!h.active) {
        status = 1u << ERR_CAPACITY;
    } else {
        const uint32_t ecd = (node_load(node_ptr(t, base, h.root)).meta >> META_ECODE_SHIFT) & 3u;
        const bool full_err = (t.err[ERR_CAPACITY] | t.err[ERR_HASH_FULL]) != 0u;
        if (ecd != E_NONE) status = 1u << ERR_TERMINAL_ROOT;
        else if (full_err && (h.len + BLOCK_SLOTS > t.R || h.count + BLOCK_SLOTS > t.reserve_nodes)) status = 1u << ERR_CAPACITY;
        const typename G::State s = G::unpack(node_key(t, base, h.root));
        rp = root_policy<G, RR>(t, h.root, g, sub, r.temp, r.seed, r.game_id, (uint64_t)G::stones(s));
    }
    if (sub < NA) {
        out[i].pi[sub] = rp.pi;
        out[i].q[sub] = rp.q;
        out[i].counts[sub] = (uint16_t)rp.count;
    }
    if (sub == 0) out[i].status = status;
}

// sums the per-tree counters into totals (one atomicAdd per counter per wave) and clears them
__global__ __launch_bounds__(256) void k_harvest(TreeDev t, unsigned long long* totals, uint32_t* node_counts) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    uint32_t st[ST_TOTALS] = {0, 0, 0, 0, 0, 0, 0};
    if (g < t.G) {
        TreeHead* hp = &t.head[g].head;
#pragma unroll
        for (int k = 0; k < ST_COUNT; ++k) { st[k] = hp->stat[k]; hp->stat[k] = 0; }
        if (node_counts) node_counts[g] = hp->count;
        if (t.thr)
            for (int tt = 0; tt < t.T; ++tt) { TreeHead* tp = &t.thr[(size_t)g * t.T + tt].head; st[ST_ABANDONED] += tp->stat[0]; tp->stat[0] = 0; }
    }
#pragma unroll
    for (int k = 0; k < ST_TOTALS; ++k) {
        unsigned long long v = st[k];                 // 64 lanes x < 2^32 each: the sum fits 38 bits
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), off, 64), lo = (uint32_t)__shfl_xor((int)(uint32_t)v, off, 64);
            v += ((unsigned long long)hi << 32) | lo;
        }
        if (lane == 0 && v) atomicAdd(&totals[k], v);
    }
}

__global__ __launch_bounds__(256) void k_call_readback(unsigned long long* totals, unsigned long long* dd_stat, const uint32_t* err,
                                                       CallReadback* out) {
    __shared__ unsigned long long dd[DD_COUNT];
    const int tid = threadIdx.x;
    if (tid < DD_COUNT) dd[tid] = 0;
    __syncthreads();
    if (dd_stat && tid < DD_REPLICAS) {
#pragma unroll
        for (int i = 0; i < DD_COUNT; ++i) {
            const unsigned long long v = dd_stat[tid * DD_STRIDE + i];
            if (v) { atomicAdd(&dd[i], v); dd_stat[tid * DD_STRIDE + i] = 0; }
        }
    }
    __syncthreads();
    if (tid < ST_TOTALS) { out->totals[tid] = totals[tid]; totals[tid] = 0; }
    if (tid < DD_COUNT) out->dd[tid] = dd[tid];
    if (tid < ERR_COUNT) out->err[tid] = err[tid];
}

// ---- Coach::execute_episode, one ply of one slot (src/coach.rs:118-156) -------------------
// Returns 0: the game goes on (gd.state / player / ply advanced); 1: the episode ended and the slot got the next one (its tree must be
// rebuilt: need_reset); 2: the episode ended and the slot stays idle (h.active = 0).
// PC (playout cap): *word = the slot's word for the move being played (az_tree.h PlayoutCap).  The ply's full flag goes into the episode's
// mask (k_emit_samples compacts to the full plies; pi / state / player are stored by ply either way), the mode of the slot's NEXT move -- the
// next ply, or ply 0 of the episode a refilled slot gets -- is drawn, and its word is stored and handed back in *word.
// RR_FORCED (forced playouts): a forced move's pi -- recorded and sampled from -- is formed from the pruned counts when "policy_prune" is on
// RR_GUMBEL: a Gumbel move records the improved policy and PLAYS the selected action; its RNG_MOVE draw is not used (draws are counter-based)
template <class G, bool PC = false, int RR = RR_NONE>
AZ_D int selfplay_move_body(const TreeDev& t, TreeHead& h, const GamesDev& gd, const SelfplayMoveParams& mp, int g, int sub, uint32_t* word = nullptr) {
    constexpr int GW = G::GROUP;
    constexpr int NA = G::ACTIONS;
    const int gi = gd.gid[g];
    const int ply = gd.ply[g];
    const int8_t player = gd.player[g];
    const typename G::State s = gd.state[g];
    const uint64_t game_id = mp.first_game_id + (uint64_t)gi;
    const float temp = (ply + 1 < mp.temp_threshold) ? 1.0f : 0.0f;         // :122-126 (episode_step = ply + 1)
    bool forced = true;
    if constexpr (RR != RR_NONE && PC) forced = (*word & PLAYOUT_FULL_BIT) != 0u;
    RootPolicy rp = root_policy<G, RR>(t, h.root, g, sub, temp, mp.seed, game_id, (uint64_t)ply, forced);   // :128
    const size_t so = (size_t)gi * G::MAX_PLIES + ply;
    if (sub < NA) gd.smp_pi[so * NA + sub] = rp.pi;                         // :130-135 (symmetries regenerated at emit)
    // choose_weighted, :137-138
    float w[NA];
#pragma unroll
    for (int a = 0; a < NA; ++a) w[a] = gshflf<GW>(rp.pi, a);
    float total = 0.0f;
#pragma unroll
    for (int a = 0; a < NA; ++a) total = __fadd_rn(total, w[a]);
    const uint64_t r = rng_draw(mp.seed, game_id, (uint64_t)ply, RNG_MOVE);
    const float uu = (float)(uint32_t)(r >> 40) * (1.0f / 16777216.0f);
    const float target = __fmul_rn(uu, total);
    float acc = 0.0f;
    int action = -1, last = -1;
#pragma unroll
    for (int a = 0; a < NA; ++a) {
        if (w[a] > 0.0f) {
            acc = __fadd_rn(acc, w[a]);
            last = a;
            if (action < 0 && target < acc) action = a;
        }
    }
    if (action < 0) action = last;
    if (action < 0) action = 0;
    if constexpr (RR == RR_GUMBEL) { if (forced) action = rp.sel; }
    const typename G::State s2 = G::play(s, action);                        // :140-142
    const uint32_t ec = G::ended_code(s2);                                  // r = get_game_ended(cur_player), :144
    int status = 0;
    uint32_t next_word = 0u;
    if (sub == 0) {
        if constexpr (PC) { if (*word & PLAYOUT_FULL_BIT) gd.g_full[gi] |= 1ull << ply; }      // one slot owns an episode: a plain read-modify-write
        gd.smp_state[so] = s;
        gd.smp_player[so] = player;
        gd.moves[so] = (uint8_t)action;
        if (ec != E_NONE) {
            // canonical ended(s') = -e: -1 when the side to move has lost, DRAW_EPS on a full board
            gd.g_result[gi] = -ecode_value(ec);
            gd.g_final_player[gi] = (int8_t)-player;
            gd.g_len[gi] = ply + 1;
            if (gd.g_log_len) gd.g_log_len[gi] = (int32_t)h.log_len;
            if (gi >= mp.done_lo && gi < mp.done_hi) atomicAdd(&gd.counters[1], 1u);
            int next = -1;
            if (mp.refill) {
                uint32_t nx = atomicAdd(&gd.counters[0], 1u);
                if (nx < (uint32_t)gd.n_games) next = (int)nx;
            }
            gd.gid[g] = next;
            if (next >= 0) {
                gd.state[g] = G::init();
                gd.player[g] = 1;
                gd.ply[g] = 0;
                gd.need_reset[g] = 1;
                status = 1;
            } else {
                atomicSub(&gd.counters[2], 1u);
                status = 2;
            }
        } else {
            gd.state[g] = s2;
            gd.player[g] = (int8_t)-player;
            gd.ply[g] = ply + 1;
        }
        if constexpr (PC) {
            if (status != 2) {
                next_word = status == 1 ? playout_cap_word(mp.seed, mp.first_game_id + (uint64_t)gd.gid[g], 0ull, t.move.cap.thresh24, t.move.cap.num_sims, t.move.cap.cap_sims)
                                        : playout_cap_word(mp.seed, game_id, (uint64_t)ply + 1ull, t.move.cap.thresh24, t.move.cap.num_sims, t.move.cap.cap_sims);
                t.move.cap.word[g] = next_word;
                atomicMax(&gd.counters[4], next_word & ~PLAYOUT_FULL_BIT);
            }
        }
    }
    status = (int)gshfl<GW>((uint32_t)status, 0);
    if constexpr (PC) *word = gshfl<GW>(next_word, 0);
    if (status == 2) h.active = 0;
    return status;
}
template <class G, bool PC, int RR>
__global__ __launch_bounds__(64) void k_selfplay_move(TreeDev t, GamesDev gd, SelfplayMoveParams mp) {
    constexpr int GW = G::GROUP;
    int tid = blockIdx.x * 64 + threadIdx.x;
    int g = tid / GW, sub = tid % GW;
    if (g >= t.G) return;
    const int gi = gd.gid[g];
    TreeHead h = head_load(t, g);
    if (gi < 0 || !h.active) return;
    uint32_t word = 0u;
    if constexpr (PC) word = t.move.cap.word[g];
    if (selfplay_move_body<G, PC, RR>(t, h, gd, mp, g, sub, &word) == 2 && sub == 0) t.head[g].head.active = 0;
}

// "selfplay_record_search": the root value R (az_target.h) and the root children's stored priors by action of the move k_selfplay_move is
// about to play, into the (episode, ply) slot.  Reads the root record and its child block as root_policy does; writes nothing else.
template <class G>
__global__ __launch_bounds__(64) void k_selfplay_record(TreeDev t, GamesDev gd, SearchRecDev rec) {
    constexpr int GW = G::GROUP;
    constexpr int NA = G::ACTIONS;
    static_assert(NA == TARGET_ACTIONS, "az_target.h's rule is stated for 7 actions");
    const int tid = blockIdx.x * 64 + threadIdx.x;
    const int g = tid / GW, sub = tid % GW;
    if (g >= t.G) return;
    const int gi = gd.gid[g];
    const TreeHead h = head_load(t, g);
    if (gi < 0 || !h.active) return;
    const size_t base = (size_t)g * t.R;
    const NodeRec pr = node_load(node_ptr(t, base, h.root));
    const uint32_t nchild = (pr.meta >> META_NCHILD_SHIFT) & 7u, cb = pr.child_base;
    uint32_t ca = 0, cn = 0;
    float cq = 0.0f, cp = 0.0f;
    if ((uint32_t)sub < nchild) {
        const NodeRec cr = node_load(node_ptr(t, base, cb + sub));
        const uint64_t cc = cr.link != NONE ? node_ctr(node_ptr(t, base, cr.link)) : cr.ctr;
        ca = cr.meta & META_A_MASK;
        cn = ctr_n(cc);
        cq = ctr_q(cc);
        cp = __uint_as_float(cr.prior);
    }
    uint32_t an = 0u;                                                // lane a: action a's count, q and prior (0 for an invalid action)
    float aq = 0.0f, ap = 0.0f;
#pragma unroll
    for (int j = 0; j < NA; ++j) {
        const uint32_t aj = gshfl<GW>(ca, j), nj = gshfl<GW>(cn, j);
        const float qj = gshflf<GW>(cq, j), pj = gshflf<GW>(cp, j);
        if ((uint32_t)j < nchild && aj == (uint32_t)sub) { an = nj; aq = qj; ap = pj; }
    }
    float acc = 0.0f;
    uint32_t N = 0u;
#pragma unroll
    for (int a = 0; a < NA; ++a) target_root_term(acc, N, gshfl<GW>(an, a), gshflf<GW>(aq, a));
    const size_t so = (size_t)gi * G::MAX_PLIES + gd.ply[g];
    if (sub < NA) rec.root_prior[so * NA + sub] = ap;
    if (sub == 0) rec.root_q[so] = target_root_finish(acc, N);
}

// ---- az_reanalyse (include/az_reanalyse.h): the three kernels around the unchanged search ---------------------------
// The check: one thread per position of the whole window.  verdict[RV_FIRST] ends as (index << 7 | verdict bits) of the FIRST position that
// is refused (atomicMin over a word that starts at all ones); the validated state goes to out[i] (an empty board in a refused one's place).
__global__ __launch_bounds__(256) void k_reanalyse_check(const SampleState* __restrict__ states, const float* __restrict__ boards, int64_t n,
                                                         ulonglong2* __restrict__ out, uint32_t* __restrict__ verdict) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint64_t mine, theirs;
    const uint32_t b = reanalyse_check(states, boards, i, &mine, &theirs);
    if (b) atomicMin(&verdict[RV_FIRST], ((uint32_t)i << 7) | b);
    out[i] = b ? make_ulonglong2(0ull, 0ull) : make_ulonglong2(mine, theirs);
}
// The arm: tree g < k takes position off + g -- its root, its reset flag, its active bit and its (seed, game id) stream, which is the root
// noise's and the Gumbel variates' while either is on and the emit's tie-break stream always; the trees of a short last chunk go inactive
// and keep what they hold.
// SS (the decided-move stop is armed: temp == 0): a searching tree's word is the stop_word of an eligible move of stop.num_sims simulations
template <bool SS>
__global__ __launch_bounds__(256) void k_reanalyse_arm(TreeDev t, const ulonglong2* __restrict__ states, const uint64_t* __restrict__ game_ids,
                                                       uint64_t seed, uint64_t first_game_id, int64_t off, int k, ulonglong2* __restrict__ roots,
                                                       ulonglong2* __restrict__ streams, uint8_t* __restrict__ reset_flags) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= t.G) return;
    const bool on = g < k;
    uint32_t word = 1u;
    if constexpr (SS) word = stop_word(t.move.stop.num_sims, stop_eligible(0, t.move.stop.temp_threshold));
    t.head[g].head.active = on ? word : 0u;
    reset_flags[g] = on ? 1 : 0;
    if (!on) return;
    const int64_t i = off + g;
    roots[g] = states[i];
    streams[g] = make_ulonglong2(seed, game_ids ? game_ids[i] : first_game_id + (uint64_t)i);
}
// The emit: k_root_policy's body with the tree's own game id, plus k_selfplay_record's arithmetic on the same finished tree, into row off + g
// of the six outputs (8 lanes per tree, lane a = action a: a wave writes 8 consecutive rows).  A tree the search left inactive (its arena
// ran out at the root) or that stands at its capacity while the search raised a capacity error is blamed: the smallest such position ends
// in verdict[RV_FULL]; the first chunk that sees any error word set leaves its offset in verdict[RV_CHUNK].
template <class G, int RR>
__global__ __launch_bounds__(64) void k_reanalyse_emit(TreeDev t, float temp, const ulonglong2* __restrict__ streams, int64_t off, int k,
                                                       ReanalyseOut out, uint32_t* __restrict__ verdict) {
    constexpr int GW = G::GROUP;
    constexpr int NA = G::ACTIONS;
    static_assert(NA == TARGET_ACTIONS, "az_target.h's rule is stated for 7 actions");
    const int tid = blockIdx.x * 64 + threadIdx.x;
    const int g = tid / GW, sub = tid % GW;
    if (g >= k) return;
    const uint32_t any_err = t.err[ERR_CAPACITY] | t.err[ERR_HASH_FULL] | t.err[ERR_PATH] | t.err[ERR_TERMINAL_ROOT];
    if (g == 0 && sub == 0 && any_err) atomicMin(&verdict[RV_CHUNK], (uint32_t)off);
    const TreeHead h = head_load(t, g);
    const bool full_err = (t.err[ERR_CAPACITY] | t.err[ERR_HASH_FULL]) != 0u;
    if (!h.active || (full_err && (h.len + BLOCK_SLOTS > t.R || h.count + BLOCK_SLOTS > t.reserve_nodes))) {
        if (sub == 0) atomicMin(&verdict[RV_FULL], (uint32_t)(off + g));
        if (!h.active) return;
    }
    const size_t base = (size_t)g * t.R;
    // R and the stored priors, read as k_selfplay_record reads them
    const NodeRec pr = node_load(node_ptr(t, base, h.root));
    const uint32_t nchild = (pr.meta >> META_NCHILD_SHIFT) & 7u, cb = pr.child_base;
    uint32_t ca = 0, cn = 0;
    float cq = 0.0f, cp = 0.0f;
    if ((uint32_t)sub < nchild) {
        const NodeRec cr = node_load(node_ptr(t, base, cb + sub));
        const uint64_t cc = cr.link != NONE ? node_ctr(node_ptr(t, base, cr.link)) : cr.ctr;
        ca = cr.meta & META_A_MASK;
        cn = ctr_n(cc);
        cq = ctr_q(cc);
        cp = __uint_as_float(cr.prior);
    }
    uint32_t an = 0u;
    float aq = 0.0f, ap = 0.0f;
#pragma unroll
    for (int j = 0; j < NA; ++j) {
        const uint32_t aj = gshfl<GW>(ca, j), nj = gshfl<GW>(cn, j);
        const float qj = gshflf<GW>(cq, j), pj = gshflf<GW>(cp, j);
        if ((uint32_t)j < nchild && aj == (uint32_t)sub) { an = nj; aq = qj; ap = pj; }
    }
    float acc = 0.0f;
    uint32_t N = 0u;
#pragma unroll
    for (int a = 0; a < NA; ++a) target_root_term(acc, N, gshfl<GW>(an, a), gshflf<GW>(aq, a));
    // get_action_prob's epilogue on the tree's own stream
    const ulonglong2 st = streams[g];
    const typename G::State s = G::unpack(node_key(t, base, h.root));
    const RootPolicy rp = root_policy<G, RR>(t, h.root, g, sub, temp, st.x, st.y, (uint64_t)G::stones(s));
    const size_t row = (size_t)(off + g);
    if (sub < NA) {
        out.pi[row * NA + sub] = rp.pi;
        if (out.counts) out.counts[row * NA + sub] = (uint16_t)rp.count;
        if (out.q) out.q[row * NA + sub] = rp.q;
        if (out.root_prior) out.root_prior[row * NA + sub] = ap;
    }
    if (sub == 0) {
        if (out.root_q) out.root_q[row] = target_root_finish(acc, N);
        if (out.selected) out.selected[row] = rp.sel;
    }
}

// ---- FREE-RUNNING self-play: every slot on its own timeline ("selfplay_async") -------------------------------------------------------
// The lock-step driver runs one simulation per tree per forward, and every tree waits for the move boundary of all: of 8192 trees only
// ~40 % put a row into a step's batch (the others hit the evaluation cache, a terminal node or a transposition), so the net runs on
// batches of ~2900 rows.  Here a slot advances by itself: one launch takes a tree through backup -> [move, next root] -> select ...
// until its next leaf needs the net (bounded by max_iters), and several launches share one leaf batch: trees whose leaf was answered by
// the cache go on in the NEXT launch (the payload of an entry is only read one launch after its key was seen, as everywhere), trees
// that took a row (or point at another tree's row) stay parked until the forward.  Moves, episode ends and slot refills happen inside the
// kernel; a refilled slot's tree is rebuilt by k_reset_trees between two launches.  Each game still depends on (seed, game id) and the
// net's rows alone -- the schedule decides when a row is evaluated, never what it is.
//   gd.sims[g]   simulations of the current move done so far; -1 = the move's root is not prepared yet
//   first        the first launch behind a forward: eb_prev holds that forward's rows (parked trees back up; its table is cleared)
// PC (playout cap): the slot's move ends at its own budget (the word of az_tree.h PlayoutCap, redrawn by every move), and its root gets the
// noise only when the move is a full one.
template <class G, bool NZ, bool MIR, bool PC, int RR>
__global__ __launch_bounds__(256) void k_async_step(TreeDev t, GamesDev gd, EvalBatch eb_prev, EvalBatch eb_next, EvalCache ec, SearchParams sp,
                                                    SelfplayMoveParams mp, int num_sims, int first, int max_iters) {
    static_assert(RR != RR_GUMBEL, "never launched with Gumbel on: no such instantiation (AZ_FOR_RR)");
    constexpr int GW = G::GROUP;
    const int tid = blockIdx.x * blockDim.x + threadIdx.x;      // whole workgroups only (the launcher pads nothing: leaf_request synchronises)
    const int g = tid / GW, sub = tid % GW;
    if (first) {
        if (tid == 0) { if (eb_prev.max_n && *eb_prev.n > *eb_prev.max_n) *eb_prev.max_n = *eb_prev.n; *eb_prev.n = 0; }
        clear_election_keys(eb_prev);
    }
    if (g >= t.G) return;
    TreeHead h = head_load(t, g);
    PathRegs pth = path_load(t, g, sub);
    uint32_t* path = t.path + (size_t)g * PATH_CAP;
    int sims = gd.sims[g];
    uint32_t word = 0u;                                                        // PC: the word of the slot's current move
    if constexpr (PC) word = t.move.cap.word[g];
    const bool alive = gd.gid[g] >= 0 && h.active != 0 && !gd.need_reset[g];
    // a tree whose leaf waits for a row of the batch being filled stays parked; a leaf answered by the cache (or a value) can go on
    const bool parked = h.leaf_kind != LEAF_NONE && h.leaf_kind != LEAF_VALUE && !(h.src & SRC_CACHE) && !first;
    typename G::State leaf_s = G::init();
    bool want = false;
    if (alive && !parked) {
        for (int it = 0; it < max_iters; ++it) {
            if (h.leaf_kind != LEAF_NONE) {                                    // the pending leaf: store its prior, back its value up
                const bool was_sim = h.leaf_kind != LEAF_ROOT;
                group_memory_sync();
                backup_body<G, false, NZ, MIR>(t, h, pth, eb_prev, ec, g, sub, path, 0.0f, !PC || (word & PLAYOUT_FULL_BIT) != 0u);
                h.leaf_kind = LEAF_NONE;
                if (was_sim) ++sims;
                continue;
            }
            group_memory_sync();
            if (sims < 0) {                                                    // get_action_prob's prologue for the slot's position (S10, S1)
                leaf_s = root_prepare_body<G, NZ>(t, h, gd.state, g, sub, !PC || (word & PLAYOUT_FULL_BIT) != 0u);
                sims = 0;
                if (!h.active) break;                                          // a failed root (error flag set): the call ends with an error
                if (h.leaf_kind == LEAF_ROOT) { want = true; break; }
                continue;
            }
            if (sims >= (PC ? (int)(word & ~PLAYOUT_FULL_BIT) : num_sims)) {      // the move (src/coach.rs:128-156), then the next position's root
                const int st = selfplay_move_body<G, PC, RR>(t, h, gd, mp, g, sub, &word);
                sims = -1;
                if (st != 0) break;                                            // episode over: idle, or wait for k_reset_trees
                continue;
            }
            leaf_s = select_body<G, false, RR>(t, h, pth, sp, g, sub, path, nullptr, true, !PC || (word & PLAYOUT_FULL_BIT) != 0u);
            if (h.leaf_kind == LEAF_EVAL) { want = true; break; }
            if (h.leaf_kind == LEAF_NONE) ++sims;                              // an error cut the simulation short (flag set): it still counts
        }
    }
    const uint32_t src = leaf_request<G, MIR>(eb_next, ec, want, leaf_s, sub);
    if (want) h.src = src;
    if (sub == 0) { head_store(t, g, h); gd.sims[g] = sims; }
    path_store(t, g, sub, pth);
}

// ---- training tuples (TrainingSample, src/nnet.rs:22-27; z per B4, src/coach.rs:146-154) -----
template <class G>
__global__ __launch_bounds__(256) void k_emit_samples(GamesDev gd, const int64_t* offsets, int symmetries,
                                                      ulonglong2* out_states, float* out_boards, float* out_pis,
                                                      float* out_zs) {
    constexpr int NA = G::ACTIONS;
    constexpr int NF = G::FEATURES;
    static_assert(NF > NA + 1, "the item loop below spreads pi / z / state stores over the first feature indices");
    const int gi = blockIdx.x;
    int len = gd.g_len[gi];
    const int nsym = symmetries ? 2 : 1;
    // playout cap: only the full plies are tuples.  s_ply[k] = the k-th full ply; `len` becomes their number (offsets[] counts them too)
    __shared__ uint8_t s_ply[G::MAX_PLIES];
    const bool compact = gd.g_full != nullptr;
    if (compact) {
        const unsigned long long fm = gd.g_full[gi] & ((1ull << len) - 1ull);
        const int p = (int)threadIdx.x;
        if (p < len && ((fm >> p) & 1ull)) s_ply[__popcll(fm & ((1ull << p) - 1ull))] = (uint8_t)p;
        __syncthreads();
        len = __popcll(fm);
    }
    const float r = gd.g_result[gi];
    const int8_t fin = gd.g_final_player[gi];
    for (int item = threadIdx.x; item < len * nsym * NF; item += blockDim.x) {
        const int f = item % NF, rest = item / NF;
        const int sym = rest % nsym, k = rest / nsym;
        const int ply = compact ? (int)s_ply[k] : k;
        const size_t so = (size_t)gi * G::MAX_PLIES + ply;
        const int64_t o = (offsets[gi] + k) * nsym + sym;
        typename G::State s = gd.smp_state[so];
        if (sym) s = G::mirror(s);                                             // get_symmetries, connect_four_game.rs:205-211
        if (out_boards) out_boards[o * NF + f] = G::feature(s, f);
        if (f < NA) out_pis[o * NA + f] = gd.smp_pi[so * NA + (sym ? G::mirror_action(f) : f)];
        if (f == NA) out_zs[o] = __fmul_rn(r, gd.smp_player[so] == fin ? 1.0f : -1.0f);   // B4
        if (f == NA + 1 && out_states) out_states[o] = s;
    }
}

// k_emit_samples' sibling for the search record: the same rows in the same order
template <class G>
__global__ __launch_bounds__(256) void k_emit_search(GamesDev gd, SearchRecDev rec, const int64_t* offsets, int symmetries, float* out_q, float* out_prior) {
    constexpr int NA = G::ACTIONS;
    const int gi = blockIdx.x;
    int len = gd.g_len[gi];
    const int nsym = symmetries ? 2 : 1;
    __shared__ uint8_t s_ply[G::MAX_PLIES];
    const bool compact = gd.g_full != nullptr;
    if (compact) {
        const unsigned long long fm = gd.g_full[gi] & ((1ull << len) - 1ull);
        const int p = (int)threadIdx.x;
        if (p < len && ((fm >> p) & 1ull)) s_ply[__popcll(fm & ((1ull << p) - 1ull))] = (uint8_t)p;
        __syncthreads();
        len = __popcll(fm);
    }
    for (int item = threadIdx.x; item < len * nsym * (NA + 1); item += blockDim.x) {
        const int f = item % (NA + 1), rest = item / (NA + 1);
        const int sym = rest % nsym, k = rest / nsym;
        const int ply = compact ? (int)s_ply[k] : k;
        const size_t so = (size_t)gi * G::MAX_PLIES + ply;
        const int64_t o = (offsets[gi] + k) * nsym + sym;
        if (f < NA) { if (out_prior) out_prior[o * NA + f] = rec.root_prior[so * NA + (sym ? G::mirror_action(f) : f)]; }
        else if (out_q) out_q[o] = rec.root_q[so];
    }
}

// ---- paired arena openings: one lane per game grows its pair's opening (az_opening.h) and writes the game's start position ----
template <class G>
__global__ __launch_bounds__(256) void k_arena_openings(ArenaDev ad, ArenaOpenings op) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= ad.G) return;
    const uint64_t pair = ad.half > 0 ? (uint64_t)(ad.first + g) % (uint64_t)ad.half : (uint64_t)(ad.first + g);   // (a one-game total has no twin)
    const ulonglong2 base = op.nb > 0 ? op.book[opening_book_index(pair, (uint32_t)op.nb)] : op.base;
    uint8_t mv[OPENING_MAX_PLIES];
#pragma unroll
    for (int j = 0; j < OPENING_MAX_PLIES; ++j) mv[j] = 0;
    typename G::State out;
    const int len = opening_grow<G>(base, op.seed, pair, op.plies, &out, mv);
    ad.state[g] = out;
    op.len[g] = len;
    for (int j = 0; j < OPENING_MAX_PLIES; ++j) op.moves[(size_t)g * OPENING_MAX_PLIES + j] = mv[j];
}

// ---- arena::play_game, one ply for every running game (src/arena.rs:18-41) ------------------------
// The searching tree's owner plays argmax(get_action_prob(s, temp = 0)) (src/coach.rs:356-372): the rule of one ply of one game, for az_arena
// and az_tournament alike (tree g of a model's batch plays game gi through the model's table; in the arena gi == g).
//   g     the tree of t that searched           gi    the game's row in ad (state, player, alive, results, moves, len)
//   rid   the game's index in the tie-break stream (seed, rid, ply): the arena's global game index, the index inside the pair
template <class G>
__device__ __forceinline__ void arena_move_body(const TreeDev& t, const TreeHead& h, const ArenaDev& ad, int g, int gi, uint64_t rid, int sub,
                                                uint64_t seed) {
    constexpr int GW = G::GROUP;
    constexpr int NA = G::ACTIONS;
    const typename G::State s = ad.state[gi];
    const int8_t player = ad.player[gi];
    RootPolicy rp = root_policy<G>(t, h.root, g, sub, 0.0f, seed, rid, (uint64_t)G::stones(s));
    // argmax with max_by (last max) over the one-hot pi = the index of the 1
    const uint32_t hot = gballot<GW>(sub < NA && rp.pi == 1.0f) & ((1u << NA) - 1u);
    const int action = hot ? (31 - __clz((int)hot)) : 0;
    const bool valid = (G::valid_mask(s) >> action) & 1u;             // src/arena.rs:29-35
    const typename G::State s2 = G::play(s, action);
    const uint32_t ec = G::ended_code(s2);
    if (sub == 0) {
        if (valid && hot) {                           // the game's move record
            const int32_t k = ad.len[gi];
            if (k < G::MAX_PLIES) ad.moves[(size_t)gi * G::MAX_PLIES + k] = (uint8_t)action;
            ad.len[gi] = k + 1;
        }
        if (!valid || !hot) {
            atomicOr(&ad.counters[1], 1u);
            ad.alive[gi] = 0;
            atomicSub(&ad.counters[0], 1u);
        } else if (ec != E_NONE) {
            // cur_player' = -player; result = cur_player' * round(get_game_ended(cur_player')) (src/arena.rs:51):
            // ended = -1 -> the player who just moved won; DRAW_EPS rounds to 0
            ad.results[gi] = (ec == E_PLUS1) ? player : (ec == E_MINUS1 ? (int8_t)-player : (int8_t)0);
            ad.alive[gi] = 0;
            atomicSub(&ad.counters[0], 1u);
        } else {
            ad.state[gi] = s2;
            ad.player[gi] = (int8_t)-player;
        }
    }
}

// ---- az_arena and az_tournament: the games of all pairs in one ArenaDev (game p * n + g; the arena is the one pair), one tree batch per MODEL
// Tree g of a model's batch plays the game its table names (MatchTable, az_tree.h).  Which model moves: seat 0 moves when cur_player == +1;
// the games of a pair below ad.half seat (first listed, second listed), the rest the other way round.  The tree searches this ply when its
// game is running and its model is to move, and its root state is gathered from the per-game array.
// SS (the decided-move stop): a searching tree's word is the stop_word of an eligible move of stop.num_sims simulations (every move of a
// match is played at temperature 0)
template <bool SS>
__global__ void k_match_sync(TreeDev t, ArenaDev ad, MatchTable tb) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= t.G) return;
    const uint32_t w = tb.game[g];
    const int gi = (int)(w & MATCH_GAME_MASK);
    if (gi >= ad.G) { t.head[g].head.active = 0u; return; }            // (a table entry outside the games: never built, never followed)
    const int second = (int)(w >> 31);                                  // 0: this model is the pair's first listed ("new"), 1: its second ("old")
    const int first_model = ad.first + gi % tb.n < ad.half ? 0 : 1;     // the seating uses the arena's global index, the index inside the pair
    const int mover = ad.player[gi] == 1 ? first_model : 1 - first_model;
    uint32_t word = 1u;
    if constexpr (SS) word = stop_word(t.move.stop.num_sims, true);
    t.head[g].head.active = (ad.alive[gi] != 0 && mover == second) ? word : 0u;
    tb.roots[g] = ad.state[gi];
}

template <class G>
__global__ __launch_bounds__(64) void k_match_move(TreeDev t, ArenaDev ad, MatchTable tb, uint64_t seed) {
    constexpr int GW = G::GROUP;
    int tid = blockIdx.x * 64 + threadIdx.x;
    int g = tid / GW, sub = tid % GW;
    if (g >= t.G) return;
    const TreeHead h = head_load(t, g);
    if (!h.active) return;
    const int gi = (int)(tb.game[g] & MATCH_GAME_MASK);
    if (gi >= ad.G) return;
    arena_move_body<G>(t, h, ad, g, gi, (uint64_t)(ad.first + gi % tb.n), sub, seed);
}

// SS (the decided-move stop): the slot's word is the stop_word of its move -- the budget is the cap's own or stop.num_sims, the move is
// eligible by selfplay_move_body's temperature test on the slot's ply
template <bool SS>
__global__ void k_sync_active(TreeDev t, GamesDev gd) {
    int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= t.G) return;
    uint32_t a = gd.gid[g] >= 0 ? 1u : 0u;
    if constexpr (SS) {
        if (a) a = stop_word(t.move.cap.word ? (t.move.cap.word[g] & ~PLAYOUT_FULL_BIT) : t.move.stop.num_sims, stop_eligible(gd.ply[g], t.move.stop.temp_threshold));
    } else {
        if (a && t.move.cap.word) a |= (t.move.cap.word[g] & ~PLAYOUT_FULL_BIT) << 1;      // playout cap: the simulations the slot's move has left
    }
    t.head[g].head.active = a;
}

// ---- the decided-move stop's counters (az_stop.h StopStat): one thread per tree, where the move is played or emitted.  A tree that searched
// an eligible move adds the move, its budget and -- when it was decided -- the stop and what its word has left; one atomic per counter and wave.
__global__ __launch_bounds__(256) void k_stop_count(TreeDev t, const int32_t* __restrict__ gid) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    unsigned long long v[SS_COUNT] = {0ull, 0ull, 0ull, 0ull};
    if (g < t.G && (!gid || gid[g] >= 0)) {
        const uint32_t w = t.head[g].head.active;
        if ((w & 1u) && (w & STOP_ELIGIBLE_BIT)) {
            const bool decided = (w & STOP_DECIDED_BIT) != 0u;
            v[SS_ELIGIBLE] = 1ull;
            v[SS_STOPPED] = decided ? 1ull : 0ull;
            v[SS_BUDGET] = t.move.cap.word ? (t.move.cap.word[g] & ~PLAYOUT_FULL_BIT) : t.move.stop.num_sims;
            v[SS_SKIPPED] = decided ? stop_left(w) : 0u;
        }
    }
#pragma unroll
    for (int k = 0; k < SS_COUNT; ++k) {
        uint32_t x = (uint32_t)v[k];                  // 64 lanes x < 2^30 each: the wave's sum is taken in 64 bits
        unsigned long long sum = x;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(sum >> 32), off, 64), lo = (uint32_t)__shfl_xor((int)(uint32_t)sum, off, 64);
            sum += ((unsigned long long)hi << 32) | lo;
        }
        if ((threadIdx.x & 63) == 0 && sum) atomicAdd(&t.move.stop.stat[k], sum);
    }
}

// ---- launchers: one instantiation of every kernel per Game policy, chosen by TreeDev.game ------------------------------
template <class G> constexpr bool game_ok() {
    return G::GROUP == BLOCK_SLOTS && G::GROUP > G::ACTIONS && (G::GROUP & (G::GROUP - 1)) == 0 && sizeof(typename G::State) == 16 &&
           sizeof(typename G::Packed) == 8;
}
static_assert(game_ok<ConnectFour>() && game_ok<ConnectThree>(),
              "one lane per child plus one, power of two, one child block per group; 16-byte states, 8-byte node-resident identity");
#define AZ_FOR_GAME(game_, ...)                                    \
    do {                                                           \
        if ((game_) == 1) { using TG = ConnectThree; __VA_ARGS__; } \
        else { using TG = ConnectFour; __VA_ARGS__; }               \
    } while (0)
// ... and per root-noise setting: NZ = true only when the tree batch carries a non-zero eps
#define AZ_FOR_GAME_NZ(t_, ...)                                                          \
    do {                                                                                 \
        if ((t_).move.noise.eps != 0.0f) { constexpr bool NZ = true; AZ_FOR_GAME((t_).game, __VA_ARGS__); } \
        else { constexpr bool NZ = false; AZ_FOR_GAME((t_).game, __VA_ARGS__); }         \
    } while (0)
// ... and per "eval_mirror" setting of the leaf batch the launch requests into / backs up from (both batches of a search carry the same)
#define AZ_FOR_GAME_NZ_MIR(t_, eb_, ...)                                                 \
    do {                                                                                 \
        if ((eb_).mirror) { constexpr bool MIR = true; AZ_FOR_GAME_NZ(t_, __VA_ARGS__); } \
        else { constexpr bool MIR = false; AZ_FOR_GAME_NZ(t_, __VA_ARGS__); }            \
    } while (0)
// ... and per playout cap: PC = true only for the searches of a self-play session that has one
#define AZ_FOR_PC(t_, ...)                                                               \
    do {                                                                                 \
        if ((t_).move.cap.word) { constexpr bool PC = true; __VA_ARGS__; }                    \
        else { constexpr bool PC = false; __VA_ARGS__; }                                 \
    } while (0)
// ... and per countdown (k_backup_select, k_search_fixture): the decided-move stop while the entry point's record has stop.on, else as AZ_FOR_PC
#define AZ_FOR_PCX(t_, ...)                                                              \
    do {                                                                                 \
        if ((t_).move.stop.on) { constexpr int PC = PC_STOP; __VA_ARGS__; }              \
        else if ((t_).move.cap.word) { constexpr int PC = PC_BUDGET; __VA_ARGS__; }      \
        else { constexpr int PC = PC_NONE; __VA_ARGS__; }                                \
    } while (0)
#define AZ_FOR_SS(t_, ...)                                                               \
    do {                                                                                 \
        if ((t_).move.stop.on) { constexpr bool SS = true; __VA_ARGS__; }                \
        else { constexpr bool SS = false; __VA_ARGS__; }                                 \
    } while (0)
// ... and per root rule: Gumbel while the entry point's record has gumbel.m != 0, else forced playouts while forced.k != 0 (the two exclude
// each other), else today's kernels.  GZ = the baseline capture of a Gumbel move in the kernels that carry no selection; FP = the rule of
// k_step_mt / k_async_step / k_slot_root_policy, which are never launched with Gumbel on (refused for T > 1 and selfplay_async, zero for
// the slot calls): they take RR_OF_FP, so RR_GUMBEL resolves to their RR_NONE instantiation and no RR_GUMBEL one exists.
#define AZ_FOR_RR(t_, ...)                                                                    \
    do {                                                                                      \
        if ((t_).move.gumbel.m != 0u) { AZ_WITH_RR(RR_GUMBEL, __VA_ARGS__); }                 \
        else if ((t_).move.forced.k != 0.0f) { AZ_WITH_RR(RR_FORCED, __VA_ARGS__); }          \
        else { AZ_WITH_RR(RR_NONE, __VA_ARGS__); }                                            \
    } while (0)
#define AZ_WITH_RR(rr_, ...)                                                                  \
    constexpr int RR = rr_; constexpr bool GZ = RR == RR_GUMBEL, FP = RR == RR_FORCED;        \
    (void)RR; (void)GZ; (void)FP;                                                             \
    __VA_ARGS__
#define RR_OF_FP (FP ? RR_FORCED : RR_NONE)
// the decided-move stop is stated for the PUCT root (its entries refuse forced playouts and Gumbel): no PC_STOP instantiation carries another rule
#define RR_OF_PC (PC == PC_STOP ? RR_NONE : RR)
static inline int group_blocks(int G) { return (G * BLOCK_SLOTS + 63) / 64; }
#ifdef AZ_DIAG
// diagnostic library only: the PUCT term of best_child (src/node.rs:352-356) for n (child counter, prior bits, parent N) triples, as the
// selection kernels compute it -- lets a test hold every operation of it to the oracle's IEEE arithmetic, bit for bit
__global__ void k_diag_puct(const unsigned long long* ctr, const uint32_t* prior, const uint32_t* parent_n, float cpuct, float* out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = puct(ctr[i], __uint_as_float(prior[i]), puct_sqrt_parent(parent_n[i]), cpuct);
}
extern "C" int az_diag_puct(const unsigned long long* ctr, const uint32_t* prior, const uint32_t* parent_n, int cpuct, float* out, int n) {
    unsigned long long* d_c = nullptr; uint32_t *d_p = nullptr, *d_n = nullptr; float* d_o = nullptr;
    bool ok = hipMalloc((void**)&d_c, (size_t)n * 8) == hipSuccess && hipMalloc((void**)&d_p, (size_t)n * 4) == hipSuccess &&
              hipMalloc((void**)&d_n, (size_t)n * 4) == hipSuccess && hipMalloc((void**)&d_o, (size_t)n * 4) == hipSuccess;
    ok = ok && hipMemcpy(d_c, ctr, (size_t)n * 8, hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(d_p, prior, (size_t)n * 4, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(d_n, parent_n, (size_t)n * 4, hipMemcpyHostToDevice) == hipSuccess;
    if (ok) {
        hipLaunchKernelGGL(k_diag_puct, dim3((n + 255) / 256), dim3(256), 0, nullptr, d_c, d_p, d_n, (float)cpuct, d_o, n);
        ok = hipMemcpy(out, d_o, (size_t)n * 4, hipMemcpyDeviceToHost) == hipSuccess;
    }
    (void)hipFree(d_c); (void)hipFree(d_p); (void)hipFree(d_n); (void)hipFree(d_o);
    return ok ? 0 : -1;
}
// diagnostic library only: per-wave phase stamps of k_backup_select (tools/tree_probe.py); process-wide by design (a probe, not a product path)
constexpr int TREE_DBG_WAVES = 4096;
static unsigned long long* g_tree_dbg = nullptr;
bool tree_set_stamps(int on) {
    if (on && !g_tree_dbg) return hipMalloc((void**)&g_tree_dbg, (size_t)TREE_DBG_WAVES * 8 * sizeof(unsigned long long)) == hipSuccess &&
                                  hipMemset(g_tree_dbg, 0, (size_t)TREE_DBG_WAVES * 8 * sizeof(unsigned long long)) == hipSuccess;
    if (!on && g_tree_dbg) { (void)hipFree(g_tree_dbg); g_tree_dbg = nullptr; }
    return true;
}
bool tree_read_stamps(unsigned long long* out /*[TREE_DBG_WAVES * 8]*/) {
    return g_tree_dbg && hipMemcpy(out, g_tree_dbg, (size_t)TREE_DBG_WAVES * 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost) == hipSuccess;
}
#endif

void launch_init_heads(const TreeDev& t, hipStream_t s) {
    hipLaunchKernelGGL(k_init_heads, dim3((t.G + 255) / 256), dim3(256), 0, s, t);
}
void launch_set_active(const TreeDev& t, uint32_t value, hipStream_t s) {
    hipLaunchKernelGGL(k_set_active, dim3((t.G + 255) / 256), dim3(256), 0, s, t, value);
}
void launch_reset_trees(const TreeDev& t, const uint8_t* flags, hipStream_t s, const ulonglong2* roots) {
    AZ_FOR_GAME(t.game, hipLaunchKernelGGL(k_reset_trees<TG>, dim3(t.G), dim3(256), 0, s, t, flags, const_cast<uint8_t*>(flags), roots));
}
void launch_root_prepare(const TreeDev& t, const EvalBatch& eb, const EvalCache& ec, const ulonglong2* root_states, hipStream_t s) {
    AZ_FOR_RR(t, AZ_FOR_GAME_NZ_MIR(t, eb, hipLaunchKernelGGL((k_root_prepare<TG, NZ, MIR, GZ>), dim3(group_blocks(t.G)), dim3(64), 0, s, t, eb, ec, root_states)));
}
void launch_backup(const TreeDev& t, const EvalBatch& eb, const EvalCache& ec, hipStream_t s) {
    AZ_FOR_RR(t, AZ_FOR_GAME_NZ_MIR(t, eb, hipLaunchKernelGGL((k_backup<TG, NZ, MIR, GZ>), dim3(group_blocks(t.G)), dim3(64), 0, s, t, eb, ec)));
}
void launch_backup_select(const TreeDev& t, const EvalBatch& eb_prev, const EvalBatch& eb_next, const EvalCache& ec, SearchParams sp,
                          hipStream_t s) {
    const bool four = t.block4 && (t.G * 8) % 256 == 0;     // whole 4-wave workgroups: one row-counter atomic per workgroup (leaf_request)
    const dim3 grid(four ? (unsigned)(t.G * 8 / 256) : group_blocks(t.G)), block(four ? 256 : 64);
#ifdef AZ_DIAG
    if (g_tree_dbg && t.G * 8 / 64 <= TREE_DBG_WAVES) {
        AZ_FOR_RR(t, AZ_FOR_PCX(t, AZ_FOR_GAME_NZ_MIR(t, eb_next, hipLaunchKernelGGL((k_backup_select<TG, true, NZ, MIR, PC, RR_OF_PC>), grid, block, 0, s, t, eb_prev, eb_next, ec, sp, g_tree_dbg))));
        return;
    }
#endif
    AZ_FOR_RR(t, AZ_FOR_PCX(t, AZ_FOR_GAME_NZ_MIR(t, eb_next, hipLaunchKernelGGL((k_backup_select<TG, false, NZ, MIR, PC, RR_OF_PC>), grid, block, 0, s, t, eb_prev, eb_next, ec, sp, nullptr))));
}
void launch_step_mt(const TreeDev& t, const EvalBatch& eb_prev, const EvalBatch& eb_next, const EvalCache& ec, SearchParams sp,
                    int first, int last, hipStream_t s) {
    // one wave per workgroup: leaf_request is called T times per launch and its one-atomic-per-workgroup path keeps state in LDS
    AZ_FOR_RR(t, AZ_FOR_PC(t, AZ_FOR_GAME_NZ_MIR(t, eb_next, hipLaunchKernelGGL((k_step_mt<TG, NZ, MIR, PC, RR_OF_FP>), dim3(group_blocks(t.G)), dim3(64), 0, s, t, eb_prev, eb_next, ec, sp, first, last))));
}
void launch_search_fixture(const TreeDev& t, const ulonglong2* root_states, SearchParams sp, int num_sims, int kind, uint64_t salt,
                           hipStream_t s) {
    AZ_FOR_RR(t, AZ_FOR_PCX(t, AZ_FOR_GAME_NZ(t, hipLaunchKernelGGL((k_search_fixture<TG, NZ, PC, RR_OF_PC>), dim3(group_blocks(t.G)), dim3(64), 0, s, t, root_states, sp, num_sims, kind, salt))));
}
void launch_root_policy(const TreeDev& t, float temp, uint64_t seed, uint64_t first_game_id, float* pi,
                        uint16_t* counts, float* q, hipStream_t s) {
    AZ_FOR_RR(t, AZ_FOR_GAME(t.game, hipLaunchKernelGGL((k_root_policy<TG, RR>), dim3(group_blocks(t.G)), dim3(64), 0, s, t, temp, seed, first_game_id, pi, counts, q)));
}
void launch_slot_arm(const TreeDev& t, const SlotReq* req, int n, ulonglong2* roots, uint8_t* reset_flags, hipStream_t s, ulonglong2* streams) {
    hipLaunchKernelGGL(k_slot_arm, dim3(1), dim3(1024), 0, s, t, req, n, roots, reset_flags, streams);
}
void launch_noise_streams(ulonglong2* streams, int n, uint64_t seed, uint64_t first_game_id, hipStream_t s) {
    hipLaunchKernelGGL(k_noise_streams, dim3((n + 255) / 256), dim3(256), 0, s, streams, n, seed, first_game_id);
}
void launch_root_noise_eta(int game, int n, uint64_t seed, const uint64_t* game_ids, const ulonglong2* states, float alpha, float* eta_out, hipStream_t s) {
    if (n <= 0) return;
    AZ_FOR_GAME(game, hipLaunchKernelGGL(k_root_noise_eta<TG>, dim3(group_blocks(n)), dim3(64), 0, s, n, seed, game_ids, states, alpha, eta_out));
}
void launch_gumbel_values(int game, int n, uint64_t seed, const uint64_t* game_ids, const ulonglong2* states, bool temp_is_zero, float* g_out, hipStream_t s) {
    if (n <= 0) return;
    AZ_FOR_GAME(game, hipLaunchKernelGGL(k_gumbel_values<TG>, dim3(group_blocks(n)), dim3(64), 0, s, n, seed, game_ids, states, temp_is_zero, g_out));
}
void launch_slot_root_policy(const TreeDev& t, const SlotReq* req, int n, SlotOut* out, hipStream_t s) {
    if (n <= 0) return;
    AZ_FOR_RR(t, AZ_FOR_GAME(t.game, hipLaunchKernelGGL((k_slot_root_policy<TG, RR_OF_FP>), dim3(group_blocks(n)), dim3(64), 0, s, t, req, n, out)));
}
void launch_harvest(const TreeDev& t, unsigned long long* totals, uint32_t* node_counts, hipStream_t s) {
    hipLaunchKernelGGL(k_harvest, dim3((t.G + 255) / 256), dim3(256), 0, s, t, totals, node_counts);
}
void launch_call_readback(unsigned long long* totals, unsigned long long* dd_stat, const uint32_t* err, CallReadback* out, hipStream_t s) {
    static_assert(DD_REPLICAS <= 256, "one thread per replica");
    hipLaunchKernelGGL(k_call_readback, dim3(1), dim3(256), 0, s, totals, dd_stat, err, out);
}
void launch_selfplay_move(const TreeDev& t, const GamesDev& gd, SelfplayMoveParams mp, hipStream_t s) {
    AZ_FOR_RR(t, AZ_FOR_PC(t, AZ_FOR_GAME(t.game, hipLaunchKernelGGL((k_selfplay_move<TG, PC, RR>), dim3(group_blocks(t.G)), dim3(64), 0, s, t, gd, mp))));
}
void launch_selfplay_record(const TreeDev& t, const GamesDev& gd, const SearchRecDev& rec, hipStream_t s) {
    AZ_FOR_GAME(t.game, hipLaunchKernelGGL(k_selfplay_record<TG>, dim3(group_blocks(t.G)), dim3(64), 0, s, t, gd, rec));
}
void launch_reanalyse_check(const SampleState* states, const float* boards, int64_t n, ulonglong2* out, uint32_t* verdict, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_reanalyse_check, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, states, boards, n, out, verdict);
}
void launch_reanalyse_arm(const TreeDev& t, const ulonglong2* states, const uint64_t* game_ids, uint64_t seed, uint64_t first_game_id, int64_t off,
                          int k, ulonglong2* roots, ulonglong2* streams, uint8_t* reset_flags, hipStream_t s) {
    AZ_FOR_SS(t, hipLaunchKernelGGL(k_reanalyse_arm<SS>, dim3((t.G + 255) / 256), dim3(256), 0, s, t, states, game_ids, seed, first_game_id, off, k, roots,
                                    streams, reset_flags));
}
void launch_reanalyse_emit(const TreeDev& t, float temp, const ulonglong2* streams, int64_t off, int k, const ReanalyseOut& out, uint32_t* verdict,
                           hipStream_t s) {
    if (k <= 0) return;
    AZ_FOR_RR(t, AZ_FOR_GAME(t.game, hipLaunchKernelGGL((k_reanalyse_emit<TG, RR>), dim3(group_blocks(k)), dim3(64), 0, s, t, temp, streams, off, k, out, verdict)));
}
void launch_async_step(const TreeDev& t, const GamesDev& gd, const EvalBatch& eb_prev, const EvalBatch& eb_next, const EvalCache& ec, SearchParams sp,
                       SelfplayMoveParams mp, int num_sims, int first, int max_iters, hipStream_t s) {
    const bool four = t.block4 && (t.G * 8) % 256 == 0;
    const dim3 grid(four ? (unsigned)(t.G * 8 / 256) : group_blocks(t.G)), block(four ? 256 : 64);
    AZ_FOR_RR(t, AZ_FOR_PC(t, AZ_FOR_GAME_NZ_MIR(t, eb_next, hipLaunchKernelGGL((k_async_step<TG, NZ, MIR, PC, RR_OF_FP>), grid, block, 0, s, t, gd, eb_prev, eb_next, ec, sp, mp, num_sims, first, max_iters))));
}
void launch_selfplay_sync_active(const TreeDev& t, const GamesDev& gd, hipStream_t s) {
    AZ_FOR_SS(t, hipLaunchKernelGGL(k_sync_active<SS>, dim3((t.G + 255) / 256), dim3(256), 0, s, t, gd));
}
void launch_stop_count(const TreeDev& t, const int32_t* gid, hipStream_t s) {
    if (!t.move.stop.on) return;
    hipLaunchKernelGGL(k_stop_count, dim3((t.G + 255) / 256), dim3(256), 0, s, t, gid);
}
static_assert(OPENING_E_NONE == E_NONE && OPENING_E_PLUS1 == E_PLUS1, "az_opening.h restates the ecodes of az_common.h");
void launch_arena_openings(int game, const ArenaDev& ad, const ArenaOpenings& op, hipStream_t s) {
    AZ_FOR_GAME(game, hipLaunchKernelGGL(k_arena_openings<TG>, dim3((ad.G + 255) / 256), dim3(256), 0, s, ad, op));
}
void launch_match_sync(const TreeDev& t, const ArenaDev& ad, const MatchTable& tb, hipStream_t s) {
    AZ_FOR_SS(t, hipLaunchKernelGGL(k_match_sync<SS>, dim3((t.G + 255) / 256), dim3(256), 0, s, t, ad, tb));
}
void launch_match_move(const TreeDev& t, const ArenaDev& ad, const MatchTable& tb, uint64_t seed, hipStream_t s) {
    AZ_FOR_GAME(t.game, hipLaunchKernelGGL(k_match_move<TG>, dim3(group_blocks(t.G)), dim3(64), 0, s, t, ad, tb, seed));
}
// episodes of [lo, hi) that have already finished (g_len is set when an episode ends): a session's chunk starts its count from here
__global__ void k_count_done(const int32_t* __restrict__ g_len, int lo, int hi, uint32_t* __restrict__ counter) {
    __shared__ uint32_t part[256];
    uint32_t n = 0;
    for (int i = lo + (int)threadIdx.x; i < hi; i += 256) n += g_len[i] > 0 ? 1u : 0u;
    part[threadIdx.x] = n;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) part[threadIdx.x] += part[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) *counter = part[0];
}
void launch_count_done(const int32_t* g_len, int lo, int hi, uint32_t* counter, hipStream_t s) {
    hipLaunchKernelGGL(k_count_done, dim3(1), dim3(256), 0, s, g_len, lo, hi, counter);
}
void launch_emit_samples(const GamesDev& gd, const int64_t* offsets, int symmetries, ulonglong2* out_states,
                         float* out_boards, float* out_pis, float* out_zs, hipStream_t s) {
    // features, mirror and plies are the board's, not the rules': both games share ConnectFour's
    hipLaunchKernelGGL(k_emit_samples<ConnectFour>, dim3(gd.n_games), dim3(256), 0, s, gd, offsets, symmetries, out_states,
                       out_boards, out_pis, out_zs);
}
void launch_emit_search(const GamesDev& gd, const SearchRecDev& rec, const int64_t* offsets, int symmetries, float* out_q, float* out_prior,
                        hipStream_t s) {
    hipLaunchKernelGGL(k_emit_search<ConnectFour>, dim3(gd.n_games), dim3(256), 0, s, gd, rec, offsets, symmetries, out_q, out_prior);
}

}  // namespace az
