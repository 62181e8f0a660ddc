// az_engine.hip -- C-ABI implementation (include/az_engine.h): host orchestration of the
// tree kernels (az_tree.hip) and the nets (az_net.hip) on one HIP stream.
//
// There is NO CPU fallback: every entry point runs the HIP kernels or fails with a status.
#include "../../include/az_engine.h"
#include "../../include/az_reanalyse.h"
#include "../../include/az_search_stop.h"

#include <dlfcn.h>
#include <unistd.h>
#include <rccl/rccl.h>      // types only: the library is dlopen'ed by az_comm_* (a host that never shards never loads it)

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "az_combine.h"
#include "az_draw.h"
#include "az_local_comm.h"
#include "az_merge.h"
#include "az_net.h"
#include "az_optim.h"
#include "az_score.h"
#include "az_solve.h"
#include "az_target.h"
#include "az_rating.h"
#include "az_samples.h"
#include "az_train.h"
#include "az_tree.h"
#include "az_gumbel.h"

using namespace az;

// ---------------------------------------------------------------------------------------------
namespace {

struct HipFail { hipError_t code; const char* what; };
#define HIPCHK(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) throw HipFail{_e, #expr}; } while (0)

struct DeviceMem {
    std::vector<void*> ptrs;
    template <class T> T* alloc(size_t n) {
        void* p = nullptr;
        HIPCHK(hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T)));
        ptrs.push_back(p);
        return (T*)p;
    }
    void release() {
        for (void* p : ptrs) (void)hipFree(p);
        ptrs.clear();
    }
    ~DeviceMem() { release(); }
};

struct NetModel {
    int kind = -1;
    uint64_t salt = 0;
    ConvNet* conv = nullptr;
    uint64_t cache_tag = 0;     // evaluation-cache tag of the current weights (0 = none yet); new tag per upload
    uint64_t generation = 0;    // bumped by every weight upload / kind change of any model of the process: part of a search graph's key
    int klass = AZ_NET_CLASS_ENGINE;   // az_net_set_class: state of the id (survives uploads, dropped by az_net_free)
};
std::atomic<uint64_t> g_model_generation{0};     // engines of one process run concurrently (one host thread each)

// timed regions (profile mode): event pairs recorded on the engine stream, resolved at sync points
enum Region { RG_TREE = 0, RG_NET = 1, RG_COUNT };   // RG_NET brackets the whole predict (kept for stub nets)
struct Profiler {
    bool on = false;
    std::vector<hipEvent_t> pool;
    struct Rec { hipEvent_t a, b; int region; };
    std::vector<Rec> open;
    hipEvent_t get() {
        if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
        hipEvent_t e;
        HIPCHK(hipEventCreate(&e));
        return e;
    }
    hipEvent_t begin(hipStream_t s) { hipEvent_t a = get(); HIPCHK(hipEventRecord(a, s)); return a; }
    void end(hipEvent_t a, int region, hipStream_t s) {
        hipEvent_t b = get();
        HIPCHK(hipEventRecord(b, s));
        open.push_back({a, b, region});
    }
    // call after the stream has been synchronised
    void resolve(double* ms_by_region) {
        for (auto& r : open) {
            float ms = 0;
            if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) ms_by_region[r.region] += ms;
            pool.push_back(r.a);
            pool.push_back(r.b);
        }
        open.clear();
    }
    ~Profiler() { for (auto e : pool) (void)hipEventDestroy(e); }
};

// RCCL entry points, resolved at the first az_comm_* call.  Not a link-time dependency: a process that also hosts another copy
// of RCCL (PyTorch bundles one) must not have two sets of ncclXxx symbols bound into one namespace.  load() may race between the
// engines of one process (one host thread each): it runs under a mutex, and the table is only read once load() has returned true.
struct Rccl {
    std::mutex mu;
    void* lib = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    bool load(std::string* why) {
        std::lock_guard<std::mutex> lk(mu);
        if (lib) return true;
        for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
            lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
            if (lib) break;
        }
        if (!lib) { *why = std::string("cannot load librccl: ") + dlerror(); return false; }
        bool ok = true;
        auto sym = [&](const char* n) { void* p = dlsym(lib, n); if (!p) { ok = false; *why = std::string("librccl lacks ") + n; } return p; };
        GetUniqueId = (decltype(GetUniqueId))sym("ncclGetUniqueId");
        CommInitRank = (decltype(CommInitRank))sym("ncclCommInitRank");
        CommDestroy = (decltype(CommDestroy))sym("ncclCommDestroy");
        AllGather = (decltype(AllGather))sym("ncclAllGather");
        AllReduce = (decltype(AllReduce))sym("ncclAllReduce");
        Send = (decltype(Send))sym("ncclSend");
        Recv = (decltype(Recv))sym("ncclRecv");
        GroupStart = (decltype(GroupStart))sym("ncclGroupStart");
        GroupEnd = (decltype(GroupEnd))sym("ncclGroupEnd");
        GetErrorString = (decltype(GetErrorString))sym("ncclGetErrorString");
        if (!ok) { dlclose(lib); lib = nullptr; }
        return ok;
    }
};
Rccl g_rccl;      // function table only (no per-engine state)
// the in-process ids of az_comm_local_id (csrc/az_local_comm.h): engines of this process that form a world without RCCL
LocalCommRegistry g_local_comms{(int64_t)getpid()};

// (s, pi, z) as one 48-byte tuple: the unit of the episode-batch gather (symmetries are regenerated at the destination)
struct PackedSample { unsigned long long s0, s1; float pi[7]; float z; };
static_assert(sizeof(PackedSample) == 48, "48-byte tuples");
// ---- "eval_mirror" for az_net_predict_states: states[i] <- c(states[i]), flags[i] = mirrored; then pi rows of flagged states reversed ----
// (the board and its mirror are the same for both games)
__global__ void k_canonicalise(ulonglong2* __restrict__ states, uint8_t* __restrict__ flags, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t m;
    const ulonglong2 c = ConnectFour::canonical(states[i], &m);
    if (m) states[i] = c;
    flags[i] = (uint8_t)m;
}
// one thread per (row, slot) of the [n][8] output rows: slot a < 7 of a flagged row trades places with slot mirror_action(a); slot 7 is v
__global__ void k_unmirror_rows(float* __restrict__ pi, const uint8_t* __restrict__ flags, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int row = i >> 3, a = i & 7;
    if (row >= n || !flags[row] || a >= ConnectFour::ACTIONS / 2) return;
    const size_t lo = (size_t)row * 8 + a, hi = (size_t)row * 8 + ConnectFour::mirror_action(a);
    const float x = pi[lo];
    pi[lo] = pi[hi];
    pi[hi] = x;
}
void launch_canonicalise(ulonglong2* states, uint8_t* flags, int n, hipStream_t s) {
    if (n > 0) hipLaunchKernelGGL(k_canonicalise, dim3((n + 255) / 256), dim3(256), 0, s, states, flags, n);
}
void launch_unmirror_rows(float* pi, const uint8_t* flags, int n, hipStream_t s) {
    if (n > 0) hipLaunchKernelGGL(k_unmirror_rows, dim3((n * 8 + 255) / 256), dim3(256), 0, s, pi, flags, n);
}

__global__ void k_pack_samples(const ulonglong2* st, const float* pi, const float* z, PackedSample* out, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    PackedSample p;
    const ulonglong2 s = st[i];
    p.s0 = s.x; p.s1 = s.y;
#pragma unroll
    for (int a = 0; a < 7; ++a) p.pi[a] = pi[i * 7 + a];
    p.z = z[i];
    out[i] = p;
}
__global__ void k_unpack_samples(const PackedSample* in, ulonglong2* st, float* pi, float* z, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const PackedSample p = in[i];
    st[i] = make_ulonglong2(p.s0, p.s1);
#pragma unroll
    for (int a = 0; a < 7; ++a) pi[i * 7 + a] = p.pi[a];
    z[i] = p.z;
}

inline uint32_t next_pow2_u32(uint64_t x) {
    uint64_t p = 1;
    while (p < x) p <<= 1;
    return (uint32_t)p;
}

struct TreeHost {
    DeviceMem mem;
    TreeDev d{};
    EvalBatch eb{};         // eval batch of even simulations (and of the root evaluation)
    EvalBatch eb2{};        // eval batch of odd simulations: k_backup_select ping-pongs between the two
    // a run of simulation steps as ONE hipGraph launch (run_search): every launch of a search takes the same arguments, so the
    // instantiated graph is reused as long as nothing that shapes a launch changes (graph_key: grids, kernel choices, pointers)
    struct StepGraph { hipGraphExec_t exec = nullptr; std::vector<unsigned char> key; };
    StepGraph step_graph;
    unsigned long long* d_totals = nullptr;   // [ST_COUNT] k_harvest's sums
    // Gumbel root search ("gumbel_m"): per-tree baseline, variates and selected action of the current move; handed to the kernels through
    // TreeDev.move.gumbel only while the option is on (root_move_for)
    uint4* gz_base = nullptr;                 // [G]
    float* gz_g = nullptr;                    // [G][8]
    int32_t* gz_selected = nullptr;           // [G]
    uint32_t* d_counts = nullptr;             // [G] NodeStore::len per tree (k_harvest)
    // blocks = child blocks the trees can use (each holds the <= 7 children of one expansion, or a root);
    // reserve_nodes = reserve_space (src/node.rs:146) clamped to what is reachable
    // allocation key (the engine keeps finished calls' arenas for the next call of the same shape)
    int k_G = 0, k_T = 1; uint64_t k_blocks = 0; uint32_t k_H = 0;
    bool in_use = false;
    bool fits(int G, uint64_t blocks, uint32_t H, int T) const { return G == k_G && blocks == k_blocks && H == k_H && T == k_T; }
    // make a kept arena look freshly created (the trees themselves are rebuilt by launch_reset_trees)
    void recycle(uint64_t reserve_nodes, hipStream_t s) {
        d.reserve_nodes = (uint32_t)reserve_nodes;
        d.move = RootMove{};                      // the root-move options belong to the call that arms them (ScopedRootMove; the arena never does)
        HIPCHK(hipMemsetAsync(d.err, 0, ERR_COUNT * sizeof(uint32_t), s));
        HIPCHK(hipMemsetAsync(d_totals, 0, ST_TOTALS * sizeof(unsigned long long), s));
        HIPCHK(hipMemsetAsync(eb.n, 0, sizeof(uint32_t), s));
        HIPCHK(hipMemsetAsync(eb2.n, 0, sizeof(uint32_t), s));
        HIPCHK(hipMemsetAsync(eb.tkey, 0, ((size_t)eb.tmask + 1) * 8, s));       // a call that failed half way may have left keys behind
        HIPCHK(hipMemsetAsync(eb2.tkey, 0, ((size_t)eb2.tmask + 1) * 8, s));
        if (d.thr) HIPCHK(hipMemsetAsync(d.thr, 0, (size_t)d.G * d.T * sizeof(TreeLine), s));
        launch_init_heads(d, s);
    }
    // T = simulations in flight per tree (1: the single-simulation kernels; > 1: per-thread lines + T rows per tree in a leaf batch)
    ~TreeHost() { if (step_graph.exec) (void)hipGraphExecDestroy(step_graph.exec); }
    void create(int G, uint64_t blocks, uint64_t reserve_nodes, uint32_t H, int T, int game) {
        k_G = G; k_blocks = blocks; k_H = H; k_T = T;
        d.game = game;
        d.T = T;
        d.G = G; d.R = (uint32_t)(blocks * BLOCK_SLOTS); d.H = H; d.reserve_nodes = (uint32_t)reserve_nodes;
        size_t slots = (size_t)G * d.R;
        if (d.R > MAX_TREE_SLOTS) throw HipFail{hipErrorInvalidValue, "a tree of more than 2^20 node slots (num_sims x plies too large for the 20-bit links of the node record)"};
        d.node = mem.alloc<uint4>(slots);
        d.key = mem.alloc<unsigned long long>(slots);
        d.hash = mem.alloc<uint32_t>((size_t)G * H);
        d.head = mem.alloc<TreeLine>(G);
        d.path = mem.alloc<uint32_t>((size_t)G * T * PATH_CAP);
        d.err = mem.alloc<uint32_t>(ERR_COUNT);
        d.log_cap = 0;
        if (T > 1) {
            d.thr = mem.alloc<TreeLine>((size_t)G * T);
            HIPCHK(hipMemset(d.thr, 0, (size_t)G * T * sizeof(TreeLine)));
        }
        d_totals = mem.alloc<unsigned long long>(ST_TOTALS);
        d_counts = mem.alloc<uint32_t>(G);
        gz_base = mem.alloc<uint4>(G);
        gz_g = mem.alloc<float>((size_t)G * BLOCK_SLOTS);
        gz_selected = mem.alloc<int32_t>(G);
        HIPCHK(hipMemset(gz_base, 0, (size_t)G * sizeof(uint4)));
        HIPCHK(hipMemset(gz_g, 0, (size_t)G * BLOCK_SLOTS * sizeof(float)));
        HIPCHK(hipMemset(gz_selected, 0xFF, (size_t)G * sizeof(int32_t)));
        HIPCHK(hipMemset(d.err, 0, ERR_COUNT * sizeof(uint32_t)));
        HIPCHK(hipMemset(d_totals, 0, ST_TOTALS * sizeof(unsigned long long)));
        launch_init_heads(d, nullptr);
        HIPCHK(hipDeviceSynchronize());
        for (EvalBatch* b : {&eb, &eb2}) {
            const size_t rows = (size_t)G * T;
            b->cap = (int32_t)rows;
            b->n = mem.alloc<uint32_t>(1);
            b->state = mem.alloc<ulonglong2>(rows);
            b->pi = mem.alloc<float>(rows * 8);
            b->v = mem.alloc<float>(rows);
            HIPCHK(hipMemset(b->n, 0, sizeof(uint32_t)));
            // election table of the leaf de-duplication (used when the engine's "eval_dedup" applies to a search's net)
            const uint32_t tsize = next_pow2_u32(4ull * (uint64_t)std::max<size_t>(rows, 16));
            b->tkey = mem.alloc<unsigned long long>(tsize);
            b->tuniq = mem.alloc<uint32_t>(tsize);
            b->tmask = tsize - 1;
            HIPCHK(hipMemset(b->tkey, 0, (size_t)tsize * 8));
        }
    }
};

uint32_t next_pow2(uint64_t x) {
    uint64_t p = 1;
    while (p < x) p <<= 1;
    return (uint32_t)p;
}
// Largest tree an episode of <= `calls` get_action_prob calls can build: the initial root + 7,
// per call one fresh root (S10) and num_sims expansions, 7 placeholders each.
uint64_t reachable_slots(int num_sims, int calls) {
    return 8ull + (uint64_t)calls * ((uint64_t)num_sims * 7ull + 8ull);
}
// child blocks the same tree can use: two for the initial root, per call two for a fresh root (S10) and one per expansion;
// never more than one per pushed node
uint64_t reachable_blocks(int num_sims, int calls, uint64_t reserve_nodes) {
    return std::min<uint64_t>(2ull + (uint64_t)calls * ((uint64_t)num_sims + 2ull), std::max<uint64_t>(reserve_nodes, 2ull) + 1ull);
}
uint32_t hash_entries(int num_sims, int calls) {
    return next_pow2(2ull * ((uint64_t)calls * ((uint64_t)num_sims + 1) + 2));
}

// ---- shared tree batch (az_tree_share) ----
// One caller's get_action_prob on its slot.  The follower thread only fills this in and sleeps; the leader reads the state, runs
// the batch and writes the answer (caller buffers in device memory included), so followers never make a HIP call.
struct SlotCall {
    const uint64_t* state;
    float temp;
    uint64_t seed, game_id;
    float* pi;
    uint16_t* counts;
    float* q;
    az_status status;
};
struct SlotRunner {
    az_tree* t;
    void operator()(CombineBatch<SlotCall>& b) const;
};
constexpr size_t SLOT_ERR_LEN = 256;
struct SharedTrees {
    SlotCombiner<SlotCall, SlotRunner> comb;
    DeviceMem mem;
    SlotReq* d_req = nullptr;        // [G] the batch's request block
    uint8_t* d_reset = nullptr;      // [G] launch_reset_trees flags
    void* h_io = nullptr;            // pinned: SlotReq [G] (uploaded with one copy) + SlotOut [G] (written by k_slot_root_policy)
    SlotReq* h_req = nullptr;
    SlotOut* h_out = nullptr;
    // message of each slot's last failed call (az_tree_slot_error); written by the leader of the batch before the owner wakes
    std::vector<std::array<char, SLOT_ERR_LEN>> err;
    SharedTrees(int G, az_tree* t) : comb(G, SlotRunner{t}), err((size_t)G) {
        for (auto& m : err) m[0] = 0;
    }
    ~SharedTrees() { if (h_io) (void)hipHostFree(h_io); }
};

}  // namespace

struct az_engine {
    int device = 0;
    hipStream_t stream = nullptr;
    az_config cfg{};
    std::string err;
    std::map<int, NetModel> nets;
    az_stats stats{};
    Profiler prof;
    NetProfile netprof;
    NetOptions netopt;              // kernel-set switches of the conv net: this engine's, passed down with every forward
    int tree_block4 = 1;            // "tree_block4": k_backup_select as 4-wave workgroups
    // Dirichlet root noise of self-play and the tree calls, never of the arena ("root_noise_eps_e6" 0 = off, "root_noise_alpha_e6")
    int64_t root_noise_eps_e6 = 0, root_noise_alpha_e6 = 1000000;
    // playout cap randomization of self-play ("playout_cap_sims" 0 = off, "playout_cap_full_e6"); never the arena or the tree calls
    int64_t playout_cap_sims = 0, playout_cap_full_e6 = 250000;
    // forced playouts at the root and policy target pruning, on the moves root noise can apply to ("forced_playouts_k_e6" 0 = off, "policy_prune")
    int64_t forced_playouts_k_e6 = 0, policy_prune = 0;
    // Gumbel root search with sequential halving on the same moves ("gumbel_m" 0 = off, "gumbel_c_visit_e6", "gumbel_c_scale_e6"); never the
    // arena or the slot calls
    int64_t gumbel_m = 0, gumbel_c_visit_e6 = GUMBEL_C_VISIT_E6_DEFAULT, gumbel_c_scale_e6 = GUMBEL_C_SCALE_E6_DEFAULT;
    // the decided-move stop (include/az_search_stop.h; csrc/az_stop.h): az_search_stop_set's switch, the device counters the count kernel
    // adds to (allocated when the switch is first set to 1) and their sums, folded once per call
    int32_t search_stop = 0;
    DeviceMem stop_mem;
    unsigned long long* stop_stat = nullptr;
    uint64_t stop_totals[SS_COUNT] = {0, 0, 0, 0};
    // paired openings of az_arena, never of self-play or the tree calls ("arena_opening_plies" 0 = off; az_arena_set_opening_book)
    int64_t arena_opening_plies = 0;
    std::vector<uint64_t> ar_book;      // [entries][2] {first seat's stones, second seat's stones}; empty = no book
    std::vector<uint64_t> sp_full_plies;        // az_selfplay_get_full_plies: the full-ply masks of the last az_selfplay / az_selfplay_next
    // "selfplay_record_search": self-play keeps the root value and the root's stored priors of every move (csrc/az_target.h); the rows of the
    // last az_selfplay / az_selfplay_next, tuple for tuple in az_samples' order (az_selfplay_get_search)
    int64_t selfplay_record_search = 0;
    std::vector<float> sp_search_q, sp_search_prior;
    bool sp_search_valid = false;               // the last az_selfplay / az_selfplay_next ran with the option on
    // activation workspaces of the conv net, one per stream that runs forwards: [0] the engine stream, [1 + i] side[i] below; created on
    // first use, shared by every model id
    NetWorkspace* ws[4] = {nullptr, nullptr, nullptr, nullptr};
    // the side streams of az_arena and az_tournament (match_run): the models' searches of a ply run on the engine's stream and these.  Each
    // is created by the first call that needs it and kept until az_destroy (a search graph's key holds its stream); az_arena's old model
    // searches on side[0]
    hipStream_t side[3] = {nullptr, nullptr, nullptr};
    // eval log of the last az_selfplay
    std::vector<int32_t> sp_log_count;
    std::vector<uint64_t> sp_log_states;
    std::vector<float> sp_log_pi, sp_log_v;
    int sp_log_cap = 0;
    // eval logs of the last az_arena with record_evals: [0] the new model's trees, [1] the old model's
    struct EvalLog { std::vector<int32_t> count; std::vector<uint64_t> states; std::vector<float> pi, v; };
    EvalLog ar_log[2];
    struct SelfplaySession* sp_session = nullptr;      // az_selfplay_begin .. az_selfplay_end
    int32_t sp_model_id = 0;                           // the open session's model id (meaningful while sp_session is set)
    int ar_log_cap = 0, ar_log_games = 0;
    std::vector<uint8_t> ar_moves;      // [games][AZ_MAX_PLIES] move record of the last az_arena (az_arena_get_moves)
    std::vector<int32_t> ar_len;
    // az_arena_get_openings: where each game of the last az_arena started, and the random plies that led there from its base
    std::vector<uint64_t> ar_open_boards;   // [games][2]
    std::vector<int32_t> ar_open_len;       // [games]
    std::vector<uint8_t> ar_open_moves;     // [games][OPENING_MAX_PLIES]
    // NNet::train
    Trainer* trainer = nullptr;
    bool train_open = false;
    TrainHyper hyper;
    int train_epochs = 10, train_batch = 64;       // connect_four_net.py:13-14
    uint64_t train_seed = 0;
    int train_graph = 1;
    TrainSwitches train_sw;         // "train_gemm" ... "train_fork": the routes of a step (csrc/az_train_plan.h)
    std::vector<float> train_history;              // (loss_pi, loss_v) mean per epoch of the last az_net_train
    // the opt-in optimiser rules (csrc/az_optim.h), read by az_net_train_begin: "train_weight_decay_e9", "train_clip_norm_e6",
    // "train_lr_warmup_steps", "train_lr_decay", "train_lr_floor_e6", "train_lr_total_steps", "train_ema_decay_e9"
    int64_t train_weight_decay_e9 = 0, train_clip_norm_e6 = 0, train_lr_warmup_steps = 0, train_lr_decay = 0, train_lr_floor_e6 = 0,
            train_lr_total_steps = 0, train_ema_decay_e9 = 0;
    bool train_ema_session = false;                // the last az_net_train_begin saw "train_ema_decay_e9" > 0
    // per-epoch validation of az_net_train / az_net_train_samples (az_net_train_set_validation; csrc/az_score.h): the
    // registered set on the device (validated states, pis, zs, weights or nullptr), the model slot no id names, the last run's history
    DeviceMem val_mem;
    int64_t val_n = 0;
    ulonglong2* val_states = nullptr;
    float *val_pis = nullptr, *val_zs = nullptr;
    uint32_t* val_weights = nullptr;
    NetModel val_model;
    int64_t train_keep_best = 0, train_patience = 0;       // "train_keep_best", "train_patience"
    std::vector<double> val_history;               // (loss_pi, loss_v, kl, top1) per epoch of the last az_net_train / az_net_train_samples
    int val_best = -1;
    // leaf de-duplication + evaluation cache (az_set_option "eval_dedup", "eval_cache_log2", "eval_cache_max_stones",
    // "eval_cache_persist")
    int profile_every = 1;          // profile mode: bracket every n-th simulation step ("profile_every")
    int dedup_stats = 1;            // "dedup_stats": the leaf-row accounting counters (requested / executed / hits / duplicates)
    uint64_t profile_tick = 0;
    int search_graph = 20;          // "search_graph": simulation steps per hipGraph launch (0 = every kernel launched on its own); not in profile mode
    int selfplay_async = 0;         // "selfplay_async": 1 = az_selfplay with free-running slots (k_async_step) for nets that go through leaf batches; 0 (default) = lock-step
                                    // moves.  Bit-identical games; measured in round 4: larger batches (4000 against 2700 rows per forward), fewer forwards, the same
                                    // time per row -- the step is throughput-bound per row, so it is not the default (profiles/README.md)
    int selfplay_async_launches = 2;   // "selfplay_async_launches": tree launches that share one leaf batch (cache-answered trees go on in the next one)
    int selfplay_async_iters = 6;   // "selfplay_async_iters": stages (backup, root, move, select) a slot may run per launch
    int search_graph_rows = 1024;   // "search_graph_rows": ... for searches whose expected leaf batch has at most this many rows (the arena, a drain, single trees)
    int fused_search = 1;           // stub / hash nets: the whole search in one launch ("fused_search"; 0 = one launch per simulation)
    int eval_dedup = 1;             // 0 off, 1 conv nets (default), 2 every net (lets the hash fixture exercise the machinery)
    int eval_mirror = 0;            // "eval_mirror": conv models answer with F (the net on the canonical orientation, pi un-mirrored)
    int eval_cache_log2 = 30;       // entries = 2^log2 (40 B each: 43 GB); 0 = no cache, in-batch de-duplication only
    int eval_cache_max_stones = 42;
    int eval_cache_persist = 0;     // 0: az_selfplay / az_arena / az_tree_get_action_prob start from an empty cache
    DeviceMem cache_mem;            // the accounting counters
    EvalCache cache{};              // the view the current call uses (prepare_cache); key == nullptr: no cache
    unsigned long long* cache_keys = nullptr;       // the allocation: 2^cache_alloc_log2 entries
    float* cache_pv = nullptr;
    int cache_alloc_log2 = -1;
    uint64_t next_cache_tag = 1;    // 15 bits; wrapping clears the cache
    // tree arenas of finished az_selfplay / az_arena calls, reused by the next call of the same shape (9.7 GB at 8192 x 100:
    // no hipMalloc / hipFree per call); at most three are kept (self-play + the arena's pair)
    std::vector<std::unique_ptr<TreeHost>> tree_pool;
    uint64_t tree_pool_allocs = 0;  // arenas created (a second call of the same shape must not add to it)
    // communicator of the sharded Coach loop (az_comm_init): RCCL on the engine's stream, or an in-process group
    // (az_comm_local_id; csrc/az_local_comm.h) -- at most one of the two is set
    ncclComm_t comm = nullptr;
    std::shared_ptr<LocalGroup> local;
    int comm_rank = 0, comm_world = 1;
    bool has_comm() const { return comm || local; }
    // staging of the collectives (az_gather_samples, az_allreduce_u64): one device allocation that only grows
    struct Scratch {
        void* p = nullptr;
        size_t cap = 0;
        uint64_t serial = 0;        // moves on with every allocation: content kept across calls belongs to ONE serial (an address can come back)
        void* ensure(size_t bytes, hipStream_t s) {
            if (bytes <= cap) return p;
            HIPCHK(hipStreamSynchronize(s));
            if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
            const size_t want = std::max<size_t>(bytes + bytes / 4, (size_t)1 << 16);
            HIPCHK(hipMalloc(&p, want));
            cap = want;
            ++serial;
            return p;
        }
        void release(hipStream_t s) {
            if (!p) return;
            HIPCHK(hipStreamSynchronize(s));
            (void)hipFree(p);
            p = nullptr; cap = 0;
            ++serial;
        }
        // a workspace sized by the call: given back first when the call needs under a quarter of more than 256 MiB (merge_scratch's rule below)
        void* fit(size_t bytes, hipStream_t s) {
            if (cap > ((size_t)1 << 28) && cap / 4 > bytes) release(s);
            return ensure(bytes, s);
        }
        ~Scratch() { if (p) (void)hipFree(p); }
    } comm_scratch;
    Scratch score_scratch;          // workspace of az_net_evaluate / az_samples_holdout and of the per-epoch validation; follows merge_scratch's rule
    Scratch target_scratch;         // workspace of az_samples_blend_z / az_samples_surprise; follows merge_scratch's rule
    Scratch reanalyse_scratch;      // az_reanalyse's staged window, outputs and chunk arrays; follows merge_scratch's rule
    Scratch merge_scratch;          // workspace of az_samples_merge: sized by the call, kept for later calls of the same or a smaller size, given back
                                    // when a call needs under a quarter of a workspace of more than 256 MiB (a 2^24-tuple call holds over 10 GB)
    // az_solve / az_move_quality: solve_table = [counter][generation per lane, room for the device's lanes][lanes << tt_log2 entries], solve_io =
    // staged inputs and outputs.  Both follow merge_scratch's rule.  The table's content outlives a call (a lane's generation counter tells
    // its entries from older ones).  The layout does NOT depend on a call's lane count: lane L's counter and slice sit at the same place in
    // every call of one tt_log2, a call with fewer lanes uses a prefix.  The content belongs to one allocation (Scratch::serial) and one
    // tt_log2, and is valid for the first solve_table_lanes lanes; anything else zeroes the whole workspace first
    Scratch solve_table, solve_io;
    uint64_t solve_table_serial = 0;
    int solve_table_log2 = -1;
    uint32_t solve_table_lanes = 0;
    int solve_device_lanes = 0;     // CUs x resident waves x 64 of the search kernel, asked once
};

struct az_tree {
    az_engine* e = nullptr;
    TreeHost th;
    DeviceMem mem;
    int num_sims = 0, max_depth = 0, model_id = 0, cpuct = 0;
    ulonglong2* d_root_states = nullptr;
    ulonglong2* d_noise_streams = nullptr;     // [G] (seed, game_id) of each tree's current call: the root-noise and Gumbel streams
    bool last_gumbel = false;                  // the last az_tree_get_action_prob was a Gumbel move (az_tree_get_selected)
    // pinned host block of one get_action_prob call: the roots go up from it and k_root_policy / k_call_readback write the
    // results and counters straight into it, so a call costs one stream synchronisation instead of eight blocking copies
    void* h_io = nullptr;
    CallReadback* h_rb = nullptr;
    ulonglong2* h_states = nullptr;
    float* h_pi = nullptr;
    float* h_q = nullptr;
    uint16_t* h_counts = nullptr;
    std::unique_ptr<SharedTrees> shared;     // az_tree_share: slots driven by many host threads
    ~az_tree() { if (h_io) (void)hipHostFree(h_io); }
};

namespace {

az_status fail(az_engine* e, az_status st, const std::string& msg) {
    if (e) e->err = msg;
    return st;
}
// what az_selfplay, az_selfplay_begin and az_tree_get_action_prob refuse while "gumbel_m" is on
az_status gumbel_refusal(az_engine* e, int T, const char* who) {
    if (e->gumbel_m == 0) return AZ_OK;
    if (T > 1) return fail(e, AZ_ERR_BAD_ARGUMENT, std::string(who) + ": gumbel_m needs num_sim_threads = 1");
    if (e->selfplay_async) return fail(e, AZ_ERR_BAD_ARGUMENT, std::string(who) + ": gumbel_m and selfplay_async exclude each other");
    if (e->forced_playouts_k_e6 > 0) return fail(e, AZ_ERR_BAD_ARGUMENT, std::string(who) + ": gumbel_m and forced_playouts_k_e6 exclude each other (both claim the root's arg-max)");
    return AZ_OK;
}
// what the entries that search refuse while the decided-move stop is on (include/az_search_stop.h).  root_rules: the entry can search by
// "gumbel_m", "forced_playouts_k_e6" or "selfplay_async" (the arena and the tournament ignore all three)
az_status stop_refusal(az_engine* e, int T, const char* who, bool root_rules) {
    if (!e->search_stop) return AZ_OK;
    if (T > 1) return fail(e, AZ_ERR_BAD_ARGUMENT, std::string(who) + ": search_stop needs num_sim_threads = 1");
    if (!root_rules) return AZ_OK;
    if (e->selfplay_async) return fail(e, AZ_ERR_BAD_ARGUMENT, std::string(who) + ": search_stop and selfplay_async exclude each other");
    if (e->gumbel_m != 0) return fail(e, AZ_ERR_BAD_ARGUMENT, std::string(who) + ": search_stop and gumbel_m exclude each other (the rule is stated for the PUCT root)");
    if (e->forced_playouts_k_e6 > 0) return fail(e, AZ_ERR_BAD_ARGUMENT, std::string(who) + ": search_stop and forced_playouts_k_e6 exclude each other (the rule is stated for the PUCT root)");
    return AZ_OK;
}
// the record of an entry whose moves have budget num_sims and are eligible when stones + 1 >= temp_threshold (az_tree.h SearchStop)
SearchStop stop_for(const az_engine* e, int num_sims, int32_t temp_threshold) {
    SearchStop st{};
    if (!e->search_stop) return st;
    st.on = 1u; st.num_sims = (uint32_t)num_sims; st.temp_threshold = temp_threshold; st.stat = e->stop_stat;
    return st;
}
// The call-interleaving contract of an open self-play session (include/az_engine.h, next to az_selfplay_begin): an entry that could change
// what the session's remaining chunks are -- a tree search (it sizes, clears and retags the evaluation cache), a write to the session's
// model, an option the session captured at begin or reads while it plays -- is refused on entry, before any work, with a message that
// names it.  session_refusal: refused whatever the arguments are; session_model_refusal: refused for the session's model id only.
az_status session_refusal(az_engine* e, const char* entry) {
    if (!e->sp_session) return AZ_OK;
    return fail(e, AZ_ERR_BAD_ARGUMENT, std::string(entry) + ": refused while a self-play session is open (az_selfplay_end first)");
}
az_status session_model_refusal(az_engine* e, const char* entry, int32_t model_id) {
    if (!e->sp_session || model_id != e->sp_model_id) return AZ_OK;
    return fail(e, AZ_ERR_BAD_ARGUMENT, std::string(entry) + ": model " + std::to_string(model_id) +
                                            " belongs to the open self-play session (az_selfplay_end first)");
}
az_status fail_hip(az_engine* e, const HipFail& f) {
    char buf[512];
    std::snprintf(buf, sizeof buf, "HIP error %d (%s) at %s", (int)f.code, hipGetErrorString(f.code), f.what);
    return fail(e, AZ_ERR_HIP, buf);
}

// ---- a window of training tuples through the C ABI (csrc/az_samples.h) -------------------------------------------------------------------
// what a window lacks, for the caller to put its own name and subject in front of; allow_empty: a window of no tuples needs no array
const char* samples_shape_error(const az_samples* smp, bool allow_empty) {
    if (allow_empty && smp->count == 0) return nullptr;
    return (!smp->pis || !smp->zs || (!smp->states && !smp->boards)) ? "pis, zs and states or boards" : nullptr;
}
// the window to the device: its states, or without states its boards, to d_in; pis and zs
SampleWindow stage_window(void* d_in, void* d_pis, void* d_zs, const az_samples* smp, hipStream_t s) {
    const size_t N = (size_t)smp->count;
    if (smp->states) HIPCHK(hipMemcpyAsync(d_in, smp->states, N * 16, hipMemcpyDefault, s));
    else HIPCHK(hipMemcpyAsync(d_in, smp->boards, N * AZ_FEATURES * 4, hipMemcpyDefault, s));
    HIPCHK(hipMemcpyAsync(d_pis, smp->pis, N * AZ_ACTIONS * 4, hipMemcpyDefault, s));
    HIPCHK(hipMemcpyAsync(d_zs, smp->zs, N * 4, hipMemcpyDefault, s));
    return {smp->states ? (const ulonglong2*)d_in : nullptr, smp->states ? nullptr : (const float*)d_in, (const float*)d_pis, (const float*)d_zs};
}
// the verdict word of a validating pass, behind one synchronisation of the stream
uint32_t read_verdict(const uint32_t* d_bad, hipStream_t s) {
    uint32_t bad = 0;
    HIPCHK(hipMemcpyAsync(&bad, d_bad, sizeof bad, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
    return bad;
}

// The root-move options as the kernels take them, for searches of num_sims simulations at cpuct_f on the trees of th.  Each option that is
// off gives its all-zero sub-record whatever its secondary keys say ("root_noise_alpha_e6", "policy_prune", the Gumbel constants): the
// launchers then pick today's instantiations and the search graph's key is that of an engine that never set the keys.  The caller adds what
// only it knows: the stream (while noise or Gumbel is on), Gumbel's temp_threshold and the playout cap.
RootMove root_move_for(const az_engine* e, const TreeHost& th, int num_sims, float cpuct_f, bool gumbel_allowed) {
    RootMove m{};
    if (e->root_noise_eps_e6 != 0) {           // the divisions in double, rounded once to f32
        m.noise.eps = (float)((double)e->root_noise_eps_e6 / 1e6);
        m.noise.alpha = (float)((double)e->root_noise_alpha_e6 / 1e6);
    }
    if (e->forced_playouts_k_e6 != 0) {
        m.forced.k = forced_k_of(e->forced_playouts_k_e6);
        m.forced.prune = e->policy_prune ? 1u : 0u;
        m.forced.cpuct_f = cpuct_f;
    }
    if (gumbel_allowed && e->gumbel_m != 0) {
        m.gumbel.m = (uint32_t)e->gumbel_m;
        m.gumbel.c_visit = gumbel_of_e6(e->gumbel_c_visit_e6);
        m.gumbel.c_scale = gumbel_of_e6(e->gumbel_c_scale_e6);
        m.gumbel.num_sims = (uint32_t)num_sims;
        m.gumbel.base = th.gz_base; m.gumbel.g = th.gz_g; m.gumbel.selected = th.gz_selected;
    }
    return m;
}
inline bool uses_root_stream(const RootMove& m) { return m.noise.eps != 0.0f || m.gumbel.m != 0u; }

NetWorkspace* workspace_for(az_engine* e, hipStream_t s) {
    int i = (s == e->stream) ? 0 : 1;
    for (int j = 1; j < 3; ++j) if (e->side[j] && s == e->side[j]) i = 1 + j;
    if (!e->ws[i]) {
        const char* why = nullptr;
        e->ws[i] = netws_create(e->cfg.net_channels, e->cfg.max_batch, &why);
        if (!e->ws[i]) throw HipFail{hipErrorOutOfMemory, why ? why : "netws_create"};
    }
    return e->ws[i];
}

// The numerics class a model's forwards run in: its own (az_net_set_class) or, by default, the engine's "net_fp8" option ...
int effective_class(const az_engine* e, const NetModel& m) { return m.klass == AZ_NET_CLASS_ENGINE ? (e->netopt.net_fp8 ? 1 : 0) : m.klass; }
// ... resolved here, once per forward: the kernels only ever see NetOptions::net_fp8
NetOptions netopt_for(const az_engine* e, const NetModel& m) {
    NetOptions o = e->netopt;
    o.net_fp8 = effective_class(e, m);
    return o;
}

void net_forward(az_engine* e, const NetModel& net, const EvalBatch& eb, int rows_hint, hipStream_t s, int rows_typ = 0, bool timed = true) {
    if (net.kind == AZ_NET_CONV) {
        convnet_forward(net.conv, workspace_for(e, s), eb, rows_hint, rows_typ, s, (e->prof.on && timed) ? &e->netprof : nullptr, netopt_for(e, net));
    } else {
        launch_net_fixture(eb, net.kind, net.salt, s);
    }
}

// "net_fp8": the model's fp8 weight copies and scales follow its parameters -- built when its effective class becomes fp8 and at every
// upload while it is, never by a forward (which may run inside a stream capture)
az_status fp8_sync_model(az_engine* e, NetModel& m) {
    if (m.kind != AZ_NET_CONV || !m.conv || !effective_class(e, m)) return AZ_OK;
    if (!convnet_build_fp8(m.conv, workspace_for(e, e->stream), e->stream)) return fail(e, AZ_ERR_HIP, "net_fp8: building the model's fp8 copies failed");
    return AZ_OK;
}

// "eval_mirror" reaches conv models only: the stub and hash nets are never canonicalised, on any path
bool mirror_applies(const az_engine* e, const NetModel& net) { return e->eval_mirror != 0 && net.kind == AZ_NET_CONV; }
bool dedup_applies(const az_engine* e, const NetModel& net) {
    return e->eval_dedup == 2 || (e->eval_dedup == 1 && net.kind == AZ_NET_CONV);
}

// The engine's evaluation cache.  Sized FROM THE CALL: a search call can insert at most `inserts_bound` distinct states (trees x
// get_action_prob calls x (sims + 1)), so it gets the smallest power of two >= 4 x that bound (8-way buckets stay sparse), at most
// 2^"eval_cache_log2" entries (40 bytes each; 43 GB at the default 30, which only a bench-sized call reaches) -- a 1-tree, 25-sim
// call allocates and clears 40 KB.  The allocation only grows; a smaller call uses (and clears) a prefix of it.  With
// "eval_cache_persist" entries must stay findable across calls, so the cache then has its full configured size from the start.
void prepare_cache(az_engine* e, bool wanted, uint64_t inserts_bound, hipStream_t s) {
    if (!e->cache.stat) {
        e->cache.stat = e->cache_mem.alloc<unsigned long long>((size_t)DD_REPLICAS * DD_STRIDE);
        HIPCHK(hipMemset(e->cache.stat, 0, (size_t)DD_REPLICAS * DD_STRIDE * sizeof(unsigned long long)));
    }
    if (!wanted || e->eval_cache_log2 < 3) { e->cache.key = nullptr; e->cache.pv = nullptr; e->cache.bmask = 0; return; }
    int want = e->eval_cache_log2;
    if (!e->eval_cache_persist) {
        int need = 10;
        while (need < want && (1ull << need) < 4ull * inserts_bound) ++need;
        want = need;
    }
    if (e->cache_alloc_log2 < want) {
        HIPCHK(hipStreamSynchronize(s));
        if (e->cache_keys) { (void)hipFree(e->cache_keys); e->cache_keys = nullptr; }
        if (e->cache_pv) { (void)hipFree(e->cache_pv); e->cache_pv = nullptr; }
        e->cache_alloc_log2 = -1;
        const size_t entries = (size_t)1 << want;
        HIPCHK(hipMalloc((void**)&e->cache_keys, entries * 8));
        HIPCHK(hipMalloc((void**)&e->cache_pv, entries * 8 * sizeof(float)));
        HIPCHK(hipMemset(e->cache_keys, 0, entries * 8));
        e->cache_alloc_log2 = want;
        for (auto& kv : e->nets) kv.second.cache_tag = 0;       // a new allocation holds nobody's entries
        e->next_cache_tag = 1;
    }
    const int view = want;          // persist: the configured size, the same for every call
    e->cache.key = e->cache_keys;
    e->cache.pv = e->cache_pv;
    e->cache.bmask = (uint32_t)(((size_t)1 << view) / 8 - 1);
    if (!e->eval_cache_persist) HIPCHK(hipMemsetAsync(e->cache.key, 0, ((size_t)e->cache.bmask + 1) * 64, s));      // this call's part only
}
// a new tag for a model's new weights: its old entries can never match again
void retag_model(az_engine* e, NetModel& m) {
    if (e->next_cache_tag > 0x7FFFull) {
        if (e->cache_keys) HIPCHK(hipMemset(e->cache_keys, 0, ((size_t)1 << e->cache_alloc_log2) * 8));
        for (auto& kv : e->nets) kv.second.cache_tag = 0;
        e->next_cache_tag = 1;
    }
    m.cache_tag = e->next_cache_tag++;
}
// cache view for one search (key == nullptr when only in-batch de-duplication is wanted or nothing applies)
EvalCache cache_for(az_engine* e, NetModel& net) {
    EvalCache c{};
    if (!dedup_applies(e, net)) return c;
    if (net.cache_tag == 0) retag_model(e, net);
    c = e->cache;
    c.max_stones = (uint32_t)e->eval_cache_max_stones;
    c.tag = (unsigned long long)net.cache_tag << 49;
    if (!e->dedup_stats) c.stat = nullptr;
    return c;
}
// A tree arena for one call: a kept one of the same shape, or a new one (the oldest idle one makes room).
struct TreeLease {
    TreeHost* th = nullptr;
    ~TreeLease() { if (th) th->in_use = false; }
    TreeHost* operator->() const { return th; }
    TreeHost& operator*() const { return *th; }
};
void acquire_trees(az_engine* e, TreeLease& lease, int G, uint64_t blocks, uint64_t reserve_nodes, uint32_t H, int T, hipStream_t s) {
    for (auto& p : e->tree_pool)
        if (!p->in_use && p->fits(G, blocks, H, T)) {
            p->in_use = true;
            lease.th = p.get();
            p->recycle(reserve_nodes, s);
            return;
        }
    // drop idle arenas of other shapes before allocating (two shapes of 10 GB each should not pile up)
    for (size_t i = 0; i < e->tree_pool.size();) {
        if (!e->tree_pool[i]->in_use && (e->tree_pool.size() >= 3 || !e->tree_pool[i]->fits(G, blocks, H, T))) {
            HIPCHK(hipStreamSynchronize(s));
            e->tree_pool.erase(e->tree_pool.begin() + (long)i);
        } else {
            ++i;
        }
    }
    std::unique_ptr<TreeHost> th(new TreeHost());
    th->create(G, blocks, reserve_nodes, H, T, e->cfg.game);
    th->in_use = true;
    lease.th = th.get();
    e->tree_pool.push_back(std::move(th));
    e->tree_pool_allocs += 1;
}

// Eval log of one call (replay parity): rows * cap records in device memory, attached to a tree arena for the call's duration.
struct ScopedEvalLog {
    TreeHost* th = nullptr;
    DeviceMem mem;
    size_t rows = 0;
    int cap = 0;
    void attach(TreeHost& t, size_t rows_, int cap_, const int32_t* log_row) {
        th = &t; rows = rows_; cap = cap_;
        t.d.log_cap = cap;
        t.d.log_state = mem.alloc<ulonglong2>(rows * (size_t)cap);
        t.d.log_pi = mem.alloc<float>(rows * (size_t)cap * 7);
        t.d.log_v = mem.alloc<float>(rows * (size_t)cap);
        t.d.log_row = log_row;
    }
    void copy_out(std::vector<uint64_t>& states, std::vector<float>& pi, std::vector<float>& v) const {
        states.resize(rows * cap * 2); pi.resize(rows * cap * 7); v.resize(rows * cap);
        HIPCHK(hipMemcpy(states.data(), th->d.log_state, states.size() * 8, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(pi.data(), th->d.log_pi, pi.size() * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(v.data(), th->d.log_v, v.size() * 4, hipMemcpyDeviceToHost));
    }
    ~ScopedEvalLog() {          // the arena goes back to the pool without the call's log
        if (th) { th->d.log_cap = 0; th->d.log_state = nullptr; th->d.log_pi = nullptr; th->d.log_v = nullptr; th->d.log_row = nullptr; }
    }
};

// The root-move record of one entry point's searches (az_tree.h RootMove), installed on a tree arena for their duration: the arena goes back
// to the pool, and an az_tree waits for its next call, with the all-zero record.
struct ScopedRootMove {
    TreeHost* th = nullptr;
    void install(TreeHost& t, const RootMove& m) { th = &t; t.d.move = m; }
    ~ScopedRootMove() { if (th) th->d.move = RootMove{}; }
};

// fold the device-side de-duplication counters into the engine stats (after a stream sync)
void fold_dedup(az_engine* e, const unsigned long long* h) {
    e->stats.leaf_rows_requested += h[DD_REQUESTED];
    e->stats.leaf_rows_executed += h[DD_EXECUTED];
    e->stats.eval_cache_hits += h[DD_CACHE_HITS];
    e->stats.eval_batch_dups += h[DD_BATCH_DUPS];
    e->stats.eval_cache_inserts += h[DD_INSERTS];
}
void harvest_dedup(az_engine* e) {
    if (!e->cache.stat) return;
    unsigned long long rep[DD_REPLICAS * DD_STRIDE], h[DD_COUNT] = {};
    HIPCHK(hipMemcpy(rep, e->cache.stat, sizeof rep, hipMemcpyDeviceToHost));
    HIPCHK(hipMemset(e->cache.stat, 0, sizeof rep));
    for (int r = 0; r < DD_REPLICAS; ++r)
        for (int i = 0; i < DD_COUNT; ++i) h[i] += rep[r * DD_STRIDE + i];
    fold_dedup(e, h);
}

// get_action_prob body shared by every entry point: S10/S1 prologue, then num_sims x
// {select+expand (+ leaf request), predict, mask+store+backup}  (src/async_mcts.rs:81-82, :191-217).
// rows_hint = host-side upper bound on the leaf batch (trees still searching): sizes the net's grids and picks tiles
void run_search(az_engine* e, TreeHost& th, const ulonglong2* d_root_states, int num_sims, SearchParams sp,
                NetModel& net, int rows_hint, hipStream_t s = nullptr, int rows_typ = 0, uint32_t* d_max_rows = nullptr) {
    if (!s) s = e->stream;
    th.d.block4 = e->tree_block4;
    const int T = th.d.T;
    if (rows_hint <= 0 || rows_hint > th.d.G) rows_hint = th.d.G;
    rows_hint *= T;                              // up to T leaves per tree and step
    const bool dedup = dedup_applies(e, net);
    if (net.kind != AZ_NET_CONV && !dedup && e->fused_search && T == 1) {
        // stub / hash nets are device functions of the state: the whole search is one launch
        hipEvent_t t0 = nullptr;
        if (e->prof.on) t0 = e->prof.begin(s);
        launch_search_fixture(th.d, d_root_states, sp, num_sims, net.kind, net.salt, s);
        if (e->prof.on) { e->prof.end(t0, RG_TREE, s); e->stats.tree_launches_timed += 1; }
        e->stats.tree_launches += 1;
        return;
    }
    const EvalCache ec = cache_for(e, net);
    EvalBatch B[2] = {th.eb, th.eb2};
    B[0].dedup = B[1].dedup = dedup ? 1 : 0;
    B[0].mirror = B[1].mirror = mirror_applies(e, net) ? 1 : 0;
    B[0].max_n = B[1].max_n = d_max_rows;
    // profile mode brackets every "profile_every"-th simulation step (events cost GPU idle time between dependent kernels)
    const int every = std::max(1, e->profile_every);
    // root: prepare (its leaf goes to batch 0), predict; then num_sims x {backup of the previous leaf + select of the next
    // (one launch, the new leaf goes to the other batch), predict}; a last backup closes the search.
    launch_root_prepare(th.d, B[0], ec, d_root_states, s);
    net_forward(e, net, B[0], rows_hint, s, rows_typ, false);
    if (T > 1) {
        // num_sims / T lock-step steps of T simulations per tree (src/async_mcts.rs:191-217; num_sims % T == 0, :192)
        const int steps = num_sims / T;
        for (int i = 0; i < steps; ++i) {
            const bool timed = e->prof.on && (e->profile_tick++ % (uint64_t)every) == 0;
            hipEvent_t t0 = nullptr;
            if (timed) t0 = e->prof.begin(s);
            launch_step_mt(th.d, B[i & 1], B[(i + 1) & 1], ec, sp, i == 0 ? 1 : 0, 0, s);
            if (timed) { e->prof.end(t0, RG_TREE, s); e->stats.tree_launches_timed += 1; }
            e->stats.tree_launches += 1;
            net_forward(e, net, B[(i + 1) & 1], rows_hint, s, rows_typ, timed);
        }
        launch_step_mt(th.d, B[steps & 1], B[(steps + 1) & 1], ec, sp, steps == 0 ? 1 : 0, 1, s);
        return;
    }
    int i = 0;
    // A search is a chain of num_sims x ~8 dependent launches; on small batches (the arena, single trees, the drain of a self-play
    // call) the HOST's launch calls, not the kernels, set its pace.  Every simulation step takes the same arguments (the batches
    // ping-pong with the step's parity), so S steps (S even) are captured once into a hipGraph and replayed; the graph is kept with
    // the tree arena and re-captured only when something that shapes a launch changes.
    const int S = e->search_graph;
    // ... and only there: on big batches the kernels set the pace, and a graph's power-of-two grids and tile estimates cost more than its
    // launches save (measured in round 4: 9.90 s per 65536-episode step with graphs everywhere, 9.64 s launched one by one)
    const int expect_rows = rows_typ > 0 ? std::min(rows_typ, rows_hint) : rows_hint;
    if (S >= 2 && !e->prof.on && num_sims >= S && expect_rows <= e->search_graph_rows) {
        // the grids' bound and the tile estimate in powers of two: the graph survives from move to move (a larger bound only adds
        // workgroups that exit at once; the estimate only picks tile families)
        auto pow2_up = [](int x, int cap) { int p = 1; while (p < x) p <<= 1; return p < cap ? p : cap; };
        rows_hint = pow2_up(rows_hint, th.d.G * T);
        if (rows_typ > 0) rows_typ = pow2_up(rows_typ, rows_hint);
        struct Key {
            const void *th, *conv, *ws, *stream, *root_states, *max_rows, *ec_key, *ec_stat, *log_state, *log_row;
            unsigned long long ec_tag, salt;
            int kind, rows_hint, rows_typ, S, dedup, mirror, block4, log_cap;
            uint32_t ec_bmask, ec_stones, max_depth, reserve_nodes;
            uint64_t model_gen;
            float cpuct;
            NetOptions opt;
            RootMove move;                             // TreeDev travels by value: a graph captured with other root-move arguments is never replayed
        } k;
        std::memset(&k, 0, sizeof k);
        k.th = &th; k.conv = net.conv; k.ws = net.kind == AZ_NET_CONV ? workspace_for(e, s) : nullptr; k.stream = s; k.root_states = d_root_states;
        k.max_rows = d_max_rows; k.ec_key = ec.key; k.ec_stat = ec.stat; k.log_state = th.d.log_state; k.log_row = th.d.log_row;
        k.ec_tag = ec.tag; k.salt = net.salt; k.kind = net.kind; k.rows_hint = rows_hint; k.rows_typ = rows_typ; k.S = S; k.dedup = dedup ? 1 : 0;
        k.mirror = B[0].mirror;                    // EvalBatch travels by value too
        k.block4 = th.d.block4; k.log_cap = th.d.log_cap; k.ec_bmask = ec.bmask; k.ec_stones = ec.max_stones; k.max_depth = sp.max_depth; k.cpuct = sp.cpuct_f;
        k.opt = netopt_for(e, net);
        k.move = th.d.move;
        k.reserve_nodes = th.d.reserve_nodes;      // TreeDev travels by value into the captured launches: the capacity threshold is baked in
        k.model_gen = net.generation;              // a freed and re-created model may reuse the ConvNet's address: its weights' identity is the generation
        TreeHost::StepGraph& sg = th.step_graph;
        if (!sg.exec || sg.key.size() != sizeof k || std::memcmp(sg.key.data(), &k, sizeof k) != 0) {
            if (sg.exec) { HIPCHK(hipStreamSynchronize(s)); (void)hipGraphExecDestroy(sg.exec); sg.exec = nullptr; }
            if (net.kind == AZ_NET_CONV) convnet_prepare(workspace_for(e, s), k.opt);      // nothing may allocate while the stream is capturing
            hipGraph_t g = nullptr;
            HIPCHK(hipStreamBeginCapture(s, hipStreamCaptureModeRelaxed));
            try {
                for (int j = 0; j < S; ++j) {
                    launch_backup_select(th.d, B[j & 1], B[(j + 1) & 1], ec, sp, s);
                    net_forward(e, net, B[(j + 1) & 1], rows_hint, s, rows_typ, false);
                }
            } catch (...) {                            // never leave the engine's stream capturing: the next call on the handle would fail obscurely
                hipGraph_t dead = nullptr;
                (void)hipStreamEndCapture(s, &dead);
                if (dead) (void)hipGraphDestroy(dead);
                (void)hipGetLastError();
                throw;
            }
            HIPCHK(hipStreamEndCapture(s, &g));
            const hipError_t ie = hipGraphInstantiate(&sg.exec, g, nullptr, nullptr, 0);
            (void)hipGraphDestroy(g);
            if (ie != hipSuccess) { sg.exec = nullptr; throw HipFail{ie, "hipGraphInstantiate"}; }
            sg.key.assign((const unsigned char*)&k, (const unsigned char*)&k + sizeof k);
        }
        for (; i + S <= num_sims; i += S) {
            HIPCHK(hipGraphLaunch(sg.exec, s));
            e->stats.tree_launches += (uint64_t)S;
        }
    }
    for (; i < num_sims; ++i) {
        const bool timed = e->prof.on && (e->profile_tick++ % (uint64_t)every) == 0;
        hipEvent_t t0 = nullptr;
        if (timed) t0 = e->prof.begin(s);
        launch_backup_select(th.d, B[i & 1], B[(i + 1) & 1], ec, sp, s);
        if (timed) { e->prof.end(t0, RG_TREE, s); e->stats.tree_launches_timed += 1; }
        e->stats.tree_launches += 1;
        net_forward(e, net, B[(i + 1) & 1], rows_hint, s, rows_typ, timed);
    }
    launch_backup(th.d, B[num_sims & 1], ec, s);
}

void resolve_profile(az_engine* e) {
    if (!e->prof.on) return;
    double ms[RG_COUNT] = {0, 0};
    e->prof.resolve(ms);
    e->stats.tree_ms += ms[RG_TREE];
    for (NetWorkspace* w : e->ws) netws_resolve_profile(w, &e->netprof);
}

void fold_tree_totals(az_engine* e, const unsigned long long* h, bool dedup);
// fold the per-tree counters into the engine stats and clear them (k_harvest sums on the device)
// fold the decided-move stop's device counters into the engine (after the call's launches; one blocking copy, only while the switch is on)
void fold_stop(az_engine* e) {
    if (!e->search_stop || !e->stop_stat) return;
    unsigned long long h[SS_COUNT];
    HIPCHK(hipMemcpy(h, e->stop_stat, sizeof h, hipMemcpyDeviceToHost));
    HIPCHK(hipMemset(e->stop_stat, 0, sizeof h));
    for (int i = 0; i < SS_COUNT; ++i) e->stop_totals[i] += h[i];
}
void harvest_stats(az_engine* e, TreeHost& th, const NetModel& net) {
    harvest_dedup(e);
    fold_stop(e);
    const bool dedup = dedup_applies(e, net);
    launch_harvest(th.d, th.d_totals, th.d_counts, e->stream);
    unsigned long long h[ST_TOTALS];
    HIPCHK(hipMemcpyAsync(h, th.d_totals, sizeof h, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipMemsetAsync(th.d_totals, 0, sizeof h, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    fold_tree_totals(e, h, dedup);
}
void fold_tree_totals(az_engine* e, const unsigned long long* h, bool dedup) {
    e->stats.simulations += h[ST_SIMS];
    e->stats.expansions += h[ST_EXPANSIONS];
    e->stats.leaf_evals += h[ST_LEAF_EVALS];
    if (!dedup) { e->stats.leaf_rows_requested += h[ST_LEAF_EVALS]; e->stats.leaf_rows_executed += h[ST_LEAF_EVALS]; }
    e->stats.link_hits += h[ST_LINK_HITS];
    e->stats.terminal_hits += h[ST_TERMINAL_HITS];
    e->stats.depth_sum += h[ST_DEPTH_SUM];
    e->stats.abandoned_sims += h[ST_ABANDONED];
    // algorithmic tree bytes per simulation, SURVEY.md 8(d): 128 per selection level + 356 per expansion
    e->stats.tree_bytes += 128.0 * (double)h[ST_DEPTH_SUM] + 356.0 * (double)h[ST_SIMS];
}

az_status report_tree_errors(az_engine* e, TreeHost& th, const uint32_t* h);
az_status check_tree_errors(az_engine* e, TreeHost& th) {
    uint32_t h[ERR_COUNT];
    HIPCHK(hipMemcpy(h, th.d.err, sizeof h, hipMemcpyDeviceToHost));
    return report_tree_errors(e, th, h);
}
az_status report_tree_errors(az_engine* e, TreeHost& th, const uint32_t* h) {
    if (h[ERR_CAPACITY] || h[ERR_HASH_FULL] || h[ERR_PATH] || h[ERR_TERMINAL_ROOT])
        HIPCHK(hipMemset(th.d.err, 0, ERR_COUNT * sizeof(uint32_t)));
    if (h[ERR_CAPACITY]) return fail(e, AZ_ERR_CAPACITY, "node arena exhausted (reserve too small; src/node.rs:237)");
    if (h[ERR_HASH_FULL]) return fail(e, AZ_ERR_CAPACITY, "transposition table full");
    if (h[ERR_PATH]) return fail(e, AZ_ERR_CAPACITY, "node_path overflow");
    if (h[ERR_TERMINAL_ROOT]) return fail(e, AZ_ERR_TERMINAL_ROOT, "get_action_prob on a finished game (src/async_mcts.rs:85)");
    return AZ_OK;
}

az_status find_net(az_engine* e, int model_id, NetModel** out) {
    auto it = e->nets.find(model_id);
    if (it == e->nets.end() || it->second.kind < 0) return fail(e, AZ_ERR_NO_MODEL, "model id not initialised");
    *out = &it->second;
    return AZ_OK;
}
// the conv net's activation workspace is sized by az_config.max_batch: a tree batch may not exceed it
az_status check_batch(az_engine* e, const NetModel& net, int trees) {
    if (net.kind == AZ_NET_CONV && trees > e->cfg.max_batch)
        return fail(e, AZ_ERR_BAD_ARGUMENT, "concurrent trees exceed az_config.max_batch (conv net workspace)");
    return AZ_OK;
}

// Is a caller-supplied pointer device (or managed) memory?  Plain host memory is unknown to the runtime: the query fails and the
// sticky error is cleared.
bool on_device(const void* p) {
    if (!p) return false;
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged;
}

// links and child blocks are 20-bit fields of the 16-byte node record (az_tree.h): a tree holds at most 2^20 slots
az_status check_tree_slots(az_engine* e, uint64_t blocks) {
    if (blocks * (uint64_t)BLOCK_SLOTS > (uint64_t)MAX_TREE_SLOTS)
        return fail(e, AZ_ERR_CAPACITY, "a tree of more than 2^20 node slots: num_sims x plies exceeds what the node record's 20-bit links address");
    return AZ_OK;
}

struct ScopedTimer {
    az_engine* e;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    ~ScopedTimer() {
        e->stats.device_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
};

void set_slot_error(SharedTrees& sh, int slot, const std::string& msg) {
    std::snprintf(sh.err[(size_t)slot].data(), SLOT_ERR_LEN, "%s", msg.c_str());
}

// The leader's batch: every requested slot searches its own tree in ONE run_search over the tree batch (the others are inactive and
// untouched), then each request gets its own policy, RNG stream and status.  Runs with the combiner unlocked, one leader at a time:
// this is the only place a shared tree makes HIP calls, and the only place it writes e->err / e->stats.
void SlotRunner::operator()(CombineBatch<SlotCall>& b) const {
    az_engine* e = t->e;
    SharedTrees& sh = *t->shared;
    const int n = (int)b.slots.size();
    auto fail_all = [&](az_status st, const std::string& msg) {
        for (int i = 0; i < n; ++i) { b.reqs[i]->status = st; set_slot_error(sh, b.slots[i], msg); }
    };
    NetModel* net;
    if (az_status st = find_net(e, t->model_id, &net)) { fail_all(st, e->err); return; }
    TreeDev& d = t->th.d;
    const int G = d.G;
    if (az_status st = check_batch(e, *net, G * d.T)) { fail_all(st, e->err); return; }
    ScopedTimer timer{e};
    try {
        HIPCHK(hipSetDevice(e->device));
        hipStream_t s = e->stream;
        bool any_reset = false;
        for (int i = 0; i < n; ++i) {
            const SlotCall& c = *b.reqs[i];
            SlotReq& r = sh.h_req[i];
            if (on_device(c.state)) HIPCHK(hipMemcpy(&r.state, c.state, 16, hipMemcpyDeviceToHost));
            else std::memcpy(&r.state, c.state, 16);
            r.seed = c.seed; r.game_id = c.game_id; r.temp = c.temp;
            r.slot = b.slots[i]; r.reset = b.reset[i]; r.pad = 0;
            any_reset = any_reset || b.reset[i];
        }
        HIPCHK(hipMemcpyAsync(sh.d_req, sh.h_req, (size_t)n * sizeof(SlotReq), hipMemcpyHostToDevice, s));
        RootMove mv = root_move_for(e, t->th, t->num_sims, (float)t->cpuct, false);      // the slot calls never search by the Gumbel rule
        if (uses_root_stream(mv)) mv.stream.stream = t->d_noise_streams;                 // each request's own (seed, game_id)
        ScopedRootMove armed;
        armed.install(t->th, mv);
        launch_slot_arm(d, sh.d_req, n, t->d_root_states, sh.d_reset, s, mv.stream.stream ? t->d_noise_streams : nullptr);
        if (any_reset) launch_reset_trees(d, sh.d_reset, s);      // AsyncMcts::default for the slots acquired since their last batch
        SearchParams sp{(uint32_t)t->max_depth, (float)t->cpuct};
        // sized by the whole batch, not by this batch's requests: every batch replays the same captured graph
        prepare_cache(e, dedup_applies(e, *net), (uint64_t)G * ((uint64_t)t->num_sims + 1), s);
        run_search(e, t->th, t->d_root_states, t->num_sims, sp, *net, G);
        launch_slot_root_policy(d, sh.d_req, n, sh.h_out, s);
        launch_harvest(d, t->th.d_totals, t->th.d_counts, s);
        launch_call_readback(t->th.d_totals, e->cache.stat, d.err, t->h_rb, s);
        HIPCHK(hipStreamSynchronize(s));
        resolve_profile(e);
        fold_dedup(e, t->h_rb->dd);
        fold_tree_totals(e, t->h_rb->totals, dedup_applies(e, *net));
        e->stats.moves += (uint64_t)n;
        // a capacity error no request could be blamed for (transposition table, node_path) fails the whole batch
        const uint32_t* err = t->h_rb->err;
        bool blamed = false;
        for (int i = 0; i < n; ++i) blamed = blamed || (sh.h_out[i].status & (1u << ERR_CAPACITY));
        const bool unblamed = !blamed && (err[ERR_CAPACITY] || err[ERR_HASH_FULL] || err[ERR_PATH]);
        auto copy_out = [&](void* dst, const void* src, size_t bytes) {
            if (on_device(dst)) HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
            else std::memcpy(dst, src, bytes);
        };
        for (int i = 0; i < n; ++i) {
            SlotCall& c = *b.reqs[i];
            const SlotOut& o = sh.h_out[i];
            if (unblamed || (o.status & (1u << ERR_CAPACITY))) {
                c.status = AZ_ERR_CAPACITY;
                set_slot_error(sh, b.slots[i], err[ERR_HASH_FULL] ? "transposition table full" : err[ERR_PATH] ? "node_path overflow"
                                                   : "node arena exhausted (reserve too small; src/node.rs:237)");
                continue;
            }
            if (o.status & (1u << ERR_TERMINAL_ROOT)) {
                c.status = AZ_ERR_TERMINAL_ROOT;
                set_slot_error(sh, b.slots[i], "get_action_prob on a finished game (src/async_mcts.rs:85)");
                continue;
            }
            copy_out(c.pi, o.pi, 7 * sizeof(float));
            if (c.counts) copy_out(c.counts, o.counts, 7 * sizeof(uint16_t));
            if (c.q) copy_out(c.q, o.q, 7 * sizeof(float));
            c.status = AZ_OK;
        }
    } catch (const HipFail& f) {
        fail_hip(e, f);
        fail_all(AZ_ERR_HIP, e->err);
    }
}

// out[i][0..7) = what launch(d_game_ids, d_states, d_out) computes for root states[i] on game_ids[i] (az_root_noise_eta, az_gumbel_values):
// the caller's pointers may be host or device memory
template <class Launch>
az_status per_root_values(az_engine* e, const char* who, int32_t n, const uint64_t* game_ids, const uint64_t* states, float* out, Launch launch) {
    if (!e) return AZ_ERR_BAD_ARGUMENT;
    if (n < 0 || (n > 0 && (!game_ids || !states || !out))) return fail(e, AZ_ERR_BAD_ARGUMENT, std::string(who) + ": bad argument");
    if (n == 0) return AZ_OK;
    try {
        HIPCHK(hipSetDevice(e->device));
        DeviceMem mem;
        uint64_t* d_ids = mem.alloc<uint64_t>((size_t)n);
        ulonglong2* d_states = mem.alloc<ulonglong2>((size_t)n);
        float* d_out = mem.alloc<float>((size_t)n * 7);
        HIPCHK(hipMemcpyAsync(d_ids, game_ids, (size_t)n * 8, hipMemcpyDefault, e->stream));
        HIPCHK(hipMemcpyAsync(d_states, states, (size_t)n * 16, hipMemcpyDefault, e->stream));
        launch(d_ids, d_states, d_out);
        HIPCHK(hipMemcpyAsync(out, d_out, (size_t)n * 7 * sizeof(float), hipMemcpyDefault, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        return AZ_OK;
    } catch (const HipFail& f) { return fail_hip(e, f); }
}

}  // namespace

// =============================================================================================
extern "C" {

az_status az_create(const az_config* cfg, az_engine** out) {
    if (!out) return AZ_ERR_BAD_ARGUMENT;
    *out = nullptr;
    std::unique_ptr<az_engine> e(new az_engine());
    if (cfg) e->cfg = *cfg;
    if (e->cfg.max_batch <= 0) e->cfg.max_batch = 8192;
    if (e->cfg.net_channels <= 0) e->cfg.net_channels = 512;
    if (e->cfg.game < 0 || e->cfg.game >= GAME_COUNT) return AZ_ERR_BAD_ARGUMENT;
    e->device = e->cfg.device;
    e->prof.on = e->cfg.profile != 0;
    try {
        int n = 0;
        HIPCHK(hipGetDeviceCount(&n));
        if (n <= 0 || e->device >= n) return AZ_ERR_HIP;
        HIPCHK(hipSetDevice(e->device));
        HIPCHK(hipStreamCreate(&e->stream));
    } catch (const HipFail&) {
        return AZ_ERR_HIP;
    }
    *out = e.release();
    return AZ_OK;
}

void az_destroy(az_engine* e) {
    if (!e) return;
    (void)hipSetDevice(e->device);
    (void)hipStreamSynchronize(e->stream);
    (void)az_selfplay_end(e);
    for (auto& kv : e->nets) if (kv.second.conv) convnet_destroy(kv.second.conv);
    if (e->val_model.conv) convnet_destroy(e->val_model.conv);
    for (NetWorkspace* w : e->ws) netws_destroy(w);
    if (e->cache_keys) (void)hipFree(e->cache_keys);
    if (e->cache_pv) (void)hipFree(e->cache_pv);
    if (e->comm && g_rccl.CommDestroy) { (void)g_rccl.CommDestroy(e->comm); e->comm = nullptr; }
    if (e->local) { e->local->leave(e->comm_rank); e->local.reset(); }       // the peers' collectives fail from now on
    e->tree_pool.clear();
    trainer_destroy(e->trainer);
    { double ms[RG_COUNT] = {0, 0}; e->prof.resolve(ms); }
    for (hipStream_t ss : e->side) if (ss) (void)hipStreamDestroy(ss);
    (void)hipStreamDestroy(e->stream);
    delete e;
}

const char* az_last_error(const az_engine* e) { return e ? e->err.c_str() : "null engine"; }

az_status az_set_option(az_engine* e, const char* key, int64_t value) {
    if (!e || !key) return AZ_ERR_BAD_ARGUMENT;
    auto is = [&](const char* k) { return std::strcmp(key, k) == 0; };
    // an open self-play session captured these at begin or reads them while it plays (the evaluation cache's shape, which rows go through
    // it, the driver and its schedule, conv2's rounding): no value of them is taken until az_selfplay_end
    if (e->sp_session)
        for (const char* k : {"conv2_table", "eval_dedup", "eval_cache_log2", "eval_cache_persist", "eval_cache_max_stones", "selfplay_async",
                              "selfplay_async_launches", "selfplay_async_iters"})
            if (is(k)) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_set_option: " + std::string(k) + " cannot change while a self-play session is open");
    // ---- options of the shipped library: every one of them lives in THIS engine ----
    if (is("conv2_table") && (value == 0 || value == 1)) {
        if (value == 0 && e->netopt.net_fp8) return fail(e, AZ_ERR_BAD_ARGUMENT, "conv2_table = 0 is not available while net_fp8 is 1 (the fp8 class takes conv2 from the table kernel)");
        if (value == 0)
            for (const auto& kv : e->nets)
                if (kv.second.kind == AZ_NET_CONV && effective_class(e, kv.second))
                    return fail(e, AZ_ERR_BAD_ARGUMENT, "conv2_table = 0 is not available while model " + std::to_string(kv.first) + " is of the fp8 class (it takes conv2 from the table kernel)");
        if ((int)value == e->netopt.conv2_table) return AZ_OK;
        e->netopt.conv2_table = (int)value;
        for (auto& kv : e->nets) {
            NetModel& m = kv.second;
            if (m.kind != AZ_NET_CONV) continue;
            m.cache_tag = 0;                                      // the table set and the GEMM set round differently: a persistent cache never serves the other one's rows
            m.generation = ++g_model_generation;
        }
        return AZ_OK;
    }
    if (is("net_fp8") && (value == 0 || value == 1)) {
        if (e->sp_session) return fail(e, AZ_ERR_BAD_ARGUMENT, "net_fp8 cannot change while a self-play session is open");
        if (value == 1 && e->netopt.conv2_table != 1) return fail(e, AZ_ERR_BAD_ARGUMENT, "net_fp8 needs conv2_table = 1");
        if ((int)value == e->netopt.net_fp8) return AZ_OK;
        try {
            HIPCHK(hipSetDevice(e->device));
            e->netopt.net_fp8 = (int)value;
            for (auto& kv : e->nets) {
                NetModel& m = kv.second;
                if (m.kind != AZ_NET_CONV || m.klass != AZ_NET_CLASS_ENGINE) continue;      // a pinned model keeps its class, its tag and its graphs
                const az_status st = fp8_sync_model(e, m);
                if (st) { e->netopt.net_fp8 = 0; return st; }
                m.cache_tag = 0;                                  // the other class's cached rows and captured graphs are never used again
                m.generation = ++g_model_generation;
            }
            return AZ_OK;
        } catch (const HipFail& f) { e->netopt.net_fp8 = 0; return fail_hip(e, f); }
    }
    if (is("eval_mirror")) {
        if (value != 0 && value != 1) return fail(e, AZ_ERR_BAD_ARGUMENT, "eval_mirror must be 0 or 1");
        if (e->sp_session) return fail(e, AZ_ERR_BAD_ARGUMENT, "eval_mirror cannot change while a self-play session is open");
        if ((int)value == e->eval_mirror) return AZ_OK;
        e->eval_mirror = (int)value;
        for (auto& kv : e->nets) {
            NetModel& m = kv.second;
            if (m.kind != AZ_NET_CONV) continue;
            m.cache_tag = 0;                                      // the other class's cached rows (raw N(s) against raw N(c(s))) and captured graphs are never used again
            m.generation = ++g_model_generation;
        }
        return AZ_OK;
    }
    // the root-move keys (root_move_for): one range per key, fixed for the life of a self-play session
    struct RootMoveKey { const char* key; int64_t lo, hi; bool or_zero; int64_t az_engine::* field; const char* range; };
    static const RootMoveKey root_move_keys[] = {
        {"root_noise_eps_e6", 0, 1000000, false, &az_engine::root_noise_eps_e6, "root_noise_eps_e6 must be in 0 .. 1000000"},
        {"root_noise_alpha_e6", 50000, 100000000, false, &az_engine::root_noise_alpha_e6, "root_noise_alpha_e6 must be in 50000 .. 100000000"},
        {"playout_cap_sims", 0, PLAYOUT_CAP_MAX_SIMS, false, &az_engine::playout_cap_sims, "playout_cap_sims must be in 0 .. 65535"},
        {"playout_cap_full_e6", 0, PLAYOUT_CAP_E6, false, &az_engine::playout_cap_full_e6, "playout_cap_full_e6 must be in 0 .. 1000000"},
        {"forced_playouts_k_e6", 0, FORCED_K_E6_MAX, false, &az_engine::forced_playouts_k_e6, "forced_playouts_k_e6 must be in 0 .. 16000000"},
        {"policy_prune", 0, 1, false, &az_engine::policy_prune, "policy_prune must be 0 or 1"},
        {"gumbel_m", GUMBEL_M_MIN, GUMBEL_M_MAX, true, &az_engine::gumbel_m, "gumbel_m must be 0 or in 2 .. 7"},
        {"gumbel_c_visit_e6", 0, GUMBEL_C_VISIT_E6_MAX, false, &az_engine::gumbel_c_visit_e6, "gumbel_c_visit_e6 must be in 0 .. 1000000000"},
        {"selfplay_record_search", 0, 1, false, &az_engine::selfplay_record_search, "selfplay_record_search must be 0 or 1"},
        {"gumbel_c_scale_e6", GUMBEL_C_SCALE_E6_MIN, GUMBEL_C_SCALE_E6_MAX, false, &az_engine::gumbel_c_scale_e6, "gumbel_c_scale_e6 must be in 1 .. 100000000"},
    };
    for (const RootMoveKey& r : root_move_keys) {
        if (!is(r.key)) continue;
        if ((value < r.lo || value > r.hi) && !(r.or_zero && value == 0)) return fail(e, AZ_ERR_BAD_ARGUMENT, r.range);
        if (e->sp_session) return fail(e, AZ_ERR_BAD_ARGUMENT, std::string(r.key) + " cannot change while a self-play session is open");
        e->*r.field = value;
        return AZ_OK;
    }
    if (is("arena_opening_plies")) {
        if (value < 0 || value > OPENING_MAX_PLIES || (value & 1)) return fail(e, AZ_ERR_BAD_ARGUMENT, "arena_opening_plies must be 0 or an even value in 2 .. 12");
        e->arena_opening_plies = value;
        return AZ_OK;
    }
    if (is("conv3_small") && (value == 0 || value == 1)) { e->netopt.conv3_small = (int)value; return AZ_OK; }
    if (is("conv3_tail") && (value == 0 || value == 1)) { e->netopt.conv3_tail = (int)value; return AZ_OK; }
    if (is("ring_packed") && (value == 0 || value == 1)) { e->netopt.ring_packed = (int)value; return AZ_OK; }
    if (is("conv3_planes") && (value == 0 || value == 1)) { e->netopt.conv3_planes = (int)value; return AZ_OK; }
    if (is("conv3_wreg") && (value == 0 || value == 1)) { e->netopt.conv3_wreg = (int)value; return AZ_OK; }
    if (is("narrow_rows") && value >= 0 && value <= 65536) { e->netopt.narrow_rows = (int)value; return AZ_OK; }
    if (is("tree_block4") && (value == 0 || value == 1)) { e->tree_block4 = (int)value; return AZ_OK; }
    if (is("dedup_stats") && (value == 0 || value == 1)) { e->dedup_stats = (int)value; return AZ_OK; }
    if (is("profile_every") && value >= 1 && value <= 1000000) { e->profile_every = (int)value; return AZ_OK; }
    // the HIP-event brackets of az_config.profile, switched between calls: a timed region runs un-bracketed (its search loop as
    // hipGraph launches), a separate pass of the same call with the brackets on gives the per-kernel times
    if (is("profile") && (value == 0 || value == 1)) { e->prof.on = value != 0; return AZ_OK; }
    if (is("search_graph") && value >= 0 && value <= 1000 && value % 2 == 0) { e->search_graph = (int)value; return AZ_OK; }
    if (is("search_graph_rows") && value >= 0 && value <= 1000000) { e->search_graph_rows = (int)value; return AZ_OK; }
    if (is("selfplay_async") && (value == 0 || value == 1)) { e->selfplay_async = (int)value; return AZ_OK; }
    if (is("selfplay_async_launches") && value >= 1 && value <= 8) { e->selfplay_async_launches = (int)value; return AZ_OK; }
    if (is("selfplay_async_iters") && value >= 2 && value <= 64) { e->selfplay_async_iters = (int)value; return AZ_OK; }
    if (is("fused_search") && (value == 0 || value == 1)) { e->fused_search = (int)value; return AZ_OK; }
    if (is("eval_dedup") && value >= 0 && value <= 2) { e->eval_dedup = (int)value; return AZ_OK; }
    if (is("eval_cache_log2") && (value == 0 || (value >= 10 && value <= 30))) { e->eval_cache_log2 = (int)value; return AZ_OK; }
    if (is("eval_cache_max_stones") && value >= 0 && value <= 42) { e->eval_cache_max_stones = (int)value; return AZ_OK; }
    if (is("eval_cache_persist") && (value == 0 || value == 1)) { e->eval_cache_persist = (int)value; return AZ_OK; }
    // NNet::train hyper-parameters (defaults = connect_four_net.py:13-15, :21)
    if (is("train_epochs") && value >= 1 && value <= 100000) { e->train_epochs = (int)value; return AZ_OK; }
    if (is("train_batch") && value >= 2 && value <= TRAIN_MAX_BATCH) { e->train_batch = (int)value; return AZ_OK; }
    if (is("train_seed")) { e->train_seed = (uint64_t)value; return AZ_OK; }
    if (is("train_graph") && (value == 0 || value == 1)) { e->train_graph = (int)value; if (e->trainer) trainer_set_graph(e->trainer, value != 0); return AZ_OK; }
    // the route switches of a step (csrc/az_train_plan.h), each 0 / 1; a live trainer takes the record at once ("train_fork" may create its
    // second stream: on the engine's device)
    struct SwitchKey { const char* key; int TrainSwitches::* field; };
    static const SwitchKey switch_keys[] = {
        {"train_gemm", &TrainSwitches::gemm},
        {"train_fwd_dma", &TrainSwitches::fwd_dma},
        {"train_fwd_x3", &TrainSwitches::fwd_x3},
        {"train_wgrad_tr", &TrainSwitches::wgrad_tr},
        {"train_implicit", &TrainSwitches::implicit},
        {"train_gemm3_ring", &TrainSwitches::gemm3_ring},
        {"train_fork", &TrainSwitches::fork},
    };
    for (const SwitchKey& r : switch_keys) {
        if (!is(r.key) || (value != 0 && value != 1)) continue;
        e->train_sw.*r.field = (int)value;
        if (e->trainer) { (void)hipSetDevice(e->device); trainer_set_switches(e->trainer, e->train_sw); }
        return AZ_OK;
    }
    if (is("train_lr_e9") && value > 0) { e->hyper.lr = (float)((double)value * 1e-9); return AZ_OK; }
    if (is("train_dropout_e6") && value >= 0 && value < 1000000) { e->hyper.dropout = (float)((double)value * 1e-6); return AZ_OK; }
    // per-epoch validation (csrc/az_score.h): read when az_net_train / az_net_train_samples begin
    if (is("train_keep_best") && (value == 0 || value == 1)) { e->train_keep_best = value; return AZ_OK; }
    if (is("train_patience")) {
        if (value < 0 || value > SCORE_MAX_PATIENCE) return fail(e, AZ_ERR_BAD_ARGUMENT, "train_patience must be in 0 .. 1000");
        e->train_patience = value;
        return AZ_OK;
    }
    // the opt-in optimiser rules (csrc/az_optim.h): one range per key, read by the next az_net_train_begin
    struct OptimKey { const char* key; int64_t lo, hi; bool or_zero; int64_t az_engine::* field; const char* range; };
    static const OptimKey optim_keys[] = {
        {"train_weight_decay_e9", 0, OPTIM_WD_E9_MAX, false, &az_engine::train_weight_decay_e9, "train_weight_decay_e9 must be in 0 .. 1000000000"},
        {"train_clip_norm_e6", 1, OPTIM_CLIP_E6_MAX, true, &az_engine::train_clip_norm_e6, "train_clip_norm_e6 must be 0 or in 1 .. 1000000000000"},
        {"train_lr_warmup_steps", 0, OPTIM_STEPS_MAX, false, &az_engine::train_lr_warmup_steps, "train_lr_warmup_steps must be in 0 .. 2147483647"},
        {"train_lr_decay", 0, 2, false, &az_engine::train_lr_decay, "train_lr_decay must be 0, 1 or 2"},
        {"train_lr_floor_e6", 0, OPTIM_FLOOR_E6_MAX, false, &az_engine::train_lr_floor_e6, "train_lr_floor_e6 must be in 0 .. 1000000"},
        {"train_lr_total_steps", 0, OPTIM_STEPS_MAX, false, &az_engine::train_lr_total_steps, "train_lr_total_steps must be in 0 .. 2147483647"},
        {"train_ema_decay_e9", 1, OPTIM_EMA_E9_MAX, true, &az_engine::train_ema_decay_e9, "train_ema_decay_e9 must be 0 or in 1 .. 999999999"},
    };
    for (const OptimKey& r : optim_keys) {
        if (!is(r.key)) continue;
        if ((value < r.lo || value > r.hi) && !(r.or_zero && value == 0)) return fail(e, AZ_ERR_BAD_ARGUMENT, r.range);
        e->*r.field = value;
        return AZ_OK;
    }
#ifdef AZ_DIAG
    // ---- libaz_engine_diag.so only: superseded kernel generations, forced tiles, clock-stamp builds (every one bit-identical to the shipped kernels) ----
    NetOptions& o = e->netopt;
    if (is("conv2_table") && value == 2) { o.conv2_table = 2; return AZ_OK; }
    if (is("gemm_variant") && (value == 0 || value == 1 || value == 2 || value == 3 || value == 5 || value == 13)) { o.gemm_variant = (int)value; return AZ_OK; }
    if (is("fc_ring") && value >= 0 && value <= 3) { o.fc_ring = (int)value; return AZ_OK; }
    if (is("ring_tile") && value >= 0 && value < 60000) { const int l = (int)(value / 10000); if (l >= 3 && l <= 5) o.ring_tile[l] = (int)(value % 10000); return AZ_OK; }
    if (is("conv3_ring") && value >= 0 && value <= 3) { o.conv3_ring = (int)value; return AZ_OK; }
    if (is("conv2_pipe") && (value == 0 || value == 1)) { o.conv2_pipe = (int)value; return AZ_OK; }
    if (is("conv3_pipe") && value >= 0 && value <= 3) { o.conv3_pipe = (int)value; return AZ_OK; }
    if (is("conv1_table") && (value == 0 || value == 1)) { o.conv1_table = (int)value; return AZ_OK; }
    if (is("conv4_big") && value >= 0 && value <= 2) { o.conv4_big = (int)value; return AZ_OK; }
    if (is("tree_stamps") && (value == 0 || value == 1)) { return tree_set_stamps((int)value) ? AZ_OK : fail(e, AZ_ERR_HIP, "tree_set_stamps"); }
    if (is("print_clock_stamps")) {
        // gemm_variant 13: median in-kernel clock of conv2's K loop for model `value`
        auto it = e->nets.find((int)value);
        std::vector<unsigned long long> st(2048);
        if (it == e->nets.end() || !it->second.conv || !netws_read_clock_stamps(e->ws[0], st.data()))
            return fail(e, AZ_ERR_BAD_ARGUMENT, "no conv net under that model id");
        std::vector<double> mhz;
        for (int i = 0; i < 1024; ++i) if (st[2 * i + 1]) mhz.push_back(100.0 * (double)st[2 * i] / (double)st[2 * i + 1]);
        std::sort(mhz.begin(), mhz.end());
        if (mhz.empty()) return fail(e, AZ_ERR_BAD_ARGUMENT, "no stamps (run a forward with gemm_variant 13 first)");
        char buf[160];
        std::snprintf(buf, sizeof buf, "clock MHz min %.0f median %.0f max %.0f over %zu blocks", mhz.front(), mhz[mhz.size() / 2], mhz.back(), mhz.size());
        e->err = buf;       // returned through az_last_error
        return AZ_OK;
    }
    if (is("print_seg_stamps")) {
        // conv3_pipe 3: per-segment cycle sums of wave 0 of the first 128 workgroups of the last conv3 launch, median over blocks
        std::vector<unsigned long long> st(2048);
        if (!e->ws[0] || !netws_read_clock_stamps(e->ws[0], st.data())) return fail(e, AZ_ERR_BAD_ARGUMENT, "no workspace");
        std::string out;
        for (int i = 0; i < 10; ++i) {
            std::vector<unsigned long long> v;
            for (int b = 0; b < 128; ++b) if (st[16 * b + 8]) v.push_back(st[16 * b + i]);
            if (v.empty()) return fail(e, AZ_ERR_BAD_ARGUMENT, "no stamps (run a forward with conv3_pipe 3 first)");
            std::sort(v.begin(), v.end());
            char buf[64];
            std::snprintf(buf, sizeof buf, "%s%llu", i ? " " : "", v[v.size() / 2]);
            out += buf;
        }
        e->err = out;
        return AZ_OK;
    }
    if (is("print_tree_stamps")) {
        // "tree_stamps" = 1: cycles per phase of the last k_backup_select launch, median over its waves:
        // load head+path | backup | wait for its stores | select | leaf request | store head+path | whole kernel
        std::vector<unsigned long long> st(4096 * 8);
        if (!tree_read_stamps(st.data())) return fail(e, AZ_ERR_BAD_ARGUMENT, "no stamps (set tree_stamps 1 and run a search first)");
        std::string out;
        for (int i = 0; i < 7; ++i) {
            std::vector<unsigned long long> v;
            for (int w = 0; w < 4096; ++w) if (st[(size_t)w * 8 + 6]) v.push_back(st[(size_t)w * 8 + i]);
            if (v.empty()) return fail(e, AZ_ERR_BAD_ARGUMENT, "no stamps yet");
            std::sort(v.begin(), v.end());
            char buf[96];
            std::snprintf(buf, sizeof buf, "%s%llu/%llu/%llu", i ? " " : "", v[v.size() / 10], v[v.size() / 2], v[v.size() * 9 / 10]);
            out += buf;
        }
        e->err = out;
        return AZ_OK;
    }
#else
    // the diagnostic keys exist in libaz_engine_diag.so only; their DEFAULT value is accepted here so that a caller resetting them is not an error
    static const struct { const char* k; int64_t dflt; } diag_keys[] = {{"gemm_variant", 5}, {"fc_ring", 1}, {"conv3_ring", 0}, {"conv2_pipe", 1},
                                                                         {"conv3_pipe", 1}, {"conv1_table", 1}, {"conv4_big", 0}, {"tree_stamps", 0}};
    bool diag_key = is("print_clock_stamps") || is("print_seg_stamps") || is("print_tree_stamps") || (is("conv2_table") && value == 2);
    if (is("ring_tile")) { if (value >= 30000 && value < 60000 && value % 10000 == 0) return AZ_OK; diag_key = true; }
    for (const auto& dk : diag_keys)
        if (is(dk.k)) { if (value == dk.dflt) return AZ_OK; diag_key = true; }
    if (diag_key)
        return fail(e, AZ_ERR_BAD_ARGUMENT, std::string(key) + ": diagnostic option or value (superseded kernels and clock stamps live in libaz_engine_diag.so)");
#endif
    return fail(e, AZ_ERR_BAD_ARGUMENT, std::string("unknown option or value: ") + key);
}

az_status az_get_stats(az_engine* e, az_stats* out) {
    if (!e || !out) return AZ_ERR_BAD_ARGUMENT;
    *out = e->stats;
    out->net_launches = e->netprof.launches;
    out->net_conv2_ms = e->netprof.conv2_ms;
    out->net_conv2_flops = e->netprof.conv2_flops;
    out->net_total_ms = e->netprof.total_ms;
    out->net_total_flops = e->netprof.total_flops;
    out->net_conv3_ms = e->netprof.conv3_ms;
    out->net_conv3_flops = e->netprof.conv3_flops;
    out->net_conv2_bytes = e->netprof.conv2_bytes;
    out->net_conv4_ms = e->netprof.conv4_ms;
    out->net_conv4_flops = e->netprof.conv4_flops;
    out->net_fc_ms = e->netprof.fc_ms;
    out->net_fc_flops = e->netprof.fc_flops;
    out->net_rows_timed = e->netprof.rows;
    out->tree_arena_allocs = e->tree_pool_allocs;
    {
        unsigned long long acct[2] = {0, 0};
        (void)hipSetDevice(e->device);
        for (NetWorkspace* w : e->ws) if (w && !netws_conv3_accounting(w, acct, false)) return fail(e, AZ_ERR_HIP, "az_get_stats: reading the conv3 accounting");
        out->net_conv3_image_rows = acct[0];
        out->net_conv3_image_launches = acct[1];
    }
    return AZ_OK;
}
az_status az_reset_stats(az_engine* e) {
    if (!e) return AZ_ERR_BAD_ARGUMENT;
    e->stats = az_stats{};
    e->netprof = NetProfile{};
    unsigned long long sink[2] = {0, 0};
    (void)hipSetDevice(e->device);
    for (NetWorkspace* w : e->ws) if (w && !netws_conv3_accounting(w, sink, true)) return fail(e, AZ_ERR_HIP, "az_reset_stats: clearing the conv3 accounting");
    return AZ_OK;
}

// ---- NNet ------------------------------------------------------------------------------------
az_status az_net_set_kind(az_engine* e, int32_t model_id, az_net_kind kind, uint64_t salt) {
    if (!e || (kind != AZ_NET_STUB && kind != AZ_NET_HASH)) return fail(e, AZ_ERR_BAD_ARGUMENT, "kind must be STUB or HASH");
    if (az_status sr = session_model_refusal(e, "az_net_set_kind", model_id)) return sr;
    NetModel& m = e->nets[model_id];
    m.kind = kind;
    // two hash nets with the same salt but different model ids differ (oracle: HashNet::predict)
    m.salt = salt + (uint64_t)model_id * 0x51ED27ull;
    m.cache_tag = 0;
    m.generation = ++g_model_generation;
    return AZ_OK;
}

static az_status ensure_conv(az_engine* e, int32_t model_id, NetModel** out) {
    NetModel& m = e->nets[model_id];
    if (!m.conv) {
        const char* why = nullptr;
        m.conv = convnet_create(e->cfg.net_channels, &why);
        if (!m.conv) return fail(e, AZ_ERR_HIP, why ? why : "convnet_create failed");
    }
    *out = &m;
    return AZ_OK;
}

az_status az_net_free(az_engine* e, int32_t model_id) {
    if (!e) return AZ_ERR_BAD_ARGUMENT;
    auto it = e->nets.find(model_id);
    if (it == e->nets.end()) return fail(e, AZ_ERR_NO_MODEL, "model id not initialised");
    if (az_status sr = session_model_refusal(e, "az_net_free", model_id)) return sr;      // the session holds a pointer to it
    (void)hipSetDevice(e->device);
    (void)hipStreamSynchronize(e->stream);
    if (it->second.conv) convnet_destroy(it->second.conv);
    e->nets.erase(it);          // its evaluation-cache entries die with its tag
    return AZ_OK;
}

az_status az_net_set_class(az_engine* e, int32_t model_id, int32_t c) {
    if (!e) return AZ_ERR_BAD_ARGUMENT;
    if (c != AZ_NET_CLASS_ENGINE && c != AZ_NET_CLASS_BF16 && c != AZ_NET_CLASS_FP8) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_net_set_class: the class must be ENGINE, BF16 or FP8");
    auto it = e->nets.find(model_id);
    if (it == e->nets.end()) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_net_set_class: model id not initialised");
    NetModel& m = it->second;
    if (m.kind != AZ_NET_CONV || !m.conv) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_net_set_class: the stub / hash nets have no numerics class");
    if ((int)c == m.klass) return AZ_OK;
    if (e->sp_session) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_net_set_class: a model's class cannot change while a self-play session is open");
    if (c == AZ_NET_CLASS_FP8 && e->netopt.conv2_table != 1) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_net_set_class: the fp8 class needs conv2_table = 1");
    const int before = effective_class(e, m), stored = m.klass;
    m.klass = (int)c;
    if (effective_class(e, m) == before) return AZ_OK;          // the same kernels as before: the tag and the captured graphs stay good
    try {
        HIPCHK(hipSetDevice(e->device));
        const az_status st = fp8_sync_model(e, m);
        if (st) { m.klass = stored; return st; }
        m.cache_tag = 0;                                          // the other class's cached rows and captured graphs are never used again
        m.generation = ++g_model_generation;
        return AZ_OK;
    } catch (const HipFail& f) { m.klass = stored; return fail_hip(e, f); }
}

az_status az_net_get_class(az_engine* e, int32_t model_id, int32_t* stored, int32_t* effective) {
    if (!e) return AZ_ERR_BAD_ARGUMENT;
    auto it = e->nets.find(model_id);
    if (it == e->nets.end()) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_net_get_class: model id not initialised");
    if (it->second.kind != AZ_NET_CONV) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_net_get_class: the stub / hash nets have no numerics class");
    if (stored) *stored = it->second.klass;
    if (effective) *effective = effective_class(e, it->second);
    return AZ_OK;
}

az_status az_net_init_random(az_engine* e, int32_t model_id, uint64_t seed) {
    if (!e) return AZ_ERR_BAD_ARGUMENT;
    if (az_status sr = session_model_refusal(e, "az_net_init_random", model_id)) return sr;
    try {
        HIPCHK(hipSetDevice(e->device));
        NetModel* m;
        az_status st = ensure_conv(e, model_id, &m);
        if (st) return st;
        convnet_init_random(m->conv, seed);
        m->kind = AZ_NET_CONV;
        m->cache_tag = 0;
        m->generation = ++g_model_generation;
        return fp8_sync_model(e, *m);
    } catch (const HipFail& f) { return fail_hip(e, f); }
}

int64_t az_net_param_count(const az_engine* e) { return e ? convnet_param_count(e->cfg.net_channels) : 0; }

az_status az_net_set_params(az_engine* e, int32_t model_id, const float* params, int64_t n) {
    if (!e || !params) return AZ_ERR_BAD_ARGUMENT;
    if (az_status sr = session_model_refusal(e, "az_net_set_params", model_id)) return sr;
    if (n != convnet_param_count(e->cfg.net_channels)) return fail(e, AZ_ERR_BAD_ARGUMENT, "parameter count mismatch");
    try {
        HIPCHK(hipSetDevice(e->device));
        NetModel* m;
        az_status st = ensure_conv(e, model_id, &m);
        if (st) return st;
        if (!convnet_set_params(m->conv, params, n)) return fail(e, AZ_ERR_HIP, "convnet_set_params failed");
        m->kind = AZ_NET_CONV;
        m->cache_tag = 0;
        m->generation = ++g_model_generation;
        return fp8_sync_model(e, *m);
    } catch (const HipFail& f) { return fail_hip(e, f); }
}

az_status az_net_get_params(az_engine* e, int32_t model_id, float* params, int64_t n) {
    if (!e || !params) return AZ_ERR_BAD_ARGUMENT;
    NetModel* m;
    az_status st = find_net(e, model_id, &m);
    if (st) return st;
    if (m->kind != AZ_NET_CONV) return fail(e, AZ_ERR_BAD_ARGUMENT, "model has no parameters");
    if (!convnet_get_params(m->conv, params, n)) return fail(e, AZ_ERR_BAD_ARGUMENT, "parameter count mismatch");
    return AZ_OK;
}

az_status az_net_save(az_engine* e, int32_t model_id, const char* path) {
    if (!e || !path) return AZ_ERR_BAD_ARGUMENT;
    int64_t n = az_net_param_count(e);
    std::vector<float> p((size_t)n);
    az_status st = az_net_get_params(e, model_id, p.data(), n);
    if (st) return st;
    FILE* f = std::fopen(path, "wb");
    if (!f) return fail(e, AZ_ERR_IO, std::string("cannot write ") + path);
    const char magic[8] = {'A', 'Z', 'N', 'E', 'T', '0', '0', '1'};
    int64_t hdr[2] = {(int64_t)e->cfg.net_channels, n};
    bool ok = std::fwrite(magic, 1, 8, f) == 8 && std::fwrite(hdr, sizeof(int64_t), 2, f) == 2 &&
              std::fwrite(p.data(), sizeof(float), (size_t)n, f) == (size_t)n;
    std::fclose(f);
    return ok ? AZ_OK : fail(e, AZ_ERR_IO, "short write");
}

az_status az_net_load(az_engine* e, int32_t model_id, const char* path) {
    if (!e || !path) return AZ_ERR_BAD_ARGUMENT;
    if (az_status sr = session_model_refusal(e, "az_net_load", model_id)) return sr;
    FILE* f = std::fopen(path, "rb");
    if (!f) return fail(e, AZ_ERR_IO, std::string("cannot read ") + path);
    char magic[8];
    int64_t hdr[2];
    int64_t n = az_net_param_count(e);
    std::vector<float> p((size_t)n);
    bool ok = std::fread(magic, 1, 8, f) == 8 && std::memcmp(magic, "AZNET001", 8) == 0 &&
              std::fread(hdr, sizeof(int64_t), 2, f) == 2 && hdr[0] == e->cfg.net_channels && hdr[1] == n &&
              std::fread(p.data(), sizeof(float), (size_t)n, f) == (size_t)n;
    std::fclose(f);
    if (!ok) return fail(e, AZ_ERR_IO, "bad or mismatching weights file");
    return az_net_set_params(e, model_id, p.data(), n);
}

az_status az_net_predict_states(az_engine* e, int32_t model_id, const uint64_t* states, int32_t B, float* pi, float* v) {
    if (!e || !states || !pi || !v || B < 0) return AZ_ERR_BAD_ARGUMENT;
    NetModel* m;
    az_status st = find_net(e, model_id, &m);
    if (st) return st;
    ScopedTimer timer{e};
    try {
        HIPCHK(hipSetDevice(e->device));
        DeviceMem mem;
        const int chunk = e->cfg.max_batch;
        EvalBatch eb{};
        eb.cap = chunk;
        eb.n = mem.alloc<uint32_t>(1);
        eb.state = mem.alloc<ulonglong2>(chunk);
        eb.pi = mem.alloc<float>((size_t)chunk * 8);
        eb.v = mem.alloc<float>(chunk);
        std::vector<float> hp((size_t)chunk * 8);
        // "eval_mirror": the chunk is canonicalised in place before the forward and its pi rows are un-mirrored after it
        uint8_t* mflags = mirror_applies(e, *m) ? mem.alloc<uint8_t>(chunk) : nullptr;
        for (int b0 = 0; b0 < B; b0 += chunk) {
            uint32_t nb = (uint32_t)std::min(chunk, B - b0);
            HIPCHK(hipMemcpyAsync(eb.n, &nb, sizeof nb, hipMemcpyHostToDevice, e->stream));
            HIPCHK(hipMemcpyAsync(eb.state, states + 2 * (size_t)b0, (size_t)nb * 16, hipMemcpyDefault, e->stream));
            if (mflags) launch_canonicalise(eb.state, mflags, (int)nb, e->stream);
            net_forward(e, *m, eb, (int)nb, e->stream);
            if (mflags) launch_unmirror_rows(eb.pi, mflags, (int)nb, e->stream);
            HIPCHK(hipMemcpyAsync(hp.data(), eb.pi, (size_t)nb * 8 * sizeof(float), hipMemcpyDeviceToHost, e->stream));
            HIPCHK(hipStreamSynchronize(e->stream));
            std::vector<float> packed((size_t)nb * 7);
            for (uint32_t i = 0; i < nb; ++i)
                for (int a = 0; a < 7; ++a) packed[(size_t)i * 7 + a] = hp[(size_t)i * 8 + a];
            HIPCHK(hipMemcpy(pi + (size_t)b0 * 7, packed.data(), packed.size() * sizeof(float), hipMemcpyDefault));
            HIPCHK(hipMemcpy(v + b0, eb.v, (size_t)nb * sizeof(float), hipMemcpyDefault));
        }
        resolve_profile(e);
        return AZ_OK;
    } catch (const HipFail& f) { return fail_hip(e, f); }
}

az_status az_net_predict(az_engine* e, int32_t model_id, const float* boards, int32_t B, float* pi, float* v) {
    if (!e || !boards || B < 0) return AZ_ERR_BAD_ARGUMENT;
    try {
        // [B,2,6,7] f32 planes -> canonical bitboards (the planes are 0/1 by contract, connect_four_game.rs:227-233)
        std::vector<float> hb((size_t)B * AZ_FEATURES);
        HIPCHK(hipMemcpy(hb.data(), boards, hb.size() * sizeof(float), hipMemcpyDefault));
        std::vector<uint64_t> states((size_t)B * 2, 0);
        for (int b = 0; b < B; ++b)
            for (int r = 0; r < 6; ++r)
                for (int c = 0; c < 7; ++c) {
                    uint64_t bit = 1ull << (c * 7 + (5 - r));
                    if (hb[(size_t)b * 84 + r * 7 + c] != 0.0f) states[2 * b] |= bit;
                    if (hb[(size_t)b * 84 + 42 + r * 7 + c] != 0.0f) states[2 * b + 1] |= bit;
                }
        return az_net_predict_states(e, model_id, states.data(), B, pi, v);
    } catch (const HipFail& f) { return fail_hip(e, f); }
}

// ---- held-out loss on the device and the hold-out mask (csrc/az_score.h, DESIGN.md sections 4.1l and 8.3) ----------------------------------
}  // extern "C"

namespace {

struct ScoreSet {               // a window on the device: validated states, targets, weights (nullptr = all ones)
    int64_t n;
    const ulonglong2* states;
    const float* pis;
    const float* zs;
    const uint32_t* weights;
};
struct ScoreOut { float* ce; float* se; float* kl; };        // device, each [n] or nullptr
inline size_t score_pad(size_t bytes) { return (bytes + 255) / 256 * 256; }
// the part of the workspace a run of forwards needs: [row counts] [chunk states] [chunk pi] [chunk v] [mirror flags]
size_t score_work_bytes(const az_engine* e) {
    const size_t c = (size_t)e->cfg.max_batch;
    return 256 + score_pad(c * 16) + score_pad(c * 32) + score_pad(c * 4) + score_pad(c);
}
// Enqueues, on the engine's stream, the forward of every max_batch chunk of the window and the score kernel behind it: what
// az_net_predict_states runs per chunk, with (pi, v) read where the forward left them.  No synchronisation, no copy to the host.
void score_enqueue(az_engine* e, const NetModel& m, char* work, const ScoreSet& w, uint64_t* d_sums, const ScoreOut& o) {
    hipStream_t s = e->stream;
    const int chunk = e->cfg.max_batch;
    const size_t c = (size_t)chunk;
    uint32_t* d_rows = (uint32_t*)work;                     // [0] a full chunk, [1] the last one
    EvalBatch eb{};
    eb.cap = chunk;
    eb.state = (ulonglong2*)(work + 256);
    eb.pi = (float*)(work + 256 + score_pad(c * 16));
    eb.v = (float*)(work + 256 + score_pad(c * 16) + score_pad(c * 32));
    uint8_t* mflags = mirror_applies(e, m) ? (uint8_t*)(work + 256 + score_pad(c * 16) + score_pad(c * 32) + score_pad(c * 4)) : nullptr;
    const int64_t chunks = (w.n + chunk - 1) / chunk;
    const uint32_t h_rows[2] = {(uint32_t)chunk, (uint32_t)(w.n - (chunks - 1) * chunk)};
    HIPCHK(hipMemcpy(d_rows, h_rows, sizeof h_rows, hipMemcpyHostToDevice));
    for (int64_t k = 0; k < chunks; ++k) {
        const bool last = k + 1 == chunks;
        const int nb = (int)h_rows[last ? 1 : 0];
        eb.n = d_rows + (last ? 1 : 0);
        HIPCHK(hipMemcpyAsync(eb.state, w.states + (size_t)k * c, (size_t)nb * 16, hipMemcpyDeviceToDevice, s));
        if (mflags) launch_canonicalise(eb.state, mflags, nb, s);
        net_forward(e, m, eb, nb, s);
        if (mflags) launch_unmirror_rows(eb.pi, mflags, nb, s);
        launch_score(eb.pi, eb.v, w.states, w.pis, w.zs, w.weights, k * (int64_t)chunk, nb, d_sums, o.ce, o.se, o.kl, s);
    }
    HIPCHK(hipGetLastError());
}
const char* score_sum_text(const uint64_t* sums) {
    if (sums[4] == 0) return "the weights sum to 0";
    if (sums[4] > SCORE_MAX_WEIGHT) return "the weights sum to more than 2^24";
    return nullptr;
}
// out[0 .. 4) = loss_pi, loss_v, kl, top1 from the integers
void score_results(const uint64_t* sums, double* out) {
    const double W = (double)sums[4], one = 1073741824.0;
    out[0] = (double)sums[0] / one / W;
    out[1] = (double)sums[2] / one / W;
    out[2] = (double)sums[1] / one / W;
    out[3] = (double)sums[3] / W;
}

}  // namespace

extern "C" {

az_status az_net_evaluate(az_engine* e, int32_t model_id, const az_samples* smp, const uint32_t* weights, double* score, uint64_t* sums_out, float* ce,
                          float* se, float* kl) {
    if (!e) return AZ_ERR_BAD_ARGUMENT;
    if (!smp || !score) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_net_evaluate: the samples and score are required");
    const int64_t n = smp->count;
    if (n < 1 || n > SCORE_MAX_TUPLES) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_net_evaluate: 1 .. 2^24 tuples");
    if (const char* why = samples_shape_error(smp, false)) return fail(e, AZ_ERR_BAD_ARGUMENT, std::string("az_net_evaluate: the samples need ") + why);
    NetModel* m;
    az_status st = find_net(e, model_id, &m);
    if (st) return st;
    ScopedTimer timer{e};
    try {
        HIPCHK(hipSetDevice(e->device));
        hipStream_t s = e->stream;
        const size_t N = (size_t)n;
        const bool from_boards = !smp->states;
        Carve c;
        // [hdr: verdict, sums] [inputs] [validated states] [per-tuple outputs] [the forwards' part]
        const size_t o_hdr = c.need(256), o_in = c.need(from_boards ? N * AZ_FEATURES * 4 : N * 16), o_st = c.need(N * 16), o_pi = c.need(N * 28),
                     o_z = c.need(N * 4), o_w = c.need(weights ? N * 4 : 0), o_ce = c.need(ce ? N * 4 : 0), o_se = c.need(se ? N * 4 : 0),
                     o_kl = c.need(kl ? N * 4 : 0), o_work = c.need(score_work_bytes(e));
        char* base = (char*)e->score_scratch.fit(c.total, s);
        uint32_t* d_bad = (uint32_t*)(base + o_hdr);
        uint64_t* d_sums = (uint64_t*)(base + o_hdr + 8);
        // the whole window is staged once
        HIPCHK(hipMemsetAsync(base + o_hdr, 0, 256, s));
        const SampleWindow in = stage_window(base + o_in, base + o_pi, base + o_z, smp, s);
        if (weights) HIPCHK(hipMemcpyAsync(base + o_w, weights, N * 4, hipMemcpyDefault, s));
        launch_score_states(in, 1, n, (ulonglong2*)(base + o_st), d_bad, s);
        const ScoreSet w{n, (const ulonglong2*)(base + o_st), in.pis, in.zs, weights ? (const uint32_t*)(base + o_w) : nullptr};
        const ScoreOut o{ce ? (float*)(base + o_ce) : nullptr, se ? (float*)(base + o_se) : nullptr, kl ? (float*)(base + o_kl) : nullptr};
        score_enqueue(e, *m, base + o_work, w, d_sums, o);
        uint64_t hdr[1 + SCORE_SUMS] = {0, 0, 0, 0, 0, 0};
        HIPCHK(hipMemcpyAsync(hdr, base + o_hdr, sizeof hdr, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));                    // the one synchronisation
        resolve_profile(e);
        if (const char* why = sample_bad_text((uint32_t)hdr[0], true)) return fail(e, AZ_ERR_BAD_ARGUMENT, std::string("az_net_evaluate: ") + why);
        if (const char* why = score_sum_text(hdr + 1)) return fail(e, AZ_ERR_BAD_ARGUMENT, std::string("az_net_evaluate: ") + why);
        score[0] = (double)n;
        score[1] = (double)hdr[1 + 4];
        score_results(hdr + 1, score + 2);
        if (sums_out) std::memcpy(sums_out, hdr + 1, SCORE_SUMS * sizeof(uint64_t));
        if (ce || se || kl) {                               // a refused call leaves the caller's arrays unwritten
            if (ce) HIPCHK(hipMemcpyAsync(ce, base + o_ce, N * 4, hipMemcpyDefault, s));
            if (se) HIPCHK(hipMemcpyAsync(se, base + o_se, N * 4, hipMemcpyDefault, s));
            if (kl) HIPCHK(hipMemcpyAsync(kl, base + o_kl, N * 4, hipMemcpyDefault, s));
            HIPCHK(hipStreamSynchronize(s));
        }
        return AZ_OK;
    } catch (const HipFail& f) { return fail_hip(e, f); }
}

az_status az_samples_holdout(az_engine* e, const az_samples* smp, int64_t share_e6, uint64_t seed, uint8_t* held) {
    if (!e) return AZ_ERR_BAD_ARGUMENT;
    if (!smp || !held) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_samples_holdout: the samples and held are required");
    if (e->sp_session) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_samples_holdout: a self-play session is open");
    if (share_e6 < 0 || share_e6 > TARGET_E6) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_samples_holdout: share_e6 must be in 0 .. 1000000");
    const int64_t n = smp->count;
    if (n < 0 || n > SCORE_MAX_TUPLES) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_samples_holdout: 0 .. 2^24 tuples");
    if (const char* why = samples_shape_error(smp, true)) return fail(e, AZ_ERR_BAD_ARGUMENT, std::string("az_samples_holdout: the samples need ") + why);
    if (n == 0) return AZ_OK;
    ScopedTimer timer{e};
    try {
        HIPCHK(hipSetDevice(e->device));
        hipStream_t s = e->stream;
        const size_t N = (size_t)n;
        const bool from_boards = !smp->states;
        Carve c;
        const size_t o_hdr = c.need(256), o_in = c.need(from_boards ? N * AZ_FEATURES * 4 : N * 16), o_st = c.need(N * 16), o_pi = c.need(N * 28),
                     o_z = c.need(N * 4), o_held = c.need(N);
        char* base = (char*)e->score_scratch.fit(c.total, s);
        uint32_t* d_bad = (uint32_t*)(base + o_hdr);
        HIPCHK(hipMemsetAsync(base + o_hdr, 0, 256, s));
        launch_score_states(stage_window(base + o_in, base + o_pi, base + o_z, smp, s), 0, n, (ulonglong2*)(base + o_st), d_bad, s);
        launch_score_holdout((const ulonglong2*)(base + o_st), n, seed, score_thresh24((uint64_t)share_e6), (uint8_t*)(base + o_held), s);
        const uint32_t bad = read_verdict(d_bad, s);
        // a value fault is reported before a feature or a state fault here
        if (const char* why = sample_bad_text(bad & SAMPLE_BAD_VALUE ? SAMPLE_BAD_VALUE : bad, false)) return fail(e, AZ_ERR_BAD_ARGUMENT, std::string("az_samples_holdout: ") + why);
        HIPCHK(hipMemcpy(held, base + o_held, N, hipMemcpyDefault));
        return AZ_OK;
    } catch (const HipFail& f) { return fail_hip(e, f); }
}

// ---- per-epoch validation of az_net_train / az_net_train_samples (csrc/az_score.h) -----------------------------------
}  // extern "C"

namespace {

// what az_net_train and az_net_train_samples refuse before they begin
const char* validation_arg_error(const az_engine* e) {
    if ((e->train_keep_best || e->train_patience) && e->val_n == 0) return "\"train_keep_best\" and \"train_patience\" need a validation set (az_net_train_set_validation)";
    return nullptr;
}
// One epoch's row of the validation history: the trainer's live parameters and moving averages (what az_net_train_end would store now) go
// into the slot no id names, in the effective class of `model_id` (a fresh id: the engine's), and are scored on the registered set.  Reads
// the trainer, writes nothing of it.  *stop = the patience rule's verdict; with "train_keep_best" `best_params` follows the best epoch.
az_status validate_epoch(az_engine* e, int32_t model_id, std::vector<float>& params, std::vector<float>& best_params, bool* stop) {
    *stop = false;
    if (e->val_n == 0) return AZ_OK;
    const int64_t n = az_net_param_count(e);
    params.resize((size_t)n);
    if (!trainer_get_params(e->trainer, params.data(), n, e->stream)) return fail(e, AZ_ERR_HIP, "trainer_get_params failed");
    NetModel& m = e->val_model;
    if (!m.conv) {
        const char* why = nullptr;
        m.conv = convnet_create(e->cfg.net_channels, &why);
        if (!m.conv) return fail(e, AZ_ERR_HIP, why ? why : "convnet_create failed");
    }
    if (!convnet_set_params(m.conv, params.data(), n)) return fail(e, AZ_ERR_HIP, "convnet_set_params failed");
    m.kind = AZ_NET_CONV;
    const auto dst = e->nets.find(model_id);
    m.klass = dst != e->nets.end() && dst->second.kind == AZ_NET_CONV ? dst->second.klass : AZ_NET_CLASS_ENGINE;
    if (az_status st = fp8_sync_model(e, m)) return st;
    hipStream_t s = e->stream;
    const size_t total = 256 + score_work_bytes(e);
    char* base = (char*)e->score_scratch.ensure(total, s);
    uint64_t* d_sums = (uint64_t*)(base + 8);
    HIPCHK(hipMemsetAsync(base, 0, 256, s));
    const ScoreSet w{e->val_n, e->val_states, e->val_pis, e->val_zs, e->val_weights};
    score_enqueue(e, m, base + 256, w, d_sums, ScoreOut{nullptr, nullptr, nullptr});
    uint64_t sums[SCORE_SUMS];
    HIPCHK(hipMemcpyAsync(sums, d_sums, sizeof sums, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    double row[4];
    score_results(sums, row);
    e->val_history.insert(e->val_history.end(), row, row + 4);
    const int epochs = (int)(e->val_history.size() / 4);
    int best = 0;
    *stop = score_best_stop(e->val_history.data(), 4, epochs, (int)e->train_patience, &best);
    e->val_best = best;
    if (e->train_keep_best && best == epochs - 1) best_params = params;
    return AZ_OK;
}
// az_net_train_end, storing the best epoch's parameters where "train_keep_best" kept some
az_status train_store(az_engine* e, int32_t model_id, const std::vector<float>& best_params) {
    if (!e->train_keep_best || best_params.empty()) return az_net_train_end(e, model_id);
    e->train_open = false;
    return az_net_set_params(e, model_id, best_params.data(), (int64_t)best_params.size());
}

}  // namespace

extern "C" {

az_status az_net_train_set_validation(az_engine* e, const az_samples* v, const uint32_t* weights) {
    if (!e) return AZ_ERR_BAD_ARGUMENT;
    if (e->train_open) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_net_train_set_validation: a training session is open");
    try {
        HIPCHK(hipSetDevice(e->device));
        hipStream_t s = e->stream;
        if (!v) {
            HIPCHK(hipStreamSynchronize(s));
            e->val_mem.release();
            e->val_n = 0;
            e->val_states = nullptr; e->val_pis = nullptr; e->val_zs = nullptr; e->val_weights = nullptr;
            return AZ_OK;
        }
        const int64_t n = v->count;
        if (n < 1 || n > SCORE_MAX_TUPLES) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_net_train_set_validation: 1 .. 2^24 tuples");
        if (const char* why = samples_shape_error(v, false)) return fail(e, AZ_ERR_BAD_ARGUMENT, std::string("az_net_train_set_validation: the samples need ") + why);
        const size_t N = (size_t)n;
        uint64_t W = (uint64_t)n;
        if (weights) {
            std::vector<uint32_t> hw(N);
            HIPCHK(hipMemcpy(hw.data(), weights, N * 4, hipMemcpyDefault));
            W = 0;
            for (uint32_t x : hw) W += x;
        }
        if (W == 0 || W > SCORE_MAX_WEIGHT) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_net_train_set_validation: the weights must sum to 1 .. 2^24");
        // the new set is built beside the old one, which a refusal leaves registered
        DeviceMem mem;
        const bool from_boards = !v->states;
        ulonglong2* d_st = mem.alloc<ulonglong2>(N);
        float* d_pi = mem.alloc<float>(N * 7);
        float* d_z = mem.alloc<float>(N);
        uint32_t* d_w = weights ? mem.alloc<uint32_t>(N) : nullptr;
        uint32_t* d_bad = mem.alloc<uint32_t>(1);
        {
            DeviceMem in;
            void* d_in = from_boards ? (void*)in.alloc<float>(N * AZ_FEATURES) : (void*)in.alloc<ulonglong2>(N);
            HIPCHK(hipMemsetAsync(d_bad, 0, sizeof(uint32_t), s));
            if (d_w) HIPCHK(hipMemcpyAsync(d_w, weights, N * 4, hipMemcpyDefault, s));
            launch_score_states(stage_window(d_in, d_pi, d_z, v, s), 1, n, d_st, d_bad, s);
            if (const char* why = sample_bad_text(read_verdict(d_bad, s), true)) return fail(e, AZ_ERR_BAD_ARGUMENT, std::string("az_net_train_set_validation: ") + why);
        }
        e->val_mem.release();
        std::swap(e->val_mem.ptrs, mem.ptrs);
        e->val_n = n;
        e->val_states = d_st; e->val_pis = d_pi; e->val_zs = d_z; e->val_weights = d_w;
        return AZ_OK;
    } catch (const HipFail& f) { return fail_hip(e, f); }
}

int32_t az_net_train_validation(const az_engine* e, double* out, int32_t cap_epochs, int32_t* best_epoch) {
    if (!e) return 0;
    const int32_t epochs = (int32_t)(e->val_history.size() / 4);
    if (out)
        for (int32_t i = 0; i < std::min(epochs, cap_epochs); ++i)
            for (int j = 0; j < 4; ++j) out[4 * i + j] = e->val_history[(size_t)4 * i + j];
    if (best_epoch) *best_epoch = epochs ? e->val_best : -1;
    return epochs;
}

// ---- NNet::train, src/nnet.rs:38 ----------------------------------------------------------------
az_status az_net_train_begin(az_engine* e, int32_t previous_model_id) {
    if (!e) return AZ_ERR_BAD_ARGUMENT;
    NetModel* m;
    az_status st = find_net(e, previous_model_id, &m);
    if (st) return st;
    if (m->kind != AZ_NET_CONV) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_net_train: the previous model has no parameters");
    try {
        HIPCHK(hipSetDevice(e->device));
        if (!e->trainer) {
            const char* err = nullptr;
            e->trainer = trainer_create(e->cfg.net_channels, &err);
            if (!e->trainer) return fail(e, AZ_ERR_HIP, err ? err : "trainer_create failed");
            trainer_set_graph(e->trainer, e->train_graph != 0);
            trainer_set_switches(e->trainer, e->train_sw);
        }
        const int64_t n = az_net_param_count(e);
        std::vector<float> p((size_t)n);
        if (!convnet_get_params(m->conv, p.data(), n)) return fail(e, AZ_ERR_BAD_ARGUMENT, "parameter count mismatch");
        if (!trainer_set_params(e->trainer, p.data(), n)) return fail(e, AZ_ERR_HIP, "trainer_set_params failed");
        TrainOptim o;
        o.weight_decay = (float)((double)e->train_weight_decay_e9 / 1e9);
        o.clip_norm = (double)e->train_clip_norm_e6 / 1e6;
        o.warmup = e->train_lr_warmup_steps;
        o.decay = (int)e->train_lr_decay;
        o.floor = (double)e->train_lr_floor_e6 / 1e6;
        o.total = e->train_lr_total_steps;
        o.ema = (float)((double)e->train_ema_decay_e9 / 1e9);
        e->train_ema_session = false;
        if (!trainer_set_optim(e->trainer, o)) return fail(e, AZ_ERR_HIP, "trainer_set_optim failed");
        e->train_ema_session = o.ema > 0.0f;
        e->train_open = true;
        return AZ_OK;
    } catch (const HipFail& f) { return fail_hip(e, f); }
}

az_status az_net_train_step(az_engine* e, const float* boards, const float* pis, const float* vs, int32_t b, uint64_t mask_seed,
                            int32_t apply, float* loss_out, float* grads_out) {
    if (!e || !boards || !pis || !vs) return AZ_ERR_BAD_ARGUMENT;
    if (!e->train_open) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_net_train_step: call az_net_train_begin first");
    if (b < 2 || b > TRAIN_MAX_BATCH) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_net_train_step: batch must be in [2, 256]");
    try {
        HIPCHK(hipSetDevice(e->device));
        Trainer* t = e->trainer;
        HIPCHK(hipMemcpyAsync(trainer_batch_boards(t), boards, (size_t)b * 84 * sizeof(float), hipMemcpyDefault, e->stream));
        HIPCHK(hipMemcpyAsync(trainer_batch_pis(t), pis, (size_t)b * 7 * sizeof(float), hipMemcpyDefault, e->stream));
        HIPCHK(hipMemcpyAsync(trainer_batch_vs(t), vs, (size_t)b * sizeof(float), hipMemcpyDefault, e->stream));
        if (!trainer_step(t, e->hyper, trainer_batch_boards(t), trainer_batch_pis(t), trainer_batch_vs(t), b, mask_seed, apply != 0,
                          e->stream))
            return fail(e, AZ_ERR_HIP, "trainer_step failed");
        double l[2];
        if (!trainer_read_losses(t, l, true, e->stream)) return fail(e, AZ_ERR_HIP, "trainer_read_losses failed");
        if (loss_out) { loss_out[0] = (float)l[0]; loss_out[1] = (float)l[1]; }
        if (grads_out && !trainer_get_grads(t, grads_out, az_net_param_count(e), e->stream))
            return fail(e, AZ_ERR_HIP, "trainer_get_grads failed");
        return AZ_OK;
    } catch (const HipFail& f) { return fail_hip(e, f); }
}

az_status az_net_train_end(az_engine* e, int32_t model_id) {
    if (!e) return AZ_ERR_BAD_ARGUMENT;
    if (!e->train_open) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_net_train_end: no open training session");
    if (az_status sr = session_model_refusal(e, "az_net_train_end", model_id)) return sr;      // the training session stays open
    const int64_t n = az_net_param_count(e);
    std::vector<float> p((size_t)n);
    if (!trainer_get_params(e->trainer, p.data(), n, e->stream)) return fail(e, AZ_ERR_HIP, "trainer_get_params failed");
    e->train_open = false;
    return az_net_set_params(e, model_id, p.data(), n);
}

az_status az_net_train(az_engine* e, int32_t previous_model_id, int32_t model_id, const float* boards, const float* pis,
                       const float* vs, int64_t n) {
    if (!e || !boards || !pis || !vs || n <= 0) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_net_train: bad argument");
    if (e->train_open) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_net_train: a training session is open (az_net_train_end first)");
    if (az_status sr = session_model_refusal(e, "az_net_train", model_id)) return sr;
    if (const char* why = validation_arg_error(e)) return fail(e, AZ_ERR_BAD_ARGUMENT, (std::string("az_net_train: ") + why).c_str());
    az_status st = az_net_train_begin(e, previous_model_id);
    if (st) return st;
    ScopedTimer timer{e};
    std::vector<float> val_params, best_params;
    try {
        DeviceMem mem;
        float* d_boards = mem.alloc<float>((size_t)n * 84);
        float* d_pis = mem.alloc<float>((size_t)n * 7);
        float* d_vs = mem.alloc<float>((size_t)n);
        HIPCHK(hipMemcpy(d_boards, boards, (size_t)n * 84 * sizeof(float), hipMemcpyDefault));
        HIPCHK(hipMemcpy(d_pis, pis, (size_t)n * 7 * sizeof(float), hipMemcpyDefault));
        HIPCHK(hipMemcpy(d_vs, vs, (size_t)n * sizeof(float), hipMemcpyDefault));
        const int b = e->train_batch;
        const int64_t steps = std::max<int64_t>(1, n / b);          // connect_four_net.py:127-130: len(examples) / batch_size
        int64_t* d_idx = mem.alloc<int64_t>((size_t)steps * b);
        std::vector<int64_t> idx((size_t)steps * b);
        Trainer* t = e->trainer;
        e->train_history.clear();
        e->val_history.clear();
        e->val_best = -1;
        // a failure below closes the training session az_net_train_begin opened above: the next az_net_train must not find it open
        if (!trainer_set_lr_table(t, e->hyper, (int64_t)e->train_epochs * steps, e->stream)) { e->train_open = false; return fail(e, AZ_ERR_HIP, "trainer_set_lr_table failed"); }
        uint64_t gstep = 0;
        for (int epoch = 0; epoch < e->train_epochs; ++epoch) {
            // batches are drawn with replacement (np.random.randint, :130), from the build's counter RNG
            for (int64_t sidx = 0; sidx < steps; ++sidx)
                for (int j = 0; j < b; ++j) {
                    const uint64_t r = rng_draw(e->train_seed, gstep + (uint64_t)sidx, (uint64_t)j, RNG_BATCH);
                    idx[(size_t)sidx * b + j] = (int64_t)(((unsigned __int128)r * (unsigned __int128)n) >> 64);
                }
            HIPCHK(hipMemcpyAsync(d_idx, idx.data(), idx.size() * sizeof(int64_t), hipMemcpyHostToDevice, e->stream));
            if (!trainer_run_epoch(t, e->hyper, d_boards, d_pis, d_vs, d_idx, steps, b, mix64(e->train_seed ^ 0xD6E8FEB86659FD93ull), gstep,
                                   e->stream)) {
                e->train_open = false;
                return fail(e, AZ_ERR_HIP, "trainer_run_epoch failed");
            }
            gstep += (uint64_t)steps;
            double l[2];
            if (!trainer_read_losses(t, l, true, e->stream)) { e->train_open = false; return fail(e, AZ_ERR_HIP, "trainer_read_losses failed"); }
            e->train_history.push_back((float)(l[0] / (double)steps));
            e->train_history.push_back((float)(l[1] / (double)steps));
            bool stop = false;
            if (az_status vst = validate_epoch(e, model_id, val_params, best_params, &stop)) { e->train_open = false; return vst; }
            if (stop) break;
        }
        HIPCHK(hipStreamSynchronize(e->stream));
    } catch (const HipFail& f) { e->train_open = false; return fail_hip(e, f); }
    return train_store(e, model_id, best_params);
}

// ---- NNet::train from an az_samples, rows drawn in proportion to their multiplicities (csrc/az_draw.h) ---------------
}  // extern "C"

namespace {

// The weights on the device and their prefix sum: Q == nullptr (weights NULL) means all ones and W = n.
struct DrawTable {
    const uint64_t* Q = nullptr;
    uint64_t W = 0;
};
DrawTable draw_table(az_engine* e, DeviceMem& mem, int64_t n, const uint32_t* weights) {
    DrawTable d;
    if (!weights) { d.W = (uint64_t)n; return d; }
    uint32_t* d_w = mem.alloc<uint32_t>((size_t)n);
    uint64_t* d_q = mem.alloc<uint64_t>((size_t)n);
    uint64_t* d_bsum = mem.alloc<uint64_t>(draw_scan_blocks(n) + 1);
    uint64_t* d_total = d_bsum + draw_scan_blocks(n);
    HIPCHK(hipMemcpyAsync(d_w, weights, (size_t)n * sizeof(uint32_t), hipMemcpyDefault, e->stream));
    launch_draw_scan(d_w, n, d_q, d_bsum, d_total, e->stream);
    HIPCHK(hipMemcpyAsync(&d.W, d_total, sizeof(uint64_t), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    HIPCHK(hipGetLastError());
    d.Q = d_q;
    return d;
}
const char* draw_arg_error(const az_engine* e, int64_t n, int32_t flags) {
    if (flags & ~(AZ_TRAIN_EPOCH_BY_WEIGHT | AZ_TRAIN_MIRROR)) return "unknown flag bits";
    if (n < 1 || n > DRAW_MAX_TUPLES) return "1 .. 2^31 - 1 tuples";
    if (e->train_open) return "a training session is open";
    if (e->sp_session) return "a self-play session is open";
    return nullptr;
}

}  // namespace

extern "C" {

az_status az_net_train_draw(az_engine* e, int64_t n, const uint32_t* weights, int32_t flags, uint64_t t0, int64_t steps, int64_t* idx_out,
                            uint8_t* mirror_out) {
    if (!e) return AZ_ERR_BAD_ARGUMENT;
    if (const char* why = draw_arg_error(e, n, flags)) return fail(e, AZ_ERR_BAD_ARGUMENT, (std::string("az_net_train_draw: ") + why).c_str());
    if (!idx_out || steps < 1) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_net_train_draw: idx_out and steps >= 1 are required");
    ScopedTimer timer{e};
    try {
        HIPCHK(hipSetDevice(e->device));
        DeviceMem mem;
        const DrawTable d = draw_table(e, mem, n, weights);
        if (d.W == 0) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_net_train_draw: the weights sum to 0");
        const int b = e->train_batch;
        const size_t rows = (size_t)steps * (size_t)b;
        int64_t* d_idx = mem.alloc<int64_t>(rows);
        uint8_t* d_mir = mem.alloc<uint8_t>(rows);
        launch_draw_rows(d.Q, n, d.W, e->train_seed, t0, steps, b, (flags & AZ_TRAIN_MIRROR) != 0, d_idx, d_mir, e->stream);
        HIPCHK(hipMemcpyAsync(idx_out, d_idx, rows * sizeof(int64_t), hipMemcpyDefault, e->stream));
        if (mirror_out) HIPCHK(hipMemcpyAsync(mirror_out, d_mir, rows, hipMemcpyDefault, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        HIPCHK(hipGetLastError());
        return AZ_OK;
    } catch (const HipFail& f) { return fail_hip(e, f); }
}

az_status az_net_train_samples(az_engine* e, int32_t previous_model_id, int32_t model_id, const az_samples* s, const uint32_t* weights,
                               int32_t flags) {
    if (!e) return AZ_ERR_BAD_ARGUMENT;
    if (!s) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_net_train_samples: the samples are required");
    const int64_t n = s->count;
    if (const char* why = draw_arg_error(e, n, flags)) return fail(e, AZ_ERR_BAD_ARGUMENT, (std::string("az_net_train_samples: ") + why).c_str());
    if (const char* why = samples_shape_error(s, false)) return fail(e, AZ_ERR_BAD_ARGUMENT, std::string("az_net_train_samples: the samples need ") + why);
    if (const char* why = validation_arg_error(e)) return fail(e, AZ_ERR_BAD_ARGUMENT, (std::string("az_net_train_samples: ") + why).c_str());
    ScopedTimer timer{e};
    std::vector<float> val_params, best_params;
    try {
        HIPCHK(hipSetDevice(e->device));
        DeviceMem mem;
        // the resident set: states (16 bytes; or the planes the caller holds, 336) + pis + zs (+ weights + Q) per tuple
        TrainSamples src{};
        if (s->states) {
            ulonglong2* d_states = mem.alloc<ulonglong2>((size_t)n);
            uint32_t* d_bad = mem.alloc<uint32_t>(1);
            HIPCHK(hipMemcpyAsync(d_states, s->states, (size_t)n * 16, hipMemcpyDefault, e->stream));
            HIPCHK(hipMemsetAsync(d_bad, 0, sizeof(uint32_t), e->stream));
            launch_draw_check_states(d_states, n, d_bad, e->stream);
            if (const char* why = sample_bad_text(read_verdict(d_bad, e->stream), false)) return fail(e, AZ_ERR_BAD_ARGUMENT, std::string("az_net_train_samples: ") + why);
            src.states = d_states;
        } else {
            float* d_boards = mem.alloc<float>((size_t)n * 84);
            HIPCHK(hipMemcpyAsync(d_boards, s->boards, (size_t)n * 84 * sizeof(float), hipMemcpyDefault, e->stream));
            src.boards = d_boards;
        }
        const DrawTable d = draw_table(e, mem, n, weights);
        if (d.W == 0) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_net_train_samples: the weights sum to 0");
        float* d_pis = mem.alloc<float>((size_t)n * 7);
        float* d_vs = mem.alloc<float>((size_t)n);
        HIPCHK(hipMemcpyAsync(d_pis, s->pis, (size_t)n * 7 * sizeof(float), hipMemcpyDefault, e->stream));
        HIPCHK(hipMemcpyAsync(d_vs, s->zs, (size_t)n * sizeof(float), hipMemcpyDefault, e->stream));
        src.pis = d_pis;
        src.vs = d_vs;
        const int b = e->train_batch;
        const int64_t steps = draw_epoch_steps((flags & AZ_TRAIN_EPOCH_BY_WEIGHT) ? d.W : (uint64_t)n, b);
        const bool mirror = (flags & AZ_TRAIN_MIRROR) != 0;
        int64_t* d_idx = mem.alloc<int64_t>((size_t)steps * b);
        uint8_t* d_mir = mirror ? mem.alloc<uint8_t>((size_t)steps * b) : nullptr;
        HIPCHK(hipStreamSynchronize(e->stream));
        // every refusal is behind us: from here on it is az_net_train with another index table and another gather
        az_status st = az_net_train_begin(e, previous_model_id);
        if (st) return st;
        try {
            Trainer* t = e->trainer;
            e->train_history.clear();
            e->val_history.clear();
            e->val_best = -1;
            if (!trainer_set_lr_table(t, e->hyper, (int64_t)e->train_epochs * steps, e->stream)) {
                e->train_open = false;
                return fail(e, AZ_ERR_HIP, "trainer_set_lr_table failed");
            }
            uint64_t gstep = 0;
            for (int epoch = 0; epoch < e->train_epochs; ++epoch) {
                launch_draw_rows(d.Q, n, d.W, e->train_seed, gstep, steps, b, mirror, d_idx, d_mir, e->stream);
                if (!trainer_run_epoch_samples(t, e->hyper, src, d_idx, d_mir, steps, b, mix64(e->train_seed ^ 0xD6E8FEB86659FD93ull), gstep,
                                               e->stream)) {
                    e->train_open = false;
                    return fail(e, AZ_ERR_HIP, "trainer_run_epoch_samples failed");
                }
                gstep += (uint64_t)steps;
                double l[2];
                if (!trainer_read_losses(t, l, true, e->stream)) { e->train_open = false; return fail(e, AZ_ERR_HIP, "trainer_read_losses failed"); }
                e->train_history.push_back((float)(l[0] / (double)steps));
                e->train_history.push_back((float)(l[1] / (double)steps));
                bool stop = false;
                if (az_status vst = validate_epoch(e, model_id, val_params, best_params, &stop)) { e->train_open = false; return vst; }
                if (stop) break;
            }
            HIPCHK(hipStreamSynchronize(e->stream));
        } catch (const HipFail& f) { e->train_open = false; return fail_hip(e, f); }
    } catch (const HipFail& f) { return fail_hip(e, f); }
    return train_store(e, model_id, best_params);
}

az_status az_net_train_ema(az_engine* e, int32_t model_id) {
    if (!e) return AZ_ERR_BAD_ARGUMENT;
    if (az_status sr = session_model_refusal(e, "az_net_train_ema", model_id)) return sr;
    if (!e->trainer || !e->train_ema_session)
        return fail(e, AZ_ERR_BAD_ARGUMENT, "az_net_train_ema: the last az_net_train_begin did not see \"train_ema_decay_e9\" > 0");
    try {
        HIPCHK(hipSetDevice(e->device));
        const int64_t n = az_net_param_count(e);
        std::vector<float> p((size_t)n);
        if (!trainer_get_ema(e->trainer, p.data(), n, e->stream)) return fail(e, AZ_ERR_HIP, "trainer_get_ema failed");
        return az_net_set_params(e, model_id, p.data(), n);
    } catch (const HipFail& f) { return fail_hip(e, f); }
}

az_status az_net_train_step_info(const az_engine* e, double out[4]) {
    if (!e || !out) return AZ_ERR_BAD_ARGUMENT;
    if (!e->trainer) return AZ_ERR_BAD_ARGUMENT;
    if (hipSetDevice(e->device) != hipSuccess || !trainer_step_info(e->trainer, out, e->stream)) return AZ_ERR_HIP;
    return AZ_OK;
}

int32_t az_net_train_history(const az_engine* e, float* out, int32_t cap_epochs) {
    if (!e) return 0;
    const int32_t epochs = (int32_t)(e->train_history.size() / 2);
    if (out)
        for (int32_t i = 0; i < std::min(epochs, cap_epochs); ++i) { out[2 * i] = e->train_history[2 * i]; out[2 * i + 1] = e->train_history[2 * i + 1]; }
    return epochs;
}

// ---- AsyncMcts -------------------------------------------------------------------------------
// num_sims % num_threads == 0 (assert!, src/async_mcts.rs:192); 0 means 1
static az_status check_threads(az_engine* e, int num_sims, int* num_threads) {
    if (*num_threads == 0) *num_threads = 1;
    if (*num_threads < 1 || *num_threads > MAX_SIM_THREADS) return fail(e, AZ_ERR_BAD_ARGUMENT, "num_threads must be in [1, 8]");
    if (num_sims % *num_threads != 0) return fail(e, AZ_ERR_BAD_ARGUMENT, "num_sims % num_threads != 0 (src/async_mcts.rs:192)");
    return AZ_OK;
}

az_status az_tree_create(az_engine* e, int32_t n_games, uint64_t reserve, int32_t num_sims, int32_t num_threads, int32_t max_depth,
                         int32_t model_id, int32_t cpuct, az_tree** out) {
    if (!e || !out || n_games <= 0 || num_sims <= 0 || reserve < 8 || max_depth < 0)
        return fail(e, AZ_ERR_BAD_ARGUMENT, "az_tree_create: bad argument");
    if (az_status st = check_threads(e, num_sims, &num_threads)) return st;
    if (n_games > 1024 * 64) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_tree_create: at most 65536 trees per batch");
    *out = nullptr;
    try {
        HIPCHK(hipSetDevice(e->device));
        std::unique_ptr<az_tree> t(new az_tree());
        t->e = e;
        t->num_sims = num_sims; t->max_depth = max_depth; t->model_id = model_id; t->cpuct = cpuct;
        const uint64_t nodes = std::min<uint64_t>(reserve, reachable_slots(num_sims, AZ_MAX_PLIES));
        if (az_status cs = check_tree_slots(e, reachable_blocks(num_sims, AZ_MAX_PLIES, nodes))) return cs;
        t->th.create(n_games, reachable_blocks(num_sims, AZ_MAX_PLIES, nodes), nodes, hash_entries(num_sims, AZ_MAX_PLIES), num_threads, e->cfg.game);
        t->d_root_states = t->mem.alloc<ulonglong2>(n_games);
        t->d_noise_streams = t->mem.alloc<ulonglong2>(n_games);
        {
            const size_t G = (size_t)n_games, head = (sizeof(CallReadback) + 63) / 64 * 64;
            HIPCHK(hipHostMalloc(&t->h_io, head + G * 16 + G * 7 * 4 * 2 + G * 7 * 2, hipHostMallocDefault));
            char* p = (char*)t->h_io;
            t->h_rb = (CallReadback*)p; p += head;
            t->h_states = (ulonglong2*)p; p += G * 16;
            t->h_pi = (float*)p; p += G * 7 * 4;
            t->h_q = (float*)p; p += G * 7 * 4;
            t->h_counts = (uint16_t*)p;
        }
        launch_reset_trees(t->th.d, nullptr, e->stream);
        HIPCHK(hipStreamSynchronize(e->stream));
        *out = t.release();
        return AZ_OK;
    } catch (const HipFail& f) { return fail_hip(e, f); }
}

void az_tree_destroy(az_tree* t) {
    if (!t) return;
    (void)hipSetDevice(t->e->device);
    (void)hipStreamSynchronize(t->e->stream);
    delete t;
}

az_status az_tree_reset(az_tree* t, const uint64_t* root_states) {
    if (!t) return AZ_ERR_BAD_ARGUMENT;
    az_engine* e = t->e;
    if (t->shared) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_tree_reset on a shared tree batch (its slots belong to their threads)");
    try {
        HIPCHK(hipSetDevice(e->device));
        const ulonglong2* roots = nullptr;
        if (root_states) {
            HIPCHK(hipMemcpyAsync(t->d_root_states, root_states, (size_t)t->th.d.G * 16, hipMemcpyDefault, e->stream));
            roots = t->d_root_states;
        }
        launch_reset_trees(t->th.d, nullptr, e->stream, roots);
        launch_harvest(t->th.d, t->th.d_totals, nullptr, e->stream);          // forget the old trees' counters
        HIPCHK(hipMemsetAsync(t->th.d_totals, 0, ST_TOTALS * sizeof(unsigned long long), e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        return AZ_OK;
    } catch (const HipFail& f) { return fail_hip(e, f); }
}

az_status az_tree_record_evals(az_tree* t, int32_t cap) {
    if (!t || cap < 0) return AZ_ERR_BAD_ARGUMENT;
    if (t->shared) return fail(t->e, AZ_ERR_BAD_ARGUMENT, "az_tree_record_evals on a shared tree batch (it would rebuild held slots' trees)");
    try {
        HIPCHK(hipSetDevice(t->e->device));
        TreeDev& d = t->th.d;
        d.log_cap = cap;
        d.log_state = t->mem.alloc<ulonglong2>((size_t)d.G * cap);
        d.log_pi = t->mem.alloc<float>((size_t)d.G * cap * 7);
        d.log_v = t->mem.alloc<float>((size_t)d.G * cap);
        launch_reset_trees(d, nullptr, t->e->stream);      // the log starts with fresh trees (log_len = 0)
        HIPCHK(hipStreamSynchronize(t->e->stream));
        return AZ_OK;
    } catch (const HipFail& f) { return fail_hip(t->e, f); }
}

az_status az_tree_get_evals(az_tree* t, int32_t* rec_count, uint64_t* states, float* pis, float* vs) {
    if (!t) return AZ_ERR_BAD_ARGUMENT;
    try {
        HIPCHK(hipSetDevice(t->e->device));
        TreeDev& d = t->th.d;
        size_t n = (size_t)d.G * d.log_cap;
        if (rec_count) {
            std::vector<TreeLine> heads(d.G);
            HIPCHK(hipMemcpy(heads.data(), d.head, (size_t)d.G * sizeof(TreeLine), hipMemcpyDeviceToHost));
            std::vector<int32_t> cnt(d.G);
            for (int g = 0; g < d.G; ++g) cnt[g] = (int32_t)heads[g].head.log_len;
            HIPCHK(hipMemcpy(rec_count, cnt.data(), d.G * sizeof(int32_t), hipMemcpyDefault));
        }
        if (states) HIPCHK(hipMemcpy(states, d.log_state, n * 16, hipMemcpyDefault));
        if (pis) HIPCHK(hipMemcpy(pis, d.log_pi, n * 7 * sizeof(float), hipMemcpyDefault));
        if (vs) HIPCHK(hipMemcpy(vs, d.log_v, n * sizeof(float), hipMemcpyDefault));
        return AZ_OK;
    } catch (const HipFail& f) { return fail_hip(t->e, f); }
}

az_status az_tree_node_counts(az_tree* t, uint32_t* out) {
    if (!t || !out) return AZ_ERR_BAD_ARGUMENT;
    try {
        HIPCHK(hipSetDevice(t->e->device));
        std::vector<TreeLine> heads(t->th.d.G);
        HIPCHK(hipMemcpy(heads.data(), t->th.d.head, heads.size() * sizeof(TreeLine), hipMemcpyDeviceToHost));
        std::vector<uint32_t> cnt(heads.size());
        for (size_t g = 0; g < heads.size(); ++g) cnt[g] = heads[g].head.count;
        HIPCHK(hipMemcpy(out, cnt.data(), cnt.size() * sizeof(uint32_t), hipMemcpyDefault));
        return AZ_OK;
    } catch (const HipFail& f) { return fail_hip(t->e, f); }
}

az_status az_tree_get_action_prob(az_tree* t, const uint64_t* states, float temp, uint64_t seed, uint64_t first_game_id,
                                  float* pi, uint16_t* counts, float* q) {
    if (!t || !states || !pi) return AZ_ERR_BAD_ARGUMENT;
    az_engine* e = t->e;
    if (az_status sr = session_refusal(e, "az_tree_get_action_prob")) return sr;       // a search sizes, clears and retags the evaluation cache
    if (t->shared) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_tree_get_action_prob on a shared tree batch: use az_tree_slot_get_action_prob");
    NetModel* net;
    az_status st = find_net(e, t->model_id, &net);
    if (st) return st;
    st = check_batch(e, *net, t->th.d.G * t->th.d.T);
    if (st) return st;
    st = gumbel_refusal(e, t->th.d.T, "az_tree_get_action_prob");
    if (st) return st;
    st = stop_refusal(e, t->th.d.T, "az_tree_get_action_prob", true);
    if (st) return st;
    ScopedTimer timer{e};
    try {
        HIPCHK(hipSetDevice(e->device));
        TreeDev& d = t->th.d;
        const int G = d.G;
        // include/az_engine.h: caller pointers may be host or device memory.  Host memory takes the pinned fast path (one stream
        // synchronisation per call); device memory is copied by the runtime.
        if (on_device(states)) {
            HIPCHK(hipMemcpyAsync(t->d_root_states, states, (size_t)G * 16, hipMemcpyDeviceToDevice, e->stream));
        } else {
            std::memcpy(t->h_states, states, (size_t)G * 16);
            HIPCHK(hipMemcpyAsync(t->d_root_states, t->h_states, (size_t)G * 16, hipMemcpyHostToDevice, e->stream));
        }
        RootMove mv = root_move_for(e, t->th, t->num_sims, (float)t->cpuct, true);
        if (temp == 0.0f) mv.stop = stop_for(e, t->num_sims, INT32_MIN);        // (another temperature: no move is eligible, the call runs feature-off)
        launch_set_active(d, mv.stop.on ? stop_word((uint32_t)t->num_sims, true) : 1u, e->stream);
        t->last_gumbel = mv.gumbel.m != 0u;
        if (uses_root_stream(mv)) {      // tree g's stream: (seed, first_game_id + g), from device memory so the search graph survives the call's seed
            launch_noise_streams(t->d_noise_streams, G, seed, first_game_id, e->stream);
            mv.stream.stream = t->d_noise_streams;
        }
        if (mv.gumbel.m != 0u) mv.gumbel.temp_threshold = temp == 0.0f ? INT32_MIN : INT32_MAX;
        ScopedRootMove armed;
        armed.install(t->th, mv);
        SearchParams sp{(uint32_t)t->max_depth, (float)t->cpuct};
        prepare_cache(e, dedup_applies(e, *net), (uint64_t)G * ((uint64_t)t->num_sims + 1), e->stream);
        run_search(e, t->th, t->d_root_states, t->num_sims, sp, *net, G);
        launch_root_policy(d, temp, seed, first_game_id, t->h_pi, t->h_counts, t->h_q, e->stream);
        launch_stop_count(d, nullptr, e->stream);
        launch_harvest(d, t->th.d_totals, t->th.d_counts, e->stream);
        launch_call_readback(t->th.d_totals, e->cache.stat, d.err, t->h_rb, e->stream);
        HIPCHK(hipStreamSynchronize(e->stream));
        if (mv.stop.on) fold_stop(e);
        resolve_profile(e);
        fold_dedup(e, t->h_rb->dd);
        fold_tree_totals(e, t->h_rb->totals, dedup_applies(e, *net));
        e->stats.moves += (uint64_t)G;
        st = report_tree_errors(e, t->th, t->h_rb->err);
        if (st) return st;
        auto copy_out = [&](void* dst, const void* src, size_t bytes) {
            if (on_device(dst)) HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
            else std::memcpy(dst, src, bytes);
        };
        copy_out(pi, t->h_pi, (size_t)G * 7 * sizeof(float));
        if (counts) copy_out(counts, t->h_counts, (size_t)G * 7 * sizeof(uint16_t));
        if (q) copy_out(q, t->h_q, (size_t)G * 7 * sizeof(float));
        return AZ_OK;
    } catch (const HipFail& f) { return fail_hip(e, f); }
}

// The device sampler alone (csrc/az_noise.h as the search kernels run it) for n roots at the engine's current alpha.
az_status az_root_noise_eta(az_engine* e, int32_t n, uint64_t seed, const uint64_t* game_ids, const uint64_t* states, float* eta_out) {
    return per_root_values(e, "az_root_noise_eta", n, game_ids, states, eta_out, [&](const uint64_t* d_ids, const ulonglong2* d_states, float* d_eta) {
        launch_root_noise_eta(e->cfg.game, n, seed, d_ids, d_states, (float)((double)e->root_noise_alpha_e6 / 1e6), d_eta, e->stream);
    });
}

// The selected action of each tree's last az_tree_get_action_prob when that was a Gumbel move ("gumbel_m"), else -1.
az_status az_tree_get_selected(az_tree* t, int32_t* actions) {
    if (!t || !actions) return AZ_ERR_BAD_ARGUMENT;
    az_engine* e = t->e;
    try {
        HIPCHK(hipSetDevice(e->device));
        const size_t G = (size_t)t->th.d.G;
        if (t->last_gumbel) {
            HIPCHK(hipMemcpy(actions, t->th.gz_selected, G * sizeof(int32_t), hipMemcpyDefault));
        } else {
            const std::vector<int32_t> none(G, -1);
            HIPCHK(hipMemcpy(actions, none.data(), G * sizeof(int32_t), hipMemcpyDefault));
        }
        return AZ_OK;
    } catch (const HipFail& f) { return fail_hip(e, f); }
}

// The device's Gumbel variates alone (csrc/az_gumbel.h as the search kernels run it) for n roots: g_out[i][a], 0 for an invalid action.
az_status az_gumbel_values(az_engine* e, int32_t n, uint64_t seed, const uint64_t* game_ids, const uint64_t* states, int32_t temp_is_zero, float* g_out) {
    return per_root_values(e, "az_gumbel_values", n, game_ids, states, g_out, [&](const uint64_t* d_ids, const ulonglong2* d_states, float* d_g) {
        launch_gumbel_values(e->cfg.game, n, seed, d_ids, d_states, temp_is_zero != 0, d_g, e->stream);
    });
}

// ---- az_reanalyse (include/az_reanalyse.h) -------------------------------------------------------------------------
// A window of stored positions through a pool of G trees, chunk after chunk on the engine's stream: arm (roots, reset flags, active bits,
// streams), reset, the unchanged search, emit (rows [off, off + k) of the staged outputs), harvest.  Every search takes the same number of
// steps, so no tree is refilled inside a chunk.  The host waits twice: for the check's verdict (a refused window searches nothing) and at
// the end (the counters, the error words, the outputs).
az_status az_reanalyse(az_engine* e, const az_reanalyse_params* p, int64_t n, const uint64_t* states, const float* boards, const uint64_t* game_ids,
                       float* pi, float* root_q, float* root_prior, uint16_t* counts, float* q, int32_t* selected) {
    if (!e) return AZ_ERR_BAD_ARGUMENT;
    if (az_status sr = session_refusal(e, "az_reanalyse")) return sr;                 // a search sizes, clears and retags the evaluation cache
    if (!p) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_reanalyse: the params are required");
    if (n < 0 || n > REANALYSE_MAX_POSITIONS) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_reanalyse: 0 .. 2^24 positions");
    if (e->cfg.game != AZ_GAME_CONNECT_FOUR) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_reanalyse: the position check is Connect Four's (az_config.game = 0)");
    if (p->num_sims < 1 || p->reserve < 8 || p->max_depth < 0 || p->concurrent < 0)
        return fail(e, AZ_ERR_BAD_ARGUMENT, "az_reanalyse: num_sims >= 1, reserve >= 8, max_depth >= 0 and concurrent >= 0 are required");
    if (p->concurrent > 1024 * 64) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_reanalyse: at most 65536 trees per chunk");
    int T = p->num_sim_threads;
    if (az_status st = check_threads(e, p->num_sims, &T)) return st;
    if (az_status st = gumbel_refusal(e, T, "az_reanalyse")) return st;
    if (e->forced_playouts_k_e6 > 0 && T > 1) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_reanalyse: forced_playouts_k_e6 needs num_sim_threads = 1");
    if (az_status st = stop_refusal(e, T, "az_reanalyse", true)) return st;
    if (n == 0) return AZ_OK;
    if (!pi) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_reanalyse: pi is required");
    if (!states && !boards) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_reanalyse: states or boards are required");
    NetModel* net;
    if (az_status st = find_net(e, p->model_id, &net)) return st;
    int G = p->concurrent;
    if (G == 0) {
        G = REANALYSE_DEFAULT_CONCURRENT;
        if (net->kind == AZ_NET_CONV) G = std::max(1, std::min(G, e->cfg.max_batch / T));
    }
    G = (int)std::min<int64_t>(G, n);
    if (az_status st = check_batch(e, *net, G * T)) return st;
    const uint64_t nodes = std::min<uint64_t>(p->reserve, reachable_slots(p->num_sims, AZ_MAX_PLIES));      // az_tree_create's capacity threshold
    // every tree is built at its position and searched once: the root's two blocks and one per expansion
    const uint64_t blocks = reachable_blocks(p->num_sims, 1, nodes);
    if (az_status cs = check_tree_slots(e, blocks)) return cs;
    ScopedTimer timer{e};
    try {
        HIPCHK(hipSetDevice(e->device));
        hipStream_t s = e->stream;
        const size_t N = (size_t)n, Gs = (size_t)G;
        Carve c;
        // [hdr: verdict words, the call's readback] [inputs] [validated states] [game ids] [the six outputs] [the chunk's roots, streams, flags]
        const size_t o_hdr = c.need(512), o_in = c.need(states ? N * 16 : N * AZ_FEATURES * 4), o_st = c.need(N * 16), o_id = c.need(game_ids ? N * 8 : 0),
                     o_pi = c.need(N * 28), o_rq = c.need(root_q ? N * 4 : 0), o_rp = c.need(root_prior ? N * 28 : 0), o_cn = c.need(counts ? N * 14 : 0),
                     o_q = c.need(q ? N * 28 : 0), o_sel = c.need(selected ? N * 4 : 0), o_roots = c.need(Gs * 16), o_streams = c.need(Gs * 16),
                     o_flags = c.need(Gs);
        char* base = (char*)e->reanalyse_scratch.fit(c.total, s);
        uint32_t* d_verdict = (uint32_t*)(base + o_hdr);
        CallReadback* d_rb = (CallReadback*)(base + o_hdr + 256);
        static_assert(sizeof(CallReadback) <= 256 && RV_COUNT * sizeof(uint32_t) <= 256, "the header holds both");
        // the whole window is staged once
        HIPCHK(hipMemsetAsync(d_verdict, 0xFF, 256, s));
        HIPCHK(hipMemcpyAsync(base + o_in, states ? (const void*)states : (const void*)boards, states ? N * 16 : N * AZ_FEATURES * 4, hipMemcpyDefault, s));
        const uint64_t* d_ids = nullptr;
        if (game_ids) {
            HIPCHK(hipMemcpyAsync(base + o_id, game_ids, N * 8, hipMemcpyDefault, s));
            d_ids = (const uint64_t*)(base + o_id);
        }
        ulonglong2* d_states = (ulonglong2*)(base + o_st);
        launch_reanalyse_check(states ? (const SampleState*)(base + o_in) : nullptr, states ? nullptr : (const float*)(base + o_in), n, d_states, d_verdict, s);
        const uint32_t first = read_verdict(d_verdict + RV_FIRST, s);      // the first wait: a refused window searches nothing
        if (first != 0xFFFFFFFFu)
            return fail(e, AZ_ERR_BAD_ARGUMENT, "az_reanalyse: position " + std::to_string(first >> 7) + ": " + reanalyse_bad_text(first & 0x7Fu));
        TreeLease lease;
        acquire_trees(e, lease, G, blocks, nodes, hash_entries(p->num_sims, 1), T, s);
        TreeHost& th = *lease;
        ulonglong2* d_roots = (ulonglong2*)(base + o_roots);
        ulonglong2* d_streams = (ulonglong2*)(base + o_streams);
        uint8_t* d_flags = (uint8_t*)(base + o_flags);
        const ReanalyseOut out{(float*)(base + o_pi), root_q ? (float*)(base + o_rq) : nullptr, root_prior ? (float*)(base + o_rp) : nullptr,
                               counts ? (uint16_t*)(base + o_cn) : nullptr, q ? (float*)(base + o_q) : nullptr,
                               selected ? (int32_t*)(base + o_sel) : nullptr};
        // the root-move record of az_tree_get_action_prob, each tree on its own (seed, game id)
        RootMove mv = root_move_for(e, th, p->num_sims, (float)p->cpuct, true);
        if (uses_root_stream(mv)) mv.stream.stream = d_streams;
        if (mv.gumbel.m != 0u) mv.gumbel.temp_threshold = p->temp == 0.0f ? INT32_MIN : INT32_MAX;
        if (p->temp == 0.0f) mv.stop = stop_for(e, p->num_sims, INT32_MIN);      // as the tree call arms it
        ScopedRootMove armed;
        armed.install(th, mv);
        const SearchParams sp{(uint32_t)p->max_depth, (float)p->cpuct};
        prepare_cache(e, dedup_applies(e, *net), (uint64_t)n * ((uint64_t)p->num_sims + 1), s);
        // chunks back to back; every chunk's search is sized by the pool (one captured graph serves them all, the short last one included)
        for (int64_t off = 0; off < n; off += G) {
            const int k = (int)std::min<int64_t>(G, n - off);
            launch_reanalyse_arm(th.d, d_states, d_ids, p->seed, p->first_game_id, off, k, d_roots, d_streams, d_flags, s);
            launch_reset_trees(th.d, d_flags, s, d_roots);
            run_search(e, th, d_roots, p->num_sims, sp, *net, G);
            launch_reanalyse_emit(th.d, p->temp, d_streams, off, k, out, d_verdict, s);
            launch_stop_count(th.d, nullptr, s);
            launch_harvest(th.d, th.d_totals, nullptr, s);
        }
        launch_call_readback(th.d_totals, e->cache.stat, th.d.err, d_rb, s);
        CallReadback rb;
        uint32_t verdict[RV_COUNT];
        HIPCHK(hipMemcpyAsync(&rb, d_rb, sizeof rb, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(verdict, d_verdict, sizeof verdict, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(pi, out.pi, N * 28, hipMemcpyDefault, s));
        if (root_q) HIPCHK(hipMemcpyAsync(root_q, out.root_q, N * 4, hipMemcpyDefault, s));
        if (root_prior) HIPCHK(hipMemcpyAsync(root_prior, out.root_prior, N * 28, hipMemcpyDefault, s));
        if (counts) HIPCHK(hipMemcpyAsync(counts, out.counts, N * 14, hipMemcpyDefault, s));
        if (q) HIPCHK(hipMemcpyAsync(q, out.q, N * 28, hipMemcpyDefault, s));
        if (selected) HIPCHK(hipMemcpyAsync(selected, out.selected, N * 4, hipMemcpyDefault, s));
        HIPCHK(hipStreamSynchronize(s));                    // the second wait
        HIPCHK(hipGetLastError());
        if (mv.stop.on) fold_stop(e);
        resolve_profile(e);
        fold_dedup(e, rb.dd);
        fold_tree_totals(e, rb.totals, dedup_applies(e, *net));
        e->stats.moves += (uint64_t)n;
        if (az_status st = report_tree_errors(e, th, rb.err)) {
            const std::string where = verdict[RV_FULL] != 0xFFFFFFFFu ? "position " + std::to_string(verdict[RV_FULL])
                                                                       : "a position of the chunk at " + std::to_string(verdict[RV_CHUNK]);
            return fail(e, st, "az_reanalyse: " + where + ": " + e->err);
        }
        return AZ_OK;
    } catch (const HipFail& f) { return fail_hip(e, f); }
}

// ---- shared tree batch: many host threads, one slot (one AsyncMcts) each ---------------------------------------------------
az_status az_tree_share(az_tree* t, int32_t window_us) {
    if (!t || window_us < 0) return AZ_ERR_BAD_ARGUMENT;
    if (t->shared) {                        // already shared: only the window changes
        t->shared->comb.set_window_us(window_us);
        return AZ_OK;
    }
    az_engine* e = t->e;
    if (az_status sr = session_refusal(e, "az_tree_share")) return sr;
    try {
        HIPCHK(hipSetDevice(e->device));
        const int G = t->th.d.G;
        std::unique_ptr<SharedTrees> sh(new SharedTrees(G, t));
        sh->d_req = sh->mem.alloc<SlotReq>((size_t)G);
        sh->d_reset = sh->mem.alloc<uint8_t>((size_t)G);
        HIPCHK(hipMemset(sh->d_reset, 0, (size_t)G));
        HIPCHK(hipHostMalloc(&sh->h_io, (size_t)G * (sizeof(SlotReq) + sizeof(SlotOut)), hipHostMallocDefault));
        sh->h_req = (SlotReq*)sh->h_io;
        sh->h_out = (SlotOut*)(sh->h_req + G);
        sh->comb.set_window_us(window_us);
        HIPCHK(hipStreamSynchronize(e->stream));
        t->shared = std::move(sh);
        return AZ_OK;
    } catch (const HipFail& f) { return fail_hip(e, f); }
}

// The slot calls below run on many host threads at once: they touch no engine-wide state (az_last_error included) and make no
// HIP call except as the batch's leader (SlotRunner).
az_status az_tree_slot_acquire(az_tree* t, int32_t* slot) {
    if (!t || !slot || !t->shared) return AZ_ERR_BAD_ARGUMENT;
    const int s = t->shared->comb.acquire();
    if (s < 0) return AZ_ERR_CAPACITY;
    t->shared->err[(size_t)s][0] = 0;
    *slot = s;
    return AZ_OK;
}

az_status az_tree_slot_release(az_tree* t, int32_t slot) {
    if (!t || !t->shared) return AZ_ERR_BAD_ARGUMENT;
    return t->shared->comb.release(slot) ? AZ_OK : AZ_ERR_BAD_ARGUMENT;
}

az_status az_tree_slot_get_action_prob(az_tree* t, int32_t slot, const uint64_t* state, float temp, uint64_t seed, uint64_t game_id,
                                       float* pi, uint16_t* counts, float* q) {
    if (!t || !t->shared) return AZ_ERR_BAD_ARGUMENT;
    SharedTrees& sh = *t->shared;
    if (!state || !pi) {
        if (sh.comb.holds(slot)) set_slot_error(sh, slot, "az_tree_slot_get_action_prob: state and pi are required");
        return AZ_ERR_BAD_ARGUMENT;
    }
    // a batch shared before the session was opened: its searches would run prepare_cache under the session.  No slot call is in flight
    // while another entry runs on the engine (the header's threading rule), so the session pointer is stable here
    if (t->e->sp_session) {
        if (sh.comb.holds(slot)) set_slot_error(sh, slot, "az_tree_slot_get_action_prob: refused while a self-play session is open (az_selfplay_end first)");
        return AZ_ERR_BAD_ARGUMENT;
    }
    SlotCall c{state, temp, seed, game_id, pi, counts, q, AZ_ERR_HIP};
    if (!sh.comb.submit(slot, &c)) return AZ_ERR_BAD_ARGUMENT;      // out of range, not held, or a call already in flight
    return c.status;
}

const char* az_tree_slot_error(const az_tree* t, int32_t slot) {
    if (!t || !t->shared || slot < 0 || slot >= t->th.d.G) return "";
    return t->shared->err[(size_t)slot].data();
}

az_status az_tree_share_stats(az_tree* t, uint64_t* out) {
    if (!t || !out || !t->shared) return AZ_ERR_BAD_ARGUMENT;
    const CombineStats cs = t->shared->comb.stats();
    out[0] = cs.batches; out[1] = cs.requests; out[2] = cs.largest; out[3] = cs.by_window;
    return AZ_OK;
}

// ---- Coach::execute_episode x many -----------------------------------------------------------
// ---- Coach::execute_episode x many, as a SESSION: the slots stay full across the calls that fetch the episodes -------------------------
// az_selfplay_begin fixes the session's episodes (ids 0 .. n_games-1, slot refill in id order); az_selfplay_next(k) plays until the next k
// episodes IN ID ORDER are finished and emits their tuples -- the slots those episodes freed are already playing later ones, so a host
// that fetches its episodes in chunks pays the drain (the last few slots finishing alone: 6 % of a 65536-episode call) once per session
// instead of once per chunk.  An episode depends on (seed, first_game_id + index) and the net alone, so a chunk's tuples are the ones
// az_selfplay would return for the same episodes.  az_selfplay is begin + next(all) + end.
struct SelfplaySession {
    az_selfplay_params p{};
    int C = 0, T = 1, n_games = 0;
    NetModel* net = nullptr;
    uint64_t net_generation = 0;
    TreeLease lease;
    DeviceMem mem;
    ScopedEvalLog evlog;
    ScopedRootMove armed;                // the session's root-move record on the leased arena, for the session's life
    GamesDev gd{};
    SearchRecDev rec{};                  // "selfplay_record_search": both nullptr while the option is off
    SearchParams sp{};
    SelfplayMoveParams mp{};
    uint32_t* h_ctr = nullptr;           // pinned read-back of gd.counters
    int active = 0, rows_typ = 0;
    int round_sims = 0;                  // lock-step: simulation steps of the next move round (playout cap: the largest budget among the slots' moves)
    int delivered = 0;                   // episodes handed out by az_selfplay_next so far
    long long iter = 0;
    bool async_mode = false;
    // free-running mode (selfplay_async)
    EvalBatch B[2];
    EvalCache ec{};
    int fill = 0;
    long long step = 0;
    ~SelfplaySession() { if (h_ctr) (void)hipHostFree(h_ctr); }
};

static az_status selfplay_begin_impl(az_engine* e, const az_selfplay_params* p, std::unique_ptr<SelfplaySession>& out) {
    if (p->n_games <= 0 || p->num_sims <= 0 || p->max_depth < 0 || p->reserve < 8)
        return fail(e, AZ_ERR_BAD_ARGUMENT, "az_selfplay: bad argument");
    const int n_games = p->n_games;
    const int C = (p->concurrent <= 0 || p->concurrent > n_games) ? n_games : p->concurrent;
    if (C > 1024 * 64) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_selfplay: at most 65536 concurrent games");
    NetModel* net;
    az_status st = find_net(e, p->model_id, &net);
    if (st) return st;
    int T = p->num_sim_threads;
    st = check_threads(e, p->num_sims, &T);
    if (st) return st;
    st = check_batch(e, *net, C * T);
    if (st) return st;
    st = gumbel_refusal(e, T, "az_selfplay");
    if (st) return st;
    st = stop_refusal(e, T, "az_selfplay", true);
    if (st) return st;
    if (e->selfplay_record_search && e->selfplay_async)
        return fail(e, AZ_ERR_BAD_ARGUMENT, "az_selfplay: selfplay_record_search and selfplay_async exclude each other");
    const int cap_sims = (int)e->playout_cap_sims;
    if (cap_sims > 0 && cap_sims >= p->num_sims) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_selfplay: playout_cap_sims must be below num_sims");
    if (cap_sims > 0 && cap_sims % T != 0) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_selfplay: playout_cap_sims % num_sim_threads != 0");
    HIPCHK(hipSetDevice(e->device));
    hipStream_t s = e->stream;
    const uint64_t nodes = std::min<uint64_t>(p->reserve, reachable_slots(p->num_sims, AZ_MAX_PLIES));
    if (az_status cs = check_tree_slots(e, reachable_blocks(p->num_sims, AZ_MAX_PLIES, nodes))) return cs;
    std::unique_ptr<SelfplaySession> ss(new SelfplaySession());
    ss->p = *p; ss->C = C; ss->T = T; ss->n_games = n_games; ss->net = net; ss->net_generation = net->generation;
    acquire_trees(e, ss->lease, C, reachable_blocks(p->num_sims, AZ_MAX_PLIES, nodes), nodes, hash_entries(p->num_sims, AZ_MAX_PLIES), T, s);
    TreeHost& th = *ss->lease;
    DeviceMem& mem = ss->mem;
    GamesDev& gd = ss->gd;
    gd.C = C;
    gd.n_games = n_games;
    gd.state = mem.alloc<ulonglong2>(C);
    gd.player = mem.alloc<int8_t>(C);
    gd.ply = mem.alloc<int32_t>(C);
    gd.gid = mem.alloc<int32_t>(C);
    gd.need_reset = mem.alloc<uint8_t>(C);
    const size_t ns = (size_t)n_games * 42;
    gd.smp_state = mem.alloc<ulonglong2>(ns);
    gd.smp_pi = mem.alloc<float>(ns * 7);
    gd.smp_player = mem.alloc<int8_t>(ns);
    gd.moves = mem.alloc<uint8_t>(ns);
    gd.g_len = mem.alloc<int32_t>(n_games);
    gd.g_result = mem.alloc<float>(n_games);
    gd.g_final_player = mem.alloc<int8_t>(n_games);
    gd.counters = mem.alloc<uint32_t>(8);
    if (e->selfplay_record_search) {
        ss->rec.root_q = mem.alloc<float>(ns);
        ss->rec.root_prior = mem.alloc<float>(ns * 7);
    }
    if (p->record_evals > 0) {
        // per-EPISODE logs (row = the slot's current episode id), so they survive slot refills
        gd.g_log_len = mem.alloc<int32_t>(n_games);
        HIPCHK(hipMemset(gd.g_log_len, 0, n_games * sizeof(int32_t)));
        ss->evlog.attach(th, (size_t)n_games, p->record_evals, gd.gid);
    }
    {
        std::vector<int32_t> gid(C);
        std::vector<int8_t> pl(C, 1);
        for (int i = 0; i < C; ++i) gid[i] = i;
        HIPCHK(hipMemcpy(gd.gid, gid.data(), C * sizeof(int32_t), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(gd.player, pl.data(), C, hipMemcpyHostToDevice));
        HIPCHK(hipMemset(gd.state, 0, (size_t)C * 16));
        HIPCHK(hipMemset(gd.ply, 0, C * sizeof(int32_t)));
        HIPCHK(hipMemset(gd.need_reset, 0, C));
        HIPCHK(hipMemset(gd.moves, 0, ns));
        HIPCHK(hipMemset(gd.g_len, 0, n_games * sizeof(int32_t)));
        uint32_t ctr[8] = {(uint32_t)C, 0u, (uint32_t)C, 0u, 0u, 0u, 0u, 0u};
        HIPCHK(hipMemcpy(gd.counters, ctr, sizeof ctr, hipMemcpyHostToDevice));
    }
    ss->round_sims = p->num_sims;
    // the session's root-move record: forced playouts and the Gumbel rule on the full moves only under a playout cap, the budget of a full move
    RootMove mv = root_move_for(e, th, p->num_sims, (float)p->cpuct, true);
    if (uses_root_stream(mv)) mv.stream = RootStream{p->seed, p->first_game_id, gd.gid, nullptr};      // (seed, first_game_id + the slot's episode, ply)
    if (mv.gumbel.m != 0u) mv.gumbel.temp_threshold = p->temp_threshold;
    mv.stop = stop_for(e, p->num_sims, p->temp_threshold);       // the session captures the switch here
    if (cap_sims > 0) {
        // the slots' first moves (ply 0 of episodes 0 .. C-1) are drawn here; every later one by the move that precedes it (selfplay_move_body)
        PlayoutCap cap{mem.alloc<uint32_t>(C), (uint32_t)p->num_sims, (uint32_t)cap_sims, playout_cap_thresh24((uint64_t)e->playout_cap_full_e6)};
        std::vector<uint32_t> w((size_t)C);
        uint32_t most = 0;
        for (int i = 0; i < C; ++i) {
            w[(size_t)i] = playout_cap_word(p->seed, p->first_game_id + (uint64_t)i, 0ull, cap.thresh24, cap.num_sims, cap.cap_sims);
            most = std::max(most, w[(size_t)i] & ~PLAYOUT_FULL_BIT);
        }
        HIPCHK(hipMemcpy(cap.word, w.data(), (size_t)C * sizeof(uint32_t), hipMemcpyHostToDevice));
        gd.g_full = mem.alloc<unsigned long long>(n_games);
        HIPCHK(hipMemset(gd.g_full, 0, (size_t)n_games * sizeof(unsigned long long)));
        mv.cap = cap;
        ss->round_sims = (int)most;
    }
    ss->armed.install(th, mv);
    launch_reset_trees(th.d, nullptr, s);
    prepare_cache(e, dedup_applies(e, *net), (uint64_t)n_games * AZ_MAX_PLIES * ((uint64_t)p->num_sims + 1), s);
    ss->sp = SearchParams{(uint32_t)p->max_depth, (float)p->cpuct};
    ss->mp = SelfplayMoveParams{p->seed, p->first_game_id, p->temp_threshold, C < n_games ? 1 : 0, 0, 0};
    HIPCHK(hipHostMalloc((void**)&ss->h_ctr, 8 * sizeof(uint32_t)));
    ss->active = C;                               // slots still playing (read back after every move)
    ss->rows_typ = 0;                             // expected rows per leaf batch (0 = unknown: assume `active`)
    // "selfplay_async": free-running slots (k_async_step) -- conv nets (anything that goes through leaf batches), one simulation in
    // flight per tree.  `launches` tree launches share one leaf batch, then the forward runs on it.
    ss->async_mode = e->selfplay_async != 0 && T == 1 && (net->kind == AZ_NET_CONV || dedup_applies(e, *net)) && p->num_sims >= 1;
    if (ss->async_mode) {
        gd.sims = mem.alloc<int32_t>(C);
        HIPCHK(hipMemsetAsync(gd.sims, 0xFF, (size_t)C * sizeof(int32_t), s));       // -1: no root prepared yet
        launch_selfplay_sync_active(th.d, gd, s);
        th.d.block4 = e->tree_block4;
        const bool dedup = dedup_applies(e, *net);
        ss->ec = cache_for(e, *net);
        ss->B[0] = th.eb; ss->B[1] = th.eb2;
        ss->B[0].dedup = ss->B[1].dedup = dedup ? 1 : 0;
        ss->B[0].mirror = ss->B[1].mirror = mirror_applies(e, *net) ? 1 : 0;
        ss->B[0].max_n = ss->B[1].max_n = gd.counters + 3;
    }
    out = std::move(ss);
    return AZ_OK;
}

// play until every episode below `hi` has finished (the counter of finished episodes is restarted for the range [delivered, hi))
static az_status selfplay_run_until(az_engine* e, SelfplaySession& ss, int hi) {
    hipStream_t s = e->stream;
    TreeHost& th = *ss.lease;
    GamesDev& gd = ss.gd;
    NetModel* net = ss.net;
    const az_selfplay_params* p = &ss.p;
    const int C = ss.C, T = ss.T, n_games = ss.n_games, lo = ss.delivered;
    uint32_t* h_ctr = ss.h_ctr;
    ss.mp.done_lo = lo; ss.mp.done_hi = hi;
    launch_count_done(gd.g_len, lo, hi, gd.counters + 1, s);
    const uint32_t want = (uint32_t)(hi - lo);
    az_status result = AZ_OK;
    {   // a chunk whose episodes all finished while earlier ones were being waited for
        HIPCHK(hipMemcpyAsync(h_ctr, gd.counters, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (h_ctr[1] >= want) return AZ_OK;
    }
    if (ss.async_mode) {
        const int launches = std::max(1, e->selfplay_async_launches), iters = std::max(2, e->selfplay_async_iters);
        const int every = std::max(1, e->profile_every);
        // every leaf costs a forward at the latest `launches` launches after it was requested; a move needs num_sims + 2 leaves
        const long long cap_steps = (long long)(AZ_MAX_PLIES + 2) * (n_games / C + 2) * ((long long)p->num_sims + 3) + 64;
        for (;; ++ss.step) {
            const bool timed = e->prof.on && (e->profile_tick++ % (uint64_t)every) == 0;
            for (int j = 0; j < launches; ++j) {
                hipEvent_t t0 = nullptr;
                if (timed && j == 0) t0 = e->prof.begin(s);
                launch_async_step(th.d, gd, ss.B[ss.fill ^ 1], ss.B[ss.fill], ss.ec, ss.sp, ss.mp, p->num_sims, j == 0 ? 1 : 0, iters, s);
                if (timed && j == 0) { e->prof.end(t0, RG_TREE, s); e->stats.tree_launches_timed += 1; }
                e->stats.tree_launches += 1;
            }
            if (ss.mp.refill) launch_reset_trees(th.d, gd.need_reset, s);
            net_forward(e, *net, ss.B[ss.fill], ss.active, s, ss.rows_typ, timed);
            ss.fill ^= 1;
            if ((ss.step & 15) == 15) {                  // look at the counters now and then: finished? how many slots still play?
                HIPCHK(hipMemcpyAsync(h_ctr, gd.counters, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
                HIPCHK(hipStreamSynchronize(s));
                resolve_profile(e);
                ss.active = std::max(1, (int)h_ctr[2]);
                ss.rows_typ = h_ctr[3] ? (int)std::min<uint32_t>(h_ctr[3], (uint32_t)C) : 0;
                HIPCHK(hipMemsetAsync(gd.counters + 3, 0, sizeof(uint32_t), s));
                if (h_ctr[1] >= want) { ++ss.step; break; }
                result = check_tree_errors(e, th);
                if (result) break;
                if (ss.step > cap_steps) { result = fail(e, AZ_ERR_HIP, "az_selfplay: episode loop did not terminate"); break; }
            }
        }
        return result;
    }
    for (;; ++ss.iter) {
        launch_selfplay_sync_active(th.d, gd, s);
        // tile choice from the largest batch of the previous move (de-duplication makes batches much smaller than the
        // number of searching trees); the grids still cover `active`
        // playout cap: the round runs as many steps as the largest budget among its slots' moves (left by the previous round's move kernel);
        // a tree whose own budget is smaller sits the rest of the round out
        run_search(e, th, gd.state, ss.round_sims, ss.sp, *net, ss.active, nullptr, ss.rows_typ, gd.counters + 3);
        if (ss.rec.root_q) launch_selfplay_record(th.d, gd, ss.rec, s);
        launch_stop_count(th.d, gd.gid, s);
        launch_selfplay_move(th.d, gd, ss.mp, s);
        if (ss.mp.refill) launch_reset_trees(th.d, gd.need_reset, s);
        HIPCHK(hipMemcpyAsync(h_ctr, gd.counters, 5 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        resolve_profile(e);
        ss.active = (int)h_ctr[2];
        ss.rows_typ = h_ctr[3] ? (int)std::min<uint32_t>(h_ctr[3], (uint32_t)(C * T)) : 0;      // this move's largest batch
        if (th.d.move.cap.word) ss.round_sims = h_ctr[4] ? (int)std::min<uint32_t>(h_ctr[4], (uint32_t)p->num_sims) : p->num_sims;
        HIPCHK(hipMemsetAsync(gd.counters + 3, 0, 2 * sizeof(uint32_t), s));
        if (h_ctr[1] >= want) { ++ss.iter; break; }
        if ((ss.iter & 7) == 7 || h_ctr[2] == 0) {
            result = check_tree_errors(e, th);
            if (result) break;
        }
        if (h_ctr[2] == 0) { result = fail(e, AZ_ERR_HIP, "az_selfplay: every slot is idle before the requested episodes finished"); break; }
        if (ss.iter > (long long)AZ_MAX_PLIES * (n_games / C + 2) + 8) {
            result = fail(e, AZ_ERR_HIP, "az_selfplay: episode loop did not terminate");
            break;
        }
    }
    return result;
}

// tuples of the episodes [lo, hi) into `out` (game-id order then ply order)
static az_status selfplay_emit(az_engine* e, SelfplaySession& ss, int lo, int hi, az_samples* out) {
    hipStream_t s = e->stream;
    const az_selfplay_params* p = &ss.p;
    const GamesDev& gd = ss.gd;
    const int n = hi - lo, nsym = p->symmetries ? 2 : 1;
    std::vector<int32_t> glen((size_t)n);
    HIPCHK(hipMemcpy(glen.data(), gd.g_len + lo, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    // the full-ply masks: what az_selfplay_get_full_plies returns.  Without a playout cap every ply is a full move.
    std::vector<uint64_t>& full = e->sp_full_plies;
    full.assign((size_t)n, 0ull);
    if (gd.g_full) HIPCHK(hipMemcpy(full.data(), gd.g_full + lo, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    std::vector<int64_t> off((size_t)n);
    int64_t total = 0, plies = 0;
    for (int i = 0; i < n; ++i) {
        const uint64_t all = (1ull << glen[(size_t)i]) - 1ull;
        full[(size_t)i] = gd.g_full ? (full[(size_t)i] & all) : all;
        off[(size_t)i] = total;
        total += (int64_t)__builtin_popcountll(full[(size_t)i]);          // recorded plies (== game_len without a cap)
        plies += glen[(size_t)i];
    }
    e->stats.games += (uint64_t)n;
    e->stats.moves += (uint64_t)plies;
    e->stats.samples += (uint64_t)total;
    out->count = total * nsym;
    if (out->capacity < out->count) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_selfplay: sample buffers too small");
    const size_t ns = (size_t)n * 42;
    if (out->pis && out->zs) {
        DeviceMem mem;
        int64_t* d_off = mem.alloc<int64_t>((size_t)n);
        HIPCHK(hipMemcpy(d_off, off.data(), (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice));
        const size_t cnt = (size_t)out->count;
        ulonglong2* d_states = out->states ? mem.alloc<ulonglong2>(cnt) : nullptr;
        float* d_boards = out->boards ? mem.alloc<float>(cnt * 84) : nullptr;
        float* d_pis = mem.alloc<float>(cnt * 7);
        float* d_zs = mem.alloc<float>(cnt);
        GamesDev view = gd;          // the per-episode arrays of [lo, hi)
        view.n_games = n;
        view.smp_state += (size_t)lo * 42; view.smp_pi += (size_t)lo * 42 * 7; view.smp_player += (size_t)lo * 42; view.moves += (size_t)lo * 42;
        view.g_len += lo; view.g_result += lo; view.g_final_player += lo;
        if (view.g_full) view.g_full += lo;
        launch_emit_samples(view, d_off, p->symmetries, d_states, d_boards, d_pis, d_zs, s);
        HIPCHK(hipStreamSynchronize(s));
        if (d_states) HIPCHK(hipMemcpy(out->states, d_states, cnt * 16, hipMemcpyDefault));
        if (d_boards) HIPCHK(hipMemcpy(out->boards, d_boards, cnt * 84 * sizeof(float), hipMemcpyDefault));
        HIPCHK(hipMemcpy(out->pis, d_pis, cnt * 7 * sizeof(float), hipMemcpyDefault));
        HIPCHK(hipMemcpy(out->zs, d_zs, cnt * sizeof(float), hipMemcpyDefault));
    }
    if (out->game_len) HIPCHK(hipMemcpy(out->game_len, glen.data(), (size_t)n * sizeof(int32_t), hipMemcpyDefault));
    if (out->moves) HIPCHK(hipMemcpy(out->moves, gd.moves + (size_t)lo * 42, ns, hipMemcpyDefault));
    e->sp_search_valid = ss.rec.root_q != nullptr;
    if (ss.rec.root_q) {             // the search record's rows, emitted as the tuples are (az_selfplay_get_search)
        const size_t cnt = (size_t)out->count;
        e->sp_search_q.assign(cnt, 0.0f);
        e->sp_search_prior.assign(cnt * 7, 0.0f);
        if (cnt) {
            DeviceMem mem;
            int64_t* d_off = mem.alloc<int64_t>((size_t)n);
            HIPCHK(hipMemcpy(d_off, off.data(), (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice));
            float* d_q = mem.alloc<float>(cnt);
            float* d_prior = mem.alloc<float>(cnt * 7);
            GamesDev view = gd;
            view.n_games = n;
            view.g_len += lo;
            if (view.g_full) view.g_full += lo;
            SearchRecDev rv{ss.rec.root_q + (size_t)lo * 42, ss.rec.root_prior + (size_t)lo * 42 * 7};
            launch_emit_search(view, rv, d_off, p->symmetries, d_q, d_prior, s);
            HIPCHK(hipStreamSynchronize(s));
            HIPCHK(hipMemcpy(e->sp_search_q.data(), d_q, cnt * sizeof(float), hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(e->sp_search_prior.data(), d_prior, cnt * 7 * sizeof(float), hipMemcpyDeviceToHost));
        }
    } else {
        e->sp_search_q.clear();
        e->sp_search_prior.clear();
    }
    return AZ_OK;
}

static az_status selfplay_next_impl(az_engine* e, SelfplaySession& ss, int n, az_samples* out) {
    if (ss.net->generation != ss.net_generation) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_selfplay_next: the session's model was changed");
    const int lo = ss.delivered, hi = lo + n;
    az_status result = selfplay_run_until(e, ss, hi);
    harvest_stats(e, *ss.lease, *ss.net);
    if (result == AZ_OK) result = check_tree_errors(e, *ss.lease);
    if (result) return result;
    result = selfplay_emit(e, ss, lo, hi, out);
    if (result) return result;
    ss.delivered = hi;
    if (ss.p.record_evals > 0) {          // the whole session's log so far (rows of unfinished episodes are partial)
        e->sp_log_cap = ss.p.record_evals;
        e->sp_log_count.resize((size_t)ss.n_games);
        HIPCHK(hipMemcpy(e->sp_log_count.data(), ss.gd.g_log_len, (size_t)ss.n_games * sizeof(int32_t), hipMemcpyDeviceToHost));
        ss.evlog.copy_out(e->sp_log_states, e->sp_log_pi, e->sp_log_v);
    }
    return AZ_OK;
}

az_status az_selfplay_begin(az_engine* e, const az_selfplay_params* p) {
    if (!e || !p) return AZ_ERR_BAD_ARGUMENT;
    if (e->sp_session) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_selfplay_begin: a session is open (az_selfplay_end first)");
    try {
        std::unique_ptr<SelfplaySession> ss;
        az_status st = selfplay_begin_impl(e, p, ss);
        if (st) return st;
        e->sp_model_id = p->model_id;
        e->sp_session = ss.release();
        return AZ_OK;
    } catch (const HipFail& f) { return fail_hip(e, f); }
}

az_status az_selfplay_next(az_engine* e, int32_t n_games, az_samples* out) {
    if (!e || !out) return AZ_ERR_BAD_ARGUMENT;
    SelfplaySession* ss = e->sp_session;
    if (!ss) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_selfplay_next: no open session (az_selfplay_begin first)");
    if (n_games <= 0 || ss->delivered + n_games > ss->n_games) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_selfplay_next: more episodes than the session has left");
    if (out->capacity < 0) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_selfplay: negative capacity");
    ScopedTimer timer{e};
    try {
        HIPCHK(hipSetDevice(e->device));
        return selfplay_next_impl(e, *ss, n_games, out);
    } catch (const HipFail& f) { return fail_hip(e, f); }
}

az_status az_selfplay_end(az_engine* e) {
    if (!e) return AZ_ERR_BAD_ARGUMENT;
    if (!e->sp_session) return AZ_OK;
    (void)hipSetDevice(e->device);
    (void)hipStreamSynchronize(e->stream);
    delete e->sp_session;            // the tree arena goes back to the pool, the per-episode arrays are freed
    e->sp_session = nullptr;
    return AZ_OK;
}

az_status az_selfplay(az_engine* e, const az_selfplay_params* p, az_samples* out) {
    if (!e || !p || !out) return AZ_ERR_BAD_ARGUMENT;
    if (out->capacity < 0) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_selfplay: negative capacity");
    if (e->sp_session) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_selfplay: a session is open (az_selfplay_end first)");
    ScopedTimer timer{e};
    try {
        std::unique_ptr<SelfplaySession> ss;
        az_status st = selfplay_begin_impl(e, p, ss);
        if (st) return st;
        st = selfplay_next_impl(e, *ss, ss->n_games, out);
        HIPCHK(hipStreamSynchronize(e->stream));
        return st;
    } catch (const HipFail& f) { return fail_hip(e, f); }
}

// ---- the decided-move stop (include/az_search_stop.h; csrc/az_stop.h) -----------------------------------------------
az_status az_search_stop_set(az_engine* e, int32_t on) {
    if (!e) return AZ_ERR_BAD_ARGUMENT;
    if (on != 0 && on != 1) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_search_stop_set: on must be 0 or 1");
    if (e->sp_session) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_search_stop_set: search_stop cannot change while a self-play session is open");
    if (on && !e->stop_stat) {
        try {
            HIPCHK(hipSetDevice(e->device));
            unsigned long long* p = e->stop_mem.alloc<unsigned long long>(8);
            HIPCHK(hipMemset(p, 0, 8 * sizeof(unsigned long long)));
            e->stop_stat = p;
        } catch (const HipFail& f) { return fail_hip(e, f); }
    }
    e->search_stop = on;
    return AZ_OK;
}
az_status az_search_stop_get(const az_engine* e, int32_t* on) {
    if (!e || !on) return AZ_ERR_BAD_ARGUMENT;
    *on = e->search_stop;
    return AZ_OK;
}
// the counters as the finished calls left them: no device work, so an open session never notices it
az_status az_search_stop_stats(az_engine* e, uint64_t out[4], int32_t reset) {
    if (!e || !out) return AZ_ERR_BAD_ARGUMENT;
    for (int i = 0; i < SS_COUNT; ++i) out[i] = e->stop_totals[i];
    if (reset) for (int i = 0; i < SS_COUNT; ++i) e->stop_totals[i] = 0;
    return AZ_OK;
}

az_status az_selfplay_get_full_plies(az_engine* e, uint64_t* mask) {
    if (!e) return AZ_ERR_BAD_ARGUMENT;
    if (!mask) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_selfplay_get_full_plies: null mask");
    if (!e->sp_full_plies.empty()) std::memcpy(mask, e->sp_full_plies.data(), e->sp_full_plies.size() * sizeof(uint64_t));
    return AZ_OK;
}

az_status az_selfplay_get_search(az_engine* e, float* root_q, float* root_prior) {
    if (!e) return AZ_ERR_BAD_ARGUMENT;
    if (!e->sp_search_valid) return fail(e, AZ_ERR_BAD_ARGUMENT, "no search record (run az_selfplay with selfplay_record_search = 1)");
    try {
        HIPCHK(hipSetDevice(e->device));
        if (root_q && !e->sp_search_q.empty()) HIPCHK(hipMemcpy(root_q, e->sp_search_q.data(), e->sp_search_q.size() * sizeof(float), hipMemcpyDefault));
        if (root_prior && !e->sp_search_prior.empty())
            HIPCHK(hipMemcpy(root_prior, e->sp_search_prior.data(), e->sp_search_prior.size() * sizeof(float), hipMemcpyDefault));
        return AZ_OK;
    } catch (const HipFail& f) { return fail_hip(e, f); }
}

az_status az_selfplay_get_evals(az_engine* e, int32_t* rec_count, uint64_t* states, float* pis, float* vs) {
    if (!e || e->sp_log_cap <= 0) return fail(e, AZ_ERR_BAD_ARGUMENT, "no eval log (run az_selfplay with record_evals > 0)");
    if (rec_count) std::memcpy(rec_count, e->sp_log_count.data(), e->sp_log_count.size() * sizeof(int32_t));
    if (states) std::memcpy(states, e->sp_log_states.data(), e->sp_log_states.size() * 8);
    if (pis) std::memcpy(pis, e->sp_log_pi.data(), e->sp_log_pi.size() * 4);
    if (vs) std::memcpy(vs, e->sp_log_v.data(), e->sp_log_v.size() * 4);
    return AZ_OK;
}

// az_arena_get_openings of a call without openings: every game started from the one position, no random ply
static void record_common_opening(az_engine* e, int G, uint64_t a, uint64_t b) {
    e->ar_open_boards.resize((size_t)G * 2);
    for (int g = 0; g < G; ++g) { e->ar_open_boards[2 * (size_t)g] = a; e->ar_open_boards[2 * (size_t)g + 1] = b; }
    e->ar_open_len.assign((size_t)G, 0);
    e->ar_open_moves.assign((size_t)G * OPENING_MAX_PLIES, 0);
}

// ---- the match driver of az_arena and az_tournament -------------------------------------------------------------
// P = K (K - 1) / 2 pairs of K models play n games each in ONE chain of plies: game p * n + g is game first + g of the pair's arena, and
// model k searches ONE tree batch of the (K - 1) n games it plays in, whichever pair they belong to.  K = 2, P = 1 is az_arena itself (or
// one shard of it): the table is the identity and each model's batch is the arena's n trees.
namespace {
constexpr int MATCH_MAX_MODELS = 16;

struct MatchParams {
    const char* who;                 // "arena" / "tournament": the error texts' prefix
    int K;
    NetModel* const* nets;           // [K]; the pairs are (i, j), i < j, in lexicographic order: i is the pair's "new" model, j its "old" one
    int n, half, first;              // games per pair played here; ArenaDev::half and ::first (a shard's offset; 0 for the tournament)
    int32_t num_sims, max_depth, cpuct;
    int T;
    uint64_t reserve, seed;
    const uint64_t* start_board;     // [2] play_games' `board` (src/arena.rs:62-67), the openings' base; nullptr = the initial board
    int record_evals;                // > 0 (K == 2 only): eval logs of the two models' trees, kept in e->ar_log
};

// {W, L, D} of a pair's first listed model over the pair's games [first, first + n): it holds the first seat below half (src/arena.rs:80-81)
void tally_wld(const int8_t* res, int n, int first, int half, uint64_t wld[3]) {
    wld[0] = wld[1] = wld[2] = 0;
    for (int g = 0; g < n; ++g) {
        const int win_cond = first + g < half ? 1 : -1;
        wld[res[g] == win_cond ? 0 : (res[g] == -win_cond ? 1 : 2)]++;
    }
}

// pair_wld [P][3] and results [P * n] (may be nullptr) are written, and the e->ar_* records replaced, only when the whole call succeeded
az_status match_run(az_engine* e, const MatchParams& m, uint64_t* pair_wld, int8_t* results) {
    const int K = m.K, n = m.n, P = K * (K - 1) / 2, PN = P * n, Gk = (K - 1) * n, T = m.T;
    NetModel* const* nets = m.nets;
    const std::string who = m.who;
    ScopedTimer timer{e};
    try {
        HIPCHK(hipSetDevice(e->device));
        hipStream_t s = e->stream;
        // one tree PAIR per game (B8 repair): the reference shares one nmcts / one pmcts across all games
        // (src/coach.rs:333-354) and their u16 root counters would wrap at 65536 visits.
        const int calls = AZ_MAX_PLIES / 2 + 1;
        const uint64_t nodes = std::min<uint64_t>(m.reserve, reachable_slots(m.num_sims, calls));
        const uint64_t blocks = reachable_blocks(m.num_sims, calls, nodes);
        if (az_status cs = check_tree_slots(e, blocks)) return cs;
        // The searches of a ply touch disjoint trees and (for different models) disjoint net workspaces, so they overlap: the models are dealt
        // round robin over the engine's stream and up to three side streams; two seats on one model or on one set of weights share a stream
        int stream_of[MATCH_MAX_MODELS], n_streams = 0;
        for (int k = 0; k < K; ++k) {
            stream_of[k] = -1;
            for (int j = 0; j < k; ++j)
                if (nets[k] == nets[j] || (nets[k]->conv && nets[k]->conv == nets[j]->conv)) { stream_of[k] = stream_of[j]; break; }
            if (stream_of[k] < 0) stream_of[k] = n_streams++ % 4;
        }
        n_streams = std::min(n_streams, 4);
        hipStream_t streams[4] = {s, nullptr, nullptr, nullptr};
        for (int i = 1; i < n_streams; ++i) {
            if (!e->side[i - 1]) HIPCHK(hipStreamCreate(&e->side[i - 1]));
            streams[i] = e->side[i - 1];
        }
        struct Events {
            hipEvent_t fork = nullptr, join[3] = {nullptr, nullptr, nullptr};
            ~Events() { if (fork) (void)hipEventDestroy(fork); for (hipEvent_t j : join) if (j) (void)hipEventDestroy(j); }
        } ev;
        if (n_streams > 1) {
            HIPCHK(hipEventCreateWithFlags(&ev.fork, hipEventDisableTiming));
            for (int i = 1; i < n_streams; ++i) HIPCHK(hipEventCreateWithFlags(&ev.join[i - 1], hipEventDisableTiming));
        }
        TreeLease lease[MATCH_MAX_MODELS];
        for (int k = 0; k < K; ++k) acquire_trees(e, lease[k], Gk, blocks, nodes, hash_entries(m.num_sims, calls), T, s);
        DeviceMem mem;
        ArenaDev ad{};
        ad.G = PN; ad.half = m.half; ad.first = m.first;
        ad.state = mem.alloc<ulonglong2>(PN);
        ad.player = mem.alloc<int8_t>(PN);
        ad.alive = mem.alloc<uint8_t>(PN);
        ad.results = mem.alloc<int8_t>(PN);
        ad.counters = mem.alloc<uint32_t>(2 + MATCH_MAX_MODELS);    // [2 + k]: the largest leaf batch of the ply of model k (tile / kernel choice of the next ply)
        ad.moves = mem.alloc<uint8_t>((size_t)PN * AZ_MAX_PLIES);
        ad.len = mem.alloc<int32_t>(PN);
        HIPCHK(hipMemset(ad.moves, 0, (size_t)PN * AZ_MAX_PLIES));
        HIPCHK(hipMemset(ad.len, 0, (size_t)PN * sizeof(int32_t)));
        // the tables: model k's trees are its pairs in the pairs' order, n games each
        MatchTable tb[MATCH_MAX_MODELS];
        {
            std::vector<uint32_t> h((size_t)K * Gk);
            std::vector<int> fill((size_t)K, 0);
            int pidx = 0;
            for (int i = 0; i < K; ++i)
                for (int j = i + 1; j < K; ++j, ++pidx)
                    for (int g = 0; g < n; ++g) {
                        h[(size_t)i * Gk + fill[i]++] = (uint32_t)(pidx * n + g);
                        h[(size_t)j * Gk + fill[j]++] = (uint32_t)(pidx * n + g) | 0x80000000u;
                    }
            uint32_t* d_tab = mem.alloc<uint32_t>(h.size());
            ulonglong2* d_roots = mem.alloc<ulonglong2>((size_t)K * Gk);
            HIPCHK(hipMemcpy(d_tab, h.data(), h.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
            HIPCHK(hipMemset(d_roots, 0, (size_t)K * Gk * sizeof(ulonglong2)));
            for (int k = 0; k < K; ++k) tb[k] = MatchTable{d_tab + (size_t)k * Gk, d_roots + (size_t)k * Gk, n, 0};
        }
        // paired openings: game g of a pair and its seat-swapped twin g + half start from the opening of pair g % half (csrc/az_opening.h)
        const bool openings = e->arena_opening_plies > 0 || !e->ar_book.empty();
        const ulonglong2 base = m.start_board ? make_ulonglong2(m.start_board[0], m.start_board[1]) : make_ulonglong2(0ull, 0ull);
        ArenaOpenings op{};
        std::vector<uint64_t> open_boards;                      // the positions the games start from, before the first ply changes ad.state
        if (openings) {
            // one lane per game draws its opening into ad.state and the opening record; every pair of models plays the same ones
            op.seed = m.seed;
            op.plies = (int32_t)e->arena_opening_plies;
            op.nb = (int32_t)(e->ar_book.size() / 2);
            if (op.nb) {
                ulonglong2* book = mem.alloc<ulonglong2>((size_t)op.nb);
                HIPCHK(hipMemcpy(book, e->ar_book.data(), e->ar_book.size() * 8, hipMemcpyHostToDevice));
                op.book = book;
            }
            op.base = base;
            op.len = mem.alloc<int32_t>(PN);
            op.moves = mem.alloc<uint8_t>((size_t)PN * OPENING_MAX_PLIES);
            for (int p = 0; p < P; ++p) {
                ArenaDev av = ad;
                av.G = n; av.state = ad.state + (size_t)p * n;
                ArenaOpenings ov = op;
                ov.len = op.len + (size_t)p * n; ov.moves = op.moves + (size_t)p * n * OPENING_MAX_PLIES;
                launch_arena_openings(e->cfg.game, av, ov, s);
            }
            open_boards.resize((size_t)PN * 2);
            HIPCHK(hipStreamSynchronize(s));
            HIPCHK(hipMemcpy(open_boards.data(), ad.state, open_boards.size() * 8, hipMemcpyDeviceToHost));
        } else {
            const std::vector<ulonglong2> st0((size_t)PN, base);
            HIPCHK(hipMemcpy(ad.state, st0.data(), st0.size() * sizeof(ulonglong2), hipMemcpyHostToDevice));
        }
        HIPCHK(hipMemset(ad.player, 1, PN));
        HIPCHK(hipMemset(ad.alive, 1, PN));
        HIPCHK(hipMemset(ad.results, 0, PN));
        uint32_t ctr[2 + MATCH_MAX_MODELS] = {(uint32_t)PN, 0u};
        HIPCHK(hipMemcpy(ad.counters, ctr, sizeof ctr, hipMemcpyHostToDevice));
        int typ[MATCH_MAX_MODELS] = {};              // expected rows per leaf batch, per model (0 = unknown: assume every running game)
        ScopedEvalLog logs[2];
        if (m.record_evals > 0)
            for (int k = 0; k < 2; ++k) logs[k].attach(*lease[k], (size_t)Gk, m.record_evals, nullptr);
        bool any_dedup = false;
        for (int k = 0; k < K; ++k) { launch_reset_trees(lease[k]->d, nullptr, s); any_dedup = any_dedup || dedup_applies(e, *nets[k]); }
        prepare_cache(e, any_dedup, (uint64_t)PN * AZ_MAX_PLIES * ((uint64_t)m.num_sims + 1), s);
        // all tags are fixed before the first fork (retagging may clear the cache).  Two passes: when the 15-bit counter wraps at one of
        // the models, the models tagged before it lose their tags again, and the second pass hands them new ones (K <= 16: no second wrap)
        for (int pass = 0; pass < 2; ++pass)
            for (int k = 0; k < K; ++k) (void)cache_for(e, *nets[k]);
        SearchParams sp{(uint32_t)m.max_depth, (float)m.cpuct};
        // the decided-move stop: every move of a match is played at temperature 0 (the only part of the root-move record a match arms)
        ScopedRootMove armed[MATCH_MAX_MODELS];
        if (e->search_stop)
            for (int k = 0; k < K; ++k) {
                RootMove mv{};
                mv.stop = stop_for(e, m.num_sims, INT32_MIN);
                armed[k].install(*lease[k], mv);
            }
        az_status result = AZ_OK;
        for (int ply = 0; ply <= AZ_MAX_PLIES; ++ply) {
            for (int k = 0; k < K; ++k) launch_match_sync(lease[k]->d, ad, tb[k], s);
            if (n_streams > 1) {
                HIPCHK(hipEventRecord(ev.fork, s));
                for (int i = 1; i < n_streams; ++i) HIPCHK(hipStreamWaitEvent(streams[i], ev.fork, 0));
            }
            // the side streams' models first, so that their searches are queued while the host issues the engine stream's
            for (int pass = 0; pass < 2; ++pass)
                for (int k = 0; k < K; ++k) {
                    if ((stream_of[k] == 0) != (pass == 1)) continue;
                    run_search(e, *lease[k], tb[k].roots, m.num_sims, sp, *nets[k], (int)std::min<uint32_t>(ctr[0], (uint32_t)Gk), streams[stream_of[k]],
                               typ[k], ad.counters + 2 + k);
                }
            for (int i = 1; i < n_streams; ++i) {
                HIPCHK(hipEventRecord(ev.join[i - 1], streams[i]));
                HIPCHK(hipStreamWaitEvent(s, ev.join[i - 1], 0));
            }
            for (int k = 0; k < K; ++k) launch_stop_count(lease[k]->d, nullptr, s);
            for (int k = 0; k < K; ++k) launch_match_move(lease[k]->d, ad, tb[k], m.seed, s);
            HIPCHK(hipMemcpyAsync(ctr, ad.counters, sizeof ctr, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            resolve_profile(e);
            for (int k = 0; k < K; ++k) typ[k] = (int)std::min<uint32_t>(ctr[2 + k], (uint32_t)(Gk * T));
            HIPCHK(hipMemsetAsync(ad.counters + 2, 0, MATCH_MAX_MODELS * sizeof(uint32_t), s));
            if (ctr[1]) { result = fail(e, AZ_ERR_INVALID_MOVE, who + ": action is not valid (src/arena.rs:31-35)"); break; }
            if (ctr[0] == 0) break;
        }
        for (int k = 0; k < K; ++k) harvest_stats(e, *lease[k], *nets[k]);
        for (int k = 0; k < K; ++k) if (result == AZ_OK) result = check_tree_errors(e, *lease[k]);
        if (result) return result;
        if (ctr[0] != 0) return fail(e, AZ_ERR_HIP, "az_" + who + ": games did not finish");
        // everything to host vectors first ...
        std::vector<int8_t> res((size_t)PN);
        HIPCHK(hipMemcpy(res.data(), ad.results, (size_t)PN, hipMemcpyDeviceToHost));
        std::vector<uint8_t> moves((size_t)PN * AZ_MAX_PLIES), open_moves;
        std::vector<int32_t> len((size_t)PN), open_len;
        HIPCHK(hipMemcpy(moves.data(), ad.moves, moves.size(), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(len.data(), ad.len, len.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        if (openings) {
            open_len.resize((size_t)PN);
            open_moves.resize((size_t)PN * OPENING_MAX_PLIES);
            HIPCHK(hipMemcpy(open_len.data(), op.len, open_len.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(open_moves.data(), op.moves, open_moves.size(), hipMemcpyDeviceToHost));
        }
        az_engine::EvalLog evals[2];
        if (m.record_evals > 0)
            for (int k = 0; k < 2; ++k) {
                std::vector<TreeLine> heads((size_t)Gk);
                HIPCHK(hipMemcpy(heads.data(), lease[k]->d.head, heads.size() * sizeof(TreeLine), hipMemcpyDeviceToHost));
                evals[k].count.resize((size_t)Gk);
                for (int g = 0; g < Gk; ++g) evals[k].count[g] = (int32_t)heads[g].head.log_len;
                logs[k].copy_out(evals[k].states, evals[k].pi, evals[k].v);
            }
        if (results) HIPCHK(hipMemcpy(results, res.data(), (size_t)PN, hipMemcpyDefault));
        // ... nothing can fail from here on: the outputs and the records of the last call change together
        for (int p = 0; p < P; ++p) tally_wld(res.data() + (size_t)p * n, n, m.first, m.half, pair_wld + 3 * (size_t)p);
        e->ar_moves = std::move(moves);
        e->ar_len = std::move(len);
        if (openings) {
            e->ar_open_boards = std::move(open_boards);
            e->ar_open_len = std::move(open_len);
            e->ar_open_moves = std::move(open_moves);
        } else {
            record_common_opening(e, PN, base.x, base.y);
        }
        e->ar_log_cap = 0;            // without record_evals there is no eval log: az_arena_get_evals is refused
        if (m.record_evals > 0) {
            for (int k = 0; k < 2; ++k) e->ar_log[k] = std::move(evals[k]);
            e->ar_log_cap = m.record_evals;
            e->ar_log_games = PN;
        }
        e->stats.games += (uint64_t)PN;
        return AZ_OK;
    } catch (const HipFail& f) { return fail_hip(e, f); }
}
}  // namespace

az_status az_arena(az_engine* e, const az_arena_params* p, uint64_t out_wld[3], int8_t* results) {
    if (!e || !p || !out_wld) return AZ_ERR_BAD_ARGUMENT;
    if (az_status sr = session_refusal(e, "az_arena")) return sr;
    if (p->num_games < 0 || p->num_sims <= 0 || p->max_depth < 0 || p->reserve < 8)
        return fail(e, AZ_ERR_BAD_ARGUMENT, "az_arena: bad argument");
    // unsharded: num/2 games per seating (src/arena.rs:83, an odd game is dropped); sharded: this rank's range of an
    // even global total, seated by global index
    const bool sharded = p->total_games > 0;
    if (sharded && (p->first_game < 0 || p->first_game + p->num_games > p->total_games))
        return fail(e, AZ_ERR_BAD_ARGUMENT, "az_arena: shard outside [0, total_games)");
    if (!sharded && p->first_game != 0) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_arena: first_game without total_games");
    const int half = sharded ? p->total_games / 2 : p->num_games / 2;
    const int G = sharded ? p->num_games : 2 * half;
    const int first = sharded ? p->first_game : 0;
    out_wld[0] = out_wld[1] = out_wld[2] = 0;
    // a host that asks for the whole arena's tally but never bound a communicator would gate the model on its own shard's count
    if (p->allreduce_wld && (!sharded || !e->has_comm()))
        return fail(e, AZ_ERR_BAD_ARGUMENT, "az_arena: allreduce_wld needs a sharded call (total_games > 0) on an engine with a communicator (az_comm_init)");
    if (G == 0) {      // an empty shard still takes part in the tally's all-reduce
        if (p->allreduce_wld) return az_allreduce_u64(e, out_wld, 3);
        return AZ_OK;
    }
    if (G > 1024 * 64) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_arena: at most 65536 games");
    if (p->record_evals < 0) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_arena: negative record_evals");
    if (p->use_start_board && !e->ar_book.empty())
        return fail(e, AZ_ERR_BAD_ARGUMENT, "az_arena: start_board while an opening book is set (az_arena_set_opening_book with n = 0 clears it)");
    if (p->use_start_board) {
        const uint64_t a = p->start_board[0], b = p->start_board[1];
        if ((a & b) || ((a | b) & ~C4_FULL)) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_arena: start_board is not a pair of disjoint 7x6 bitboards");
        // play_game's loop condition (src/arena.rs:18) fails at once on a finished board: result = cur_player * round(ended(cur_player)), :51
        const ulonglong2 s0 = make_ulonglong2(a, b);
        const uint32_t ec = e->cfg.game == 1 ? ConnectThree::ended_code(s0) : ConnectFour::ended_code(s0);
        if (ec != E_NONE) {
            const int8_t r = ec == E_MINUS1 ? 1 : (ec == E_PLUS1 ? -1 : 0);
            std::vector<int8_t> res((size_t)G, r);
            tally_wld(res.data(), G, first, half, out_wld);
            if (results && hipMemcpy(results, res.data(), (size_t)G, hipMemcpyDefault) != hipSuccess) return fail(e, AZ_ERR_HIP, "az_arena: results copy");
            e->stats.games += (uint64_t)G;
            e->ar_log_cap = 0;
            e->ar_moves.assign((size_t)G * AZ_MAX_PLIES, 0);      // no move is played on a finished board
            e->ar_len.assign((size_t)G, 0);
            record_common_opening(e, G, a, b);
            if (p->allreduce_wld) return az_allreduce_u64(e, out_wld, 3);     // the shards' tallies, as on the played path
            return AZ_OK;
        }
    }
    NetModel* nets[2];          // {new, old}
    az_status st = find_net(e, p->new_model_id, &nets[0]);
    if (st) return st;
    st = find_net(e, p->old_model_id, &nets[1]);
    if (st) return st;
    int T = p->num_sim_threads;
    st = check_threads(e, p->num_sims, &T);
    if (st) return st;
    st = stop_refusal(e, T, "az_arena", false);
    if (st) return st;
    st = check_batch(e, *nets[0], G * T);
    if (st) return st;
    st = check_batch(e, *nets[1], G * T);
    if (st) return st;
    const MatchParams m{"arena", 2, nets, G, half, first, p->num_sims, p->max_depth, p->cpuct, T, p->reserve, p->seed,
                        p->use_start_board ? p->start_board : nullptr, p->record_evals};
    st = match_run(e, m, out_wld, results);
    if (st) return st;
    if (p->allreduce_wld) return az_allreduce_u64(e, out_wld, 3);     // every rank returns the whole arena's tally (one 3-counter all-reduce)
    return AZ_OK;
}

az_status az_tournament(az_engine* e, const int32_t* model_ids, int32_t num_models, int32_t games_per_pair, int32_t num_sims, int32_t max_depth,
                        int32_t cpuct, int32_t num_sim_threads, uint64_t reserve, uint64_t seed, uint64_t* wld, int8_t* results) {
    if (!e) return AZ_ERR_BAD_ARGUMENT;
    if (!model_ids || !wld) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_tournament: model_ids and wld are required");
    const int K = num_models, n = games_per_pair;
    if (K < 2 || K > MATCH_MAX_MODELS) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_tournament: 2 .. 16 models");
    if (n < 2 || (n & 1)) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_tournament: games_per_pair must be even and at least 2 (half per seating)");
    if ((int64_t)(K * (K - 1) / 2) * (int64_t)n > 1024 * 64) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_tournament: at most 65536 games");
    if (num_sims <= 0 || max_depth < 0 || reserve < 8) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_tournament: bad argument");
    if (e->sp_session) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_tournament: a self-play session is open (az_selfplay_end first)");
    NetModel* nets[MATCH_MAX_MODELS];
    for (int k = 0; k < K; ++k) {
        for (int j = 0; j < k; ++j)
            if (model_ids[j] == model_ids[k]) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_tournament: model id " + std::to_string(model_ids[k]) + " is listed twice");
        if (find_net(e, model_ids[k], &nets[k])) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_tournament: model id " + std::to_string(model_ids[k]) + " is not initialised");
    }
    int T = num_sim_threads;
    if (az_status st = check_threads(e, num_sims, &T)) return st;
    if (az_status st = stop_refusal(e, T, "az_tournament", false)) return st;
    for (int k = 0; k < K; ++k)
        if (az_status st = check_batch(e, *nets[k], (K - 1) * n * T)) return st;
    const int P = K * (K - 1) / 2;
    std::vector<uint64_t> pair_wld((size_t)P * 3);
    const MatchParams m{"tournament", K, nets, n, n / 2, 0, num_sims, max_depth, cpuct, T, reserve, seed, nullptr, 0};
    const az_status st = match_run(e, m, pair_wld.data(), results);
    if (st == AZ_OK) {
        for (size_t i = 0; i < (size_t)K * K * 3; ++i) wld[i] = 0;
        const uint64_t* c = pair_wld.data();
        for (int i = 0; i < K; ++i)
            for (int j = i + 1; j < K; ++j, c += 3) {
                uint64_t *a = wld + ((size_t)i * K + j) * 3, *b = wld + ((size_t)j * K + i) * 3;
                a[0] = c[0]; a[1] = c[1]; a[2] = c[2];
                b[0] = c[1]; b[1] = c[0]; b[2] = c[2];
            }
    }
    // the pool keeps what it would keep after an az_arena: at most three idle tree arenas (the newest go first)
    try {
        for (size_t i = e->tree_pool.size(); i-- > 0 && e->tree_pool.size() > 3;)
            if (!e->tree_pool[i]->in_use) {
                HIPCHK(hipStreamSynchronize(e->stream));
                e->tree_pool.erase(e->tree_pool.begin() + (long)i);
            }
    } catch (const HipFail& f) { return fail_hip(e, f); }
    return st;
}

az_status az_rating_fit(const uint64_t* wld, int32_t K, double prior_games, double* elo, double* elo_se, int32_t* sweeps) {
    return rating_fit(wld, K, prior_games, elo, elo_se, sweeps) ? AZ_OK : AZ_ERR_BAD_ARGUMENT;
}

az_status az_arena_get_moves(az_engine* e, int32_t* game_len, uint8_t* moves) {
    if (!e || e->ar_len.empty()) return fail(e, AZ_ERR_BAD_ARGUMENT, "no move record (run az_arena first)");
    if (game_len) std::memcpy(game_len, e->ar_len.data(), e->ar_len.size() * sizeof(int32_t));
    if (moves) std::memcpy(moves, e->ar_moves.data(), e->ar_moves.size());
    return AZ_OK;
}

az_status az_arena_set_opening_book(az_engine* e, const uint64_t* boards, int32_t n) {
    if (!e) return AZ_ERR_BAD_ARGUMENT;
    if (n < 0 || n > OPENING_MAX_BOOK || (n > 0 && !boards)) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_arena_set_opening_book: 0 .. 65536 entries");
    for (int32_t i = 0; i < n; ++i) {
        const uint64_t a = boards[2 * (size_t)i], b = boards[2 * (size_t)i + 1];
        if ((a & b) || ((a | b) & ~C4_FULL))
            return fail(e, AZ_ERR_BAD_ARGUMENT, "az_arena_set_opening_book: entry " + std::to_string(i) + " is not a pair of disjoint 7x6 bitboards");
        const ulonglong2 s0 = make_ulonglong2(a, b);
        if ((e->cfg.game == 1 ? ConnectThree::ended_code(s0) : ConnectFour::ended_code(s0)) != E_NONE)
            return fail(e, AZ_ERR_BAD_ARGUMENT, "az_arena_set_opening_book: entry " + std::to_string(i) + " is a finished position");
    }
    e->ar_book.assign(boards, boards + 2 * (size_t)n);
    return AZ_OK;
}

az_status az_arena_get_openings(az_engine* e, uint64_t* boards, int32_t* len, uint8_t* moves) {
    if (!e || e->ar_open_len.empty()) return fail(e, AZ_ERR_BAD_ARGUMENT, "no opening record (run az_arena first)");
    if (boards) std::memcpy(boards, e->ar_open_boards.data(), e->ar_open_boards.size() * 8);
    if (len) std::memcpy(len, e->ar_open_len.data(), e->ar_open_len.size() * sizeof(int32_t));
    if (moves) std::memcpy(moves, e->ar_open_moves.data(), e->ar_open_moves.size());
    return AZ_OK;
}

az_status az_arena_get_evals(az_engine* e, int32_t which, int32_t* rec_count, uint64_t* states, float* pis, float* vs) {
    if (!e || which < 0 || which > 1 || e->ar_log_cap <= 0) return fail(e, AZ_ERR_BAD_ARGUMENT, "no eval log (run az_arena with record_evals > 0)");
    const az_engine::EvalLog& l = e->ar_log[which];
    if (rec_count) std::memcpy(rec_count, l.count.data(), l.count.size() * sizeof(int32_t));
    if (states) std::memcpy(states, l.states.data(), l.states.size() * 8);
    if (pis) std::memcpy(pis, l.pi.data(), l.pi.size() * 4);
    if (vs) std::memcpy(vs, l.v.data(), l.v.size() * 4);
    return AZ_OK;
}

// ---- position averaging: one tuple per distinct position (csrc/az_merge.h) ---------------------------------------
az_status az_samples_merge(az_engine* e, const az_samples* src, int32_t flags, az_samples* dst, uint32_t* counts) {
    if (!e) return AZ_ERR_BAD_ARGUMENT;
    if (!src || !dst) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_samples_merge: src and dst are required");
    if (e->sp_session) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_samples_merge: a self-play session is open");
    if (flags & ~AZ_MERGE_CANONICAL) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_samples_merge: unknown flag bits");
    const long long n = src->count;
    if (n < 0 || n > MERGE_MAX_TUPLES) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_samples_merge: 0 .. 2^24 tuples");
    if (!dst->pis || !dst->zs) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_samples_merge: dst needs pis and zs");
    if (dst->capacity < n) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_samples_merge: dst->capacity is below src->count");
    if (const char* why = samples_shape_error(src, true)) return fail(e, AZ_ERR_BAD_ARGUMENT, std::string("az_samples_merge: src needs ") + why);
    {   // no dst array may overlap a src array: the inputs are read after the first outputs could have been written
        const size_t N = (size_t)n, C = (size_t)dst->capacity;
        const SampleSpan in[4] = {{src->states, N * 16}, {src->boards, N * AZ_FEATURES * 4}, {src->pis, N * AZ_ACTIONS * 4}, {src->zs, N * 4}};
        const SampleSpan out[5] = {{dst->states, C * 16}, {dst->boards, C * AZ_FEATURES * 4}, {dst->pis, C * AZ_ACTIONS * 4}, {dst->zs, C * 4}, {counts, C * 4}};
        if (sample_arrays_overlap(in, out)) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_samples_merge: a dst array overlaps a src array");
    }
    if (n == 0) { dst->count = 0; return AZ_OK; }
    ScopedTimer timer{e};
    try {
        HIPCHK(hipSetDevice(e->device));
        hipStream_t s = e->stream;
        const size_t N = (size_t)n;
        const bool from_boards = !src->states;
        const uint32_t T = std::max<uint32_t>(next_pow2_u32(2 * (uint64_t)N), 64u);
        const size_t nb = (N + 255) / 256;
        // one allocation, carved: [hdr] [inputs] [per tuple] [table] [per group] [outputs]
        Carve c;
        const size_t o_hdr = c.need(256), o_in_st = c.need(from_boards ? N * AZ_FEATURES * 4 : N * 16), o_in_pi = c.need(N * 28), o_in_z = c.need(N * 4),
                     o_cst = c.need(N * 16), o_slot = c.need(N * 4), o_tkey = c.need((size_t)T * 8), o_tmin = c.need((size_t)T * 4),
                     o_trank = c.need((size_t)T * 4), o_bsum = c.need(nb * 4), o_first = c.need(N * 4), o_sums = c.need(N * 64), o_cnt = c.need(N * 4),
                     o_out_st = c.need(N * 16), o_out_pi = c.need(N * 28), o_out_z = c.need(N * 4), o_out_b = c.need(dst->boards ? N * AZ_FEATURES * 4 : 0);
        char* base = (char*)e->merge_scratch.fit(c.total, s);      // one huge call does not pin its gigabytes
        MergeBufs b{};
        b.n = (uint32_t)N;
        b.in = stage_window(base + o_in_st, base + o_in_pi, base + o_in_z, src, s);
        b.cst = (ulonglong2*)(base + o_cst);
        b.slot = (uint32_t*)(base + o_slot);
        b.tkey = (unsigned long long*)(base + o_tkey);
        b.tmin = (uint32_t*)(base + o_tmin);
        b.trank = (uint32_t*)(base + o_trank);
        b.tmask = T - 1u;
        b.bsum = (uint32_t*)(base + o_bsum);
        b.first = (uint32_t*)(base + o_first);
        b.sums = (unsigned long long*)(base + o_sums);
        b.cnt = (uint32_t*)(base + o_cnt);
        b.hdr = (uint32_t*)(base + o_hdr);
        b.o_states = (ulonglong2*)(base + o_out_st);
        b.o_boards = dst->boards ? (float*)(base + o_out_b) : nullptr;
        b.o_pis = (float*)(base + o_out_pi);
        b.o_zs = (float*)(base + o_out_z);
        HIPCHK(hipMemsetAsync(b.hdr, 0, 256, s));
        HIPCHK(hipMemsetAsync(b.tkey, 0, (size_t)T * 8, s));
        HIPCHK(hipMemsetAsync(b.tmin, 0xFF, (size_t)T * 4, s));
        // 1. keys: every refusal that depends on the data is found here, before anything is written for the caller
        launch_merge_keys(e->cfg.game, b, (flags & AZ_MERGE_CANONICAL) ? 1 : 0, s);
        if (const char* why = sample_bad_text(read_verdict(b.hdr, s), false)) return fail(e, AZ_ERR_BAD_ARGUMENT, std::string("az_samples_merge: ") + why);
        // 2. output ranks in order of first occurrence; m groups
        launch_merge_scan(b, s);
        const size_t m = read_verdict(b.hdr + 1, s);
        if (m == 0 || m > N) return fail(e, AZ_ERR_HIP, "az_samples_merge: the scan returned an impossible group count");
        // 3. integer sums per group, 4. means or verbatim copies
        HIPCHK(hipMemsetAsync(b.sums, 0, m * 64, s));
        HIPCHK(hipMemsetAsync(b.cnt, 0, m * 4, s));
        launch_merge_accumulate(b, s);
        launch_merge_finalise(e->cfg.game, b, (uint32_t)m, s);
        if (dst->states) HIPCHK(hipMemcpyAsync(dst->states, b.o_states, m * 16, hipMemcpyDefault, s));
        if (dst->boards) HIPCHK(hipMemcpyAsync(dst->boards, b.o_boards, m * AZ_FEATURES * 4, hipMemcpyDefault, s));
        HIPCHK(hipMemcpyAsync(dst->pis, b.o_pis, m * 28, hipMemcpyDefault, s));
        HIPCHK(hipMemcpyAsync(dst->zs, b.o_zs, m * 4, hipMemcpyDefault, s));
        if (counts) HIPCHK(hipMemcpyAsync(counts, b.cnt, m * 4, hipMemcpyDefault, s));
        HIPCHK(hipStreamSynchronize(s));
        dst->count = (int64_t)m;
        return AZ_OK;
    } catch (const HipFail& f) { return fail_hip(e, f); }
}

// ---- search statistics as training targets: z/q blend and surprise resampling (csrc/az_target.h) -----------------------
az_status az_samples_blend_z(az_engine* e, int64_t n, const float* zs, const float* root_q, int64_t lambda_e6, float* zs_out) {
    if (!e) return AZ_ERR_BAD_ARGUMENT;
    if (e->sp_session) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_samples_blend_z: a self-play session is open");
    if (e->train_open) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_samples_blend_z: a training session is open");
    if (n < 0 || n > DRAW_MAX_TUPLES) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_samples_blend_z: 0 .. 2^31 - 1 values");
    if (lambda_e6 < 0 || lambda_e6 > TARGET_E6) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_samples_blend_z: lambda_e6 must be in 0 .. 1000000");
    if (n == 0) return AZ_OK;
    if (!zs || !root_q || !zs_out) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_samples_blend_z: zs, root_q and zs_out are required");
    ScopedTimer timer{e};
    try {
        HIPCHK(hipSetDevice(e->device));
        hipStream_t s = e->stream;
        const size_t N = (size_t)n;
        Carve c;
        const size_t o_hdr = c.need(256), o_z = c.need(N * 4), o_r = c.need(N * 4), o_o = c.need(N * 4);
        char* base = (char*)e->target_scratch.fit(c.total, s);
        uint32_t* d_bad = (uint32_t*)(base + o_hdr);
        float *d_z = (float*)(base + o_z), *d_r = (float*)(base + o_r), *d_o = (float*)(base + o_o);
        HIPCHK(hipMemsetAsync(d_bad, 0, 256, s));
        HIPCHK(hipMemcpyAsync(d_z, zs, N * 4, hipMemcpyDefault, s));
        HIPCHK(hipMemcpyAsync(d_r, root_q, N * 4, hipMemcpyDefault, s));
        launch_target_blend(d_z, d_r, n, lambda_e6, d_o, d_bad, s);
        if (read_verdict(d_bad, s)) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_samples_blend_z: a z or a root_q that is NaN or outside [-1, 1]");
        HIPCHK(hipMemcpyAsync(zs_out, d_o, N * 4, hipMemcpyDefault, s));
        HIPCHK(hipStreamSynchronize(s));
        return AZ_OK;
    } catch (const HipFail& f) { return fail_hip(e, f); }
}

az_status az_samples_surprise(az_engine* e, const az_samples* src, const float* priors, int64_t share_e6, uint64_t seed, az_samples* dst,
                              uint32_t* counts, float* kl) {
    if (!e) return AZ_ERR_BAD_ARGUMENT;
    if (!src) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_samples_surprise: src is required");
    if (e->sp_session) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_samples_surprise: a self-play session is open");
    if (e->train_open) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_samples_surprise: a training session is open");
    if (share_e6 < 0 || share_e6 > TARGET_E6) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_samples_surprise: share_e6 must be in 0 .. 1000000");
    const long long n = src->count;
    if (n < 0 || n > TARGET_MAX_TUPLES) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_samples_surprise: 0 .. 2^24 tuples");
    if (n > 0 && (!priors || samples_shape_error(src, false)))
        return fail(e, AZ_ERR_BAD_ARGUMENT, "az_samples_surprise: needs priors and src's pis, zs and states or boards");
    if (dst) {
        if (!dst->pis || !dst->zs) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_samples_surprise: dst needs pis and zs");
        if (dst->capacity < 2 * n) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_samples_surprise: dst->capacity is below 2 * src->count");
        if (n > 0 && ((dst->states && !src->states) || (dst->boards && !src->boards)))
            return fail(e, AZ_ERR_BAD_ARGUMENT, "az_samples_surprise: dst asks for an array (states / boards) that src does not have");
        // no dst array may overlap a src array, as in az_samples_merge
        const size_t N = (size_t)n, C = (size_t)dst->capacity;
        const SampleSpan in[5] = {{src->states, N * 16}, {src->boards, N * AZ_FEATURES * 4}, {src->pis, N * AZ_ACTIONS * 4}, {src->zs, N * 4},
                                  {priors, N * AZ_ACTIONS * 4}};
        const SampleSpan out[4] = {{dst->states, C * 16}, {dst->boards, C * AZ_FEATURES * 4}, {dst->pis, C * AZ_ACTIONS * 4}, {dst->zs, C * 4}};
        if (sample_arrays_overlap(in, out)) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_samples_surprise: a dst array overlaps a src array");
    }
    if (n == 0) { if (dst) dst->count = 0; return AZ_OK; }
    ScopedTimer timer{e};
    try {
        HIPCHK(hipSetDevice(e->device));
        hipStream_t s = e->stream;
        const size_t N = (size_t)n, M = 2 * N;
        const bool st = src->states != nullptr, bd = src->boards != nullptr;
        const bool o_st = dst && dst->states, o_bd = dst && dst->boards;
        const size_t nb = draw_scan_blocks(n);
        Carve c;
        // [hdr: bad, SK, W] [inputs] [per tuple] [outputs, 2n rows]
        const size_t o_hdr = c.need(256), o_in_st = c.need(st ? N * 16 : 0), o_in_b = c.need(bd ? N * AZ_FEATURES * 4 : 0), o_in_pi = c.need(N * 28),
                     o_in_z = c.need(N * 4), o_in_pr = c.need(N * 28), o_kl = c.need(N * 4), o_K = c.need(N * 8), o_cnt = c.need(N * 4), o_Q = c.need(N * 8),
                     o_bsum = c.need(nb * 8), o_idx = c.need(dst ? M * 4 : 0), o_out_st = c.need(o_st ? M * 16 : 0),
                     o_out_b = c.need(o_bd ? M * AZ_FEATURES * 4 : 0), o_out_pi = c.need(dst ? M * 28 : 0), o_out_z = c.need(dst ? M * 4 : 0);
        char* base = (char*)e->target_scratch.fit(c.total, s);
        uint32_t* d_bad = (uint32_t*)(base + o_hdr);
        uint64_t *d_SK = (uint64_t*)(base + o_hdr + 8), *d_W = (uint64_t*)(base + o_hdr + 16);
        const float *d_b = bd ? (const float*)(base + o_in_b) : nullptr, *d_pr = (const float*)(base + o_in_pr);
        float* d_kl = (float*)(base + o_kl);
        uint64_t *d_K = (uint64_t*)(base + o_K), *d_Q = (uint64_t*)(base + o_Q), *d_bsum = (uint64_t*)(base + o_bsum);
        uint32_t* d_cnt = (uint32_t*)(base + o_cnt);
        HIPCHK(hipMemsetAsync(base + o_hdr, 0, 256, s));
        const SampleWindow in = stage_window(base + (st ? o_in_st : o_in_b), base + o_in_pi, base + o_in_z, src, s);
        if (st && bd) HIPCHK(hipMemcpyAsync(base + o_in_b, src->boards, N * AZ_FEATURES * 4, hipMemcpyDefault, s));      // the gather copies both
        HIPCHK(hipMemcpyAsync(base + o_in_pr, priors, N * 28, hipMemcpyDefault, s));
        // 1. KL, K and their integer sum; every refusal that depends on the data is found here, before anything is written for the caller
        launch_target_kl(in, d_pr, n, d_kl, d_K, d_SK, d_bad, s);
        if (const char* why = sample_bad_text(read_verdict(d_bad, s), false)) return fail(e, AZ_ERR_BAD_ARGUMENT, std::string("az_samples_surprise: ") + why);
        // 2. copies, 3. their inclusive prefix
        launch_target_copies(d_K, d_SK, n, share_e6, seed, d_cnt, s);
        launch_draw_scan(d_cnt, n, d_Q, d_bsum, d_W, s);
        uint64_t W = 0;
        HIPCHK(hipMemcpyAsync(&W, d_W, sizeof W, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (dst) {
            if (W > (uint64_t)M) return fail(e, AZ_ERR_HIP, "az_samples_surprise: the scan returned an impossible row count");
            // 4. the gather
            launch_target_gather(d_Q, n, (int64_t)W, (uint32_t*)(base + o_idx), in.states, d_b, in.pis, in.zs, o_st ? (ulonglong2*)(base + o_out_st) : nullptr,
                                 o_bd ? (float*)(base + o_out_b) : nullptr, (float*)(base + o_out_pi), (float*)(base + o_out_z), s);
            if (W) {
                if (o_st) HIPCHK(hipMemcpyAsync(dst->states, base + o_out_st, (size_t)W * 16, hipMemcpyDefault, s));
                if (o_bd) HIPCHK(hipMemcpyAsync(dst->boards, base + o_out_b, (size_t)W * AZ_FEATURES * 4, hipMemcpyDefault, s));
                HIPCHK(hipMemcpyAsync(dst->pis, base + o_out_pi, (size_t)W * 28, hipMemcpyDefault, s));
                HIPCHK(hipMemcpyAsync(dst->zs, base + o_out_z, (size_t)W * 4, hipMemcpyDefault, s));
            }
        }
        if (counts) HIPCHK(hipMemcpyAsync(counts, d_cnt, N * 4, hipMemcpyDefault, s));
        if (kl) HIPCHK(hipMemcpyAsync(kl, d_kl, N * 4, hipMemcpyDefault, s));
        HIPCHK(hipStreamSynchronize(s));
        if (dst) dst->count = (int64_t)W;
        return AZ_OK;
    } catch (const HipFail& f) { return fail_hip(e, f); }
}

// ---- exact endgame solver and move-quality report (csrc/az_solve.h) ------------------------------------------------
}  // extern "C"

namespace {

constexpr size_t SOLVE_TABLE_BUDGET = (size_t)4 << 30;       // bytes of table at most: the lanes are cut to fit (tt_log2 = 16: 8192 lanes)

const char* solve_param_error(int32_t n, uint32_t max_nodes, int32_t min_stones, int32_t tt_log2, int32_t max_lanes) {
    if (n < 0 || n > (1 << 24)) return "0 .. 2^24 positions";
    if (max_nodes < 1u || max_nodes > (1u << 30)) return "max_nodes must be in 1 .. 2^30";
    if (min_stones < 0 || min_stones > AZ_MAX_PLIES) return "min_stones must be in 0 .. 42";
    if (tt_log2 != 0 && (tt_log2 < 8 || tt_log2 > 16)) return "tt_log2 must be 0 or 8 .. 16";
    if (max_lanes < 0 || max_lanes % 64 != 0) return "max_lanes must be 0 or a multiple of 64";
    return nullptr;
}

// The search over b.n positions already on the device (states, active, mv, nodes, values set by the caller): sizes the grid, readies the
// table, launches.
void solve_on_device(az_engine* e, SolveBufs b, int32_t max_lanes) {
    hipStream_t s = e->stream;
    if (e->solve_device_lanes == 0) e->solve_device_lanes = solve_device_lanes(e->cfg.game);
    if (e->solve_device_lanes <= 0) throw HipFail{hipErrorUnknown, "solve_device_lanes"};
    const size_t items = (size_t)b.n * AZ_ACTIONS;
    size_t lanes = (size_t)e->solve_device_lanes;
    if (max_lanes > 0) lanes = std::min(lanes, (size_t)max_lanes);
    lanes = std::min(lanes, (items + 63) / 64 * 64);
    if (b.tt_log2) lanes = std::min(lanes, std::max<size_t>(64, (SOLVE_TABLE_BUDGET >> (b.tt_log2 + 3)) / 64 * 64));
    // fixed places: the counters have room for every lane the device can hold, so a slice never moves with the call's lane count
    const size_t off_gens = 256, off_tt = off_gens + ((size_t)e->solve_device_lanes * 4 + 255) / 256 * 256;
    const size_t total = off_tt + (b.tt_log2 ? (lanes * 8) << b.tt_log2 : 0);
    char* base = (char*)e->solve_table.fit(total, s);
    if (e->solve_table.serial != e->solve_table_serial || (int)b.tt_log2 != e->solve_table_log2 || lanes > e->solve_table_lanes) {
        HIPCHK(hipMemsetAsync(base, 0, total, s));         // a new allocation, another slice size, or lanes that have no counter yet
        e->solve_table_serial = e->solve_table.serial;
        e->solve_table_log2 = (int)b.tt_log2;
        e->solve_table_lanes = (uint32_t)lanes;
    } else {
        HIPCHK(hipMemsetAsync(base, 0, 256, s));          // the item counter
    }
    b.counter = (uint32_t*)base;
    b.gens = (uint32_t*)(base + off_gens);
    b.tt = (unsigned long long*)(base + off_tt);
    launch_solve(e->cfg.game, b, (uint32_t)lanes, s);
    HIPCHK(hipGetLastError());
}

}  // namespace

extern "C" {

az_status az_solve(az_engine* e, const uint64_t* states, int32_t n, uint32_t max_nodes, int32_t min_stones, int32_t tt_log2, int32_t max_lanes,
                   int8_t* move_values, int8_t* values, uint32_t* nodes) {
    if (!e) return AZ_ERR_BAD_ARGUMENT;
    if (!states || !move_values) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_solve: states and move_values are required");
    if (e->sp_session) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_solve: a self-play session is open");
    if (const char* why = solve_param_error(n, max_nodes, min_stones, tt_log2, max_lanes)) return fail(e, AZ_ERR_BAD_ARGUMENT, (std::string("az_solve: ") + why).c_str());
    if (n == 0) return AZ_OK;
    ScopedTimer timer{e};
    try {
        HIPCHK(hipSetDevice(e->device));
        hipStream_t s = e->stream;
        const size_t N = (size_t)n;
        Carve c;
        const size_t o_hdr = c.need(256), o_st = c.need(N * 16), o_mv = c.need(N * 7), o_val = c.need(N), o_nodes = c.need(N * 28);
        char* base = (char*)e->solve_io.fit(c.total, s);
        HIPCHK(hipMemcpyAsync(base + o_st, states, N * 16, hipMemcpyDefault, s));
        HIPCHK(hipMemsetAsync(base + o_hdr, 0, 256, s));
        launch_solve_validate((const ulonglong2*)(base + o_st), (uint32_t)N, (uint32_t*)(base + o_hdr), s);
        HIPCHK(hipGetLastError());
        uint32_t verdict = 0;
        HIPCHK(hipMemcpyAsync(&verdict, base + o_hdr, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (verdict) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_solve: a state with overlapping stones, bits outside the 7x6 board or floating stones");
        SolveBufs b{};
        b.states = (const ulonglong2*)(base + o_st);
        b.n = (uint32_t)N;
        b.max_nodes = max_nodes;
        b.min_stones = min_stones;
        b.tt_log2 = (uint32_t)tt_log2;
        b.mv = (int8_t*)(base + o_mv);
        b.values = (int8_t*)(base + o_val);
        b.nodes = (uint32_t*)(base + o_nodes);
        solve_on_device(e, b, max_lanes);
        HIPCHK(hipMemcpyAsync(move_values, b.mv, N * 7, hipMemcpyDefault, s));
        if (values) HIPCHK(hipMemcpyAsync(values, b.values, N, hipMemcpyDefault, s));
        if (nodes) HIPCHK(hipMemcpyAsync(nodes, b.nodes, N * 28, hipMemcpyDefault, s));
        HIPCHK(hipStreamSynchronize(s));
        return AZ_OK;
    } catch (const HipFail& f) { return fail_hip(e, f); }
}

az_status az_move_quality(az_engine* e, const uint64_t* start_boards, const int32_t* game_len, const uint8_t* moves, int32_t n, uint32_t max_nodes,
                          int32_t min_stones, int32_t tt_log2, int32_t max_lanes, uint8_t* ply_class, int8_t* ply_value) {
    if (!e) return AZ_ERR_BAD_ARGUMENT;
    if (!game_len || !moves || !ply_class) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_move_quality: game_len, moves and ply_class are required");
    if (e->sp_session) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_move_quality: a self-play session is open");
    if (n > (1 << 24) / AZ_MAX_PLIES) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_move_quality: at most 2^24 / 42 games");
    if (const char* why = solve_param_error(n, max_nodes, min_stones, tt_log2, max_lanes)) return fail(e, AZ_ERR_BAD_ARGUMENT, (std::string("az_move_quality: ") + why).c_str());
    if (n == 0) return AZ_OK;
    ScopedTimer timer{e};
    try {
        HIPCHK(hipSetDevice(e->device));
        hipStream_t s = e->stream;
        const size_t N = (size_t)n, P = N * AZ_MAX_PLIES;
        Carve c;
        const size_t o_hdr = c.need(256), o_start = c.need(N * 16), o_len = c.need(N * 4), o_moves = c.need(P), o_st = c.need(P * 16), o_act = c.need(P),
                     o_mv = c.need(P * 7), o_val = c.need(P), o_nodes = c.need(P * 28), o_cls = c.need(P), o_pv = c.need(P);
        char* base = (char*)e->solve_io.fit(c.total, s);
        if (start_boards) HIPCHK(hipMemcpyAsync(base + o_start, start_boards, N * 16, hipMemcpyDefault, s));
        HIPCHK(hipMemcpyAsync(base + o_len, game_len, N * 4, hipMemcpyDefault, s));
        HIPCHK(hipMemcpyAsync(base + o_moves, moves, P, hipMemcpyDefault, s));
        HIPCHK(hipMemsetAsync(base + o_hdr, 0, 256, s));
        MoveQualityBufs q{};
        q.start = start_boards ? (const ulonglong2*)(base + o_start) : nullptr;
        q.game_len = (const int32_t*)(base + o_len);
        q.moves = (const uint8_t*)(base + o_moves);
        q.n = (uint32_t)N;
        q.min_stones = min_stones;
        q.states = (ulonglong2*)(base + o_st);
        q.active = (uint8_t*)(base + o_act);
        q.verdict = (uint32_t*)(base + o_hdr);
        q.mv = (const int8_t*)(base + o_mv);
        q.ply_class = (uint8_t*)(base + o_cls);
        q.ply_value = (int8_t*)(base + o_pv);
        launch_move_quality_replay(e->cfg.game, q, s);
        HIPCHK(hipGetLastError());
        uint32_t verdict = 0;
        HIPCHK(hipMemcpyAsync(&verdict, q.verdict, 4, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (verdict & SOLVE_BAD_STATE) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_move_quality: a start board with overlapping stones, bits outside the 7x6 board or floating stones");
        if (verdict & SOLVE_BAD_RECORD) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_move_quality: an illegal move in a record, or a game_len beyond the end of its game");
        SolveBufs b{};
        b.states = q.states;
        b.active = q.active;
        b.n = (uint32_t)P;
        b.max_nodes = max_nodes;
        b.min_stones = min_stones;
        b.tt_log2 = (uint32_t)tt_log2;
        b.mv = (int8_t*)(base + o_mv);
        b.values = (int8_t*)(base + o_val);
        b.nodes = (uint32_t*)(base + o_nodes);
        solve_on_device(e, b, max_lanes);
        launch_move_quality_classify(e->cfg.game, q, s);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(ply_class, q.ply_class, P, hipMemcpyDefault, s));
        if (ply_value) HIPCHK(hipMemcpyAsync(ply_value, q.ply_value, P, hipMemcpyDefault, s));
        HIPCHK(hipStreamSynchronize(s));
        return AZ_OK;
    } catch (const HipFail& f) { return fail_hip(e, f); }
}

// ---- the collective of the sharded Coach loop ---------------------------------------------------------------------------------
// Two backends, chosen by the id alone: RCCL (az_comm_unique_id) or an in-process group (az_comm_local_id, csrc/az_local_comm.h).
// The collectives below are shared code -- argument checks, the hello verdict, packing, offsets, unpacking -- on top of the only
// three things that differ: comm_allgather_hello, comm_sum_u64 and comm_exchange.
#define NCCLCHK(expr) do { ncclResult_t _r = (expr); if (_r != ncclSuccess) return fail(e, AZ_ERR_HIP, std::string("RCCL: ") + g_rccl.GetErrorString(_r) + " at " #expr); } while (0)

az_status az_comm_unique_id(az_engine* e, uint8_t id[AZ_COMM_ID_BYTES]) {
    if (!e || !id) return AZ_ERR_BAD_ARGUMENT;
    static_assert(sizeof(ncclUniqueId) == AZ_COMM_ID_BYTES, "ncclUniqueId is 128 bytes");
    std::string why;
    if (!g_rccl.load(&why)) return fail(e, AZ_ERR_UNSUPPORTED, why);
    ncclUniqueId u;
    NCCLCHK(g_rccl.GetUniqueId(&u));
    std::memcpy(id, &u, sizeof u);
    return AZ_OK;
}

az_status az_comm_local_id(az_engine* e, int32_t world, uint8_t id[AZ_COMM_ID_BYTES]) {
    if (!e || !id) return AZ_ERR_BAD_ARGUMENT;
    static_assert(LOCAL_ID_BYTES == AZ_COMM_ID_BYTES, "one id size for both backends");
    const std::string why = g_local_comms.create(world, id);
    return why.empty() ? AZ_OK : fail(e, AZ_ERR_BAD_ARGUMENT, why);
}

// an in-process id: join the group (returns once every rank has joined), then enable peer access towards the other members'
// devices where the hardware allows it ("already enabled" by another engine of the process is fine)
static az_status comm_init_local(az_engine* e, int32_t rank, int32_t world, const LocalId& lid) {
    try { HIPCHK(hipSetDevice(e->device)); } catch (const HipFail& f) { return fail_hip(e, f); }
    std::shared_ptr<LocalGroup> g;
    const std::string why = g_local_comms.join(lid, rank, world, e->device, &g);
    if (!why.empty()) return fail(e, AZ_ERR_BAD_ARGUMENT, why);
    std::vector<int> devs = g->devices();
    std::sort(devs.begin(), devs.end());
    devs.erase(std::unique(devs.begin(), devs.end()), devs.end());
    for (int d : devs) {
        int can = 0;
        if (d == e->device || hipDeviceCanAccessPeer(&can, e->device, d) != hipSuccess || !can) continue;
        // anything but success / already enabled leaves the copies to the runtime's staged path: still correct, so not an error
        (void)hipDeviceEnablePeerAccess(d, 0);
        (void)hipGetLastError();
    }
    e->local = std::move(g);
    e->comm_rank = rank;
    e->comm_world = world;
    return AZ_OK;
}

az_status az_comm_init(az_engine* e, int32_t rank, int32_t world, const uint8_t id[AZ_COMM_ID_BYTES]) {
    if (!e || !id || world < 1 || rank < 0 || rank >= world) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_comm_init: bad rank / world");
    if (e->has_comm()) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_comm_init: the engine already has a communicator (az_comm_destroy first)");
    LocalId lid;
    if (local_id_decode(id, &lid)) return comm_init_local(e, rank, world, lid);
    std::string why;
    if (!g_rccl.load(&why)) return fail(e, AZ_ERR_UNSUPPORTED, why);
    try { HIPCHK(hipSetDevice(e->device)); } catch (const HipFail& f) { return fail_hip(e, f); }
    ncclUniqueId u;
    std::memcpy(&u, id, sizeof u);
    NCCLCHK(g_rccl.CommInitRank(&e->comm, world, u, rank));
    e->comm_rank = rank;
    e->comm_world = world;
    return AZ_OK;
}

az_status az_comm_destroy(az_engine* e) {
    if (!e) return AZ_ERR_BAD_ARGUMENT;
    if (e->local) {          // every copy of a collective was synchronised before it returned: nothing of this engine is in flight
        e->local->leave(e->comm_rank);
        e->local.reset();
        e->comm_rank = 0; e->comm_world = 1;
    }
    if (e->comm) {
        (void)hipSetDevice(e->device);
        (void)hipStreamSynchronize(e->stream);
        NCCLCHK(g_rccl.CommDestroy(e->comm));
        e->comm = nullptr;
        e->comm_rank = 0; e->comm_world = 1;
    }
    return AZ_OK;
}

// primitive 2: in-place sum of n u64 counters over the ranks.  In-process: one round of [ok, 64 values] records summed in rank order
// (wrapping, as RCCL's ncclUint64 sum); a rank with bad arguments still takes part, so every rank returns the same error.
static az_status comm_sum_u64(az_engine* e, uint64_t* values, int32_t n, bool args_ok) {
    if (e->local) {
        uint64_t rec[1 + 64] = {args_ok ? 1ull : 0ull};
        if (args_ok && n > 0) std::memcpy(rec + 1, values, (size_t)n * 8);
        std::vector<unsigned char> all;
        const std::string err = e->local->all_gather(e->comm_rank, LOCAL_OP_ALLREDUCE, n, rec, sizeof rec, &all);
        if (!err.empty()) return fail(e, AZ_ERR_BAD_ARGUMENT, err);
        std::vector<uint64_t> q((size_t)e->comm_world * (1 + 64));
        std::memcpy(q.data(), all.data(), q.size() * 8);
        for (int r = 0; r < e->comm_world; ++r)
            if (!q[(size_t)r * 65]) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_allreduce_u64: bad argument on rank " + std::to_string(r) + " (values NULL or n outside 0..64)");
        uint64_t sum[64] = {};
        for (int r = 0; r < e->comm_world; ++r)
            for (int i = 0; i < n; ++i) sum[i] += q[(size_t)r * 65 + 1 + (size_t)i];
        if (n > 0) std::memcpy(values, sum, (size_t)n * 8);
        return AZ_OK;
    }
    try {
        HIPCHK(hipSetDevice(e->device));
        unsigned long long* d = (unsigned long long*)e->comm_scratch.ensure((size_t)n * 8, e->stream);
        HIPCHK(hipMemcpyAsync(d, values, (size_t)n * 8, hipMemcpyHostToDevice, e->stream));
        NCCLCHK(g_rccl.AllReduce(d, d, (size_t)n, ncclUint64, ncclSum, e->comm, e->stream));
        HIPCHK(hipMemcpyAsync(values, d, (size_t)n * 8, hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        return AZ_OK;
    } catch (const HipFail& f) { return fail_hip(e, f); }
}

az_status az_allreduce_u64(az_engine* e, uint64_t* values, int32_t n) {
    if (!e) return AZ_ERR_BAD_ARGUMENT;
    const bool args_ok = values && n >= 0 && n <= 64;
    if (!e->local && !args_ok) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_allreduce_u64: bad argument");
    if (!e->has_comm()) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_allreduce_u64: no communicator (az_comm_init)");
    if (n == 0 && !e->local) return AZ_OK;      // in-process, n = 0 still meets the peers: a rank that passed another n must hear of it
    return comm_sum_u64(e, values, n, args_ok);
}

struct CommHello { long long n, cap, dst, pad; };

// primitive 1: all-gather of the per-rank hello records.  RCCL: through d_stage (world + 1 records of device memory) on the engine's
// stream; in-process: one round of host records.
static az_status comm_allgather_hello(az_engine* e, const CommHello& mine, CommHello* d_stage, std::vector<CommHello>& hello) {
    const int world = e->comm_world;
    hello.resize((size_t)world);
    if (e->local) {
        std::vector<unsigned char> all;
        const std::string err = e->local->all_gather(e->comm_rank, LOCAL_OP_GATHER_HELLO, 0, &mine, sizeof mine, &all);
        if (!err.empty()) return fail(e, AZ_ERR_BAD_ARGUMENT, err);
        std::memcpy(hello.data(), all.data(), all.size());
        return AZ_OK;
    }
    hipStream_t s = e->stream;
    HIPCHK(hipMemcpyAsync(d_stage + world, &mine, sizeof mine, hipMemcpyHostToDevice, s));
    NCCLCHK(g_rccl.AllGather(d_stage + world, d_stage, sizeof(CommHello), ncclUint8, e->comm, s));
    HIPCHK(hipMemcpyAsync(hello.data(), d_stage, (size_t)world * sizeof(CommHello), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return AZ_OK;
}

// primitive 3: the exchange of the packed tuples.  off[r] = rank r's first tuple in rank order (off[world] = total); d_all = the
// receive area of a receiving rank.  RCCL: ONE grouped gatherv (a receiving rank posts a receive per peer, a sending rank one send
// per receiver).  In-process, host-synchronous (no stream ever waits on another engine's event): every rank publishes its packed
// block (device pointer, count) at barrier A, a receiving rank copies every rank's block into d_all on its own stream and
// synchronises it, and barrier B keeps every sender's block alive (comm_scratch may move it) until every copy is done.  pack_ok =
// false (in-process only): this rank's packing failed; it still meets its peers, and every rank returns the same error.
static az_status comm_exchange(az_engine* e, const PackedSample* d_mine, bool pack_ok, const std::vector<long long>& off, int dst_rank,
                               bool receiver, PackedSample* d_all) {
    const int world = e->comm_world, rank = e->comm_rank;
    hipStream_t s = e->stream;
    const long long n = off[(size_t)rank + 1] - off[(size_t)rank];
    if (e->local) {
        struct Post { unsigned long long ptr; long long n; int32_t ok, pad; };
        bool ok = pack_ok;
        if (ok && hipStreamSynchronize(s) != hipSuccess) ok = false;          // 1. packed and synchronised
        const Post mine{(unsigned long long)(uintptr_t)d_mine, n, ok ? 1 : 0, 0};
        std::vector<unsigned char> all;
        std::string err = e->local->all_gather(rank, LOCAL_OP_GATHER_POST, 0, &mine, sizeof mine, &all);     // 2. barrier A
        if (!err.empty()) return fail(e, AZ_ERR_BAD_ARGUMENT, err);
        std::vector<Post> post((size_t)world);
        std::memcpy(post.data(), all.data(), all.size());
        for (int r = 0; r < world; ++r)
            if (!post[(size_t)r].ok) return fail(e, AZ_ERR_HIP, "az_gather_samples: rank " + std::to_string(r) + " could not stage its tuples (HIP error); nothing was exchanged");
        int32_t copied = 1;                                                    // 3. the receivers' copies, on their own streams
        if (receiver) {
            for (int r = 0; r < world && copied; ++r) {
                const long long cr = off[(size_t)r + 1] - off[(size_t)r];
                if (cr > 0 && hipMemcpyAsync(d_all + off[(size_t)r], (const void*)(uintptr_t)post[(size_t)r].ptr, (size_t)cr * sizeof(PackedSample),
                                             hipMemcpyDefault, s) != hipSuccess) copied = 0;
            }
            if (hipStreamSynchronize(s) != hipSuccess) copied = 0;
        }
        err = e->local->all_gather(rank, LOCAL_OP_GATHER_DONE, 0, &copied, sizeof copied, &all);          // 4. barrier B
        if (!err.empty()) return fail(e, AZ_ERR_BAD_ARGUMENT, err);
        for (int r = 0; r < world; ++r) {
            int32_t c;
            std::memcpy(&c, all.data() + (size_t)r * sizeof c, sizeof c);
            if (!c) return fail(e, AZ_ERR_HIP, "az_gather_samples: rank " + std::to_string(r) + "'s copies of the exchange failed (HIP error)");
        }
        return AZ_OK;
    }
    struct GroupGuard {          // an error between GroupStart and GroupEnd must not leave the group open
        bool open = false;
        ~GroupGuard() { if (open) (void)g_rccl.GroupEnd(); }
    } group;
    NCCLCHK(g_rccl.GroupStart());
    group.open = true;
    for (int r = 0; r < world; ++r) {
        const long long cr = off[(size_t)r + 1] - off[(size_t)r];
        if (receiver) {
            if (r != rank && cr > 0) NCCLCHK(g_rccl.Recv(d_all + off[(size_t)r], (size_t)cr * sizeof(PackedSample), ncclUint8, r, e->comm, s));
            if (r == rank && n > 0) HIPCHK(hipMemcpyAsync(d_all + off[(size_t)r], d_mine, (size_t)n * sizeof(PackedSample), hipMemcpyDeviceToDevice, s));
        }
        if (r != rank && n > 0 && (dst_rank < 0 || r == dst_rank)) NCCLCHK(g_rccl.Send(d_mine, (size_t)n * sizeof(PackedSample), ncclUint8, r, e->comm, s));
    }
    group.open = false;
    NCCLCHK(g_rccl.GroupEnd());
    return AZ_OK;
}

// The episode-batch exchange.  EVERY decision that could make one rank leave early is taken from data every rank holds: the first
// collective carries, per rank, its tuple count (or -1: its local buffers are unusable), the capacity it can receive into (-1: not a
// receiver, -2: receive buffers unusable) and its dst_rank -- so either every rank posts its part of the exchange or every rank
// returns the same error without posting anything.  (Round 3's version returned on the receiving rank alone and left its peers
// waiting in ncclGroupEnd.)
az_status az_gather_samples(az_engine* e, const az_samples* local, int32_t dst_rank, az_samples* gathered, int64_t* counts_out) {
    if (!e || !local) return AZ_ERR_BAD_ARGUMENT;
    if (!e->has_comm()) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_gather_samples: no communicator (az_comm_init)");
    const int world = e->comm_world, rank = e->comm_rank;
    long long n = local->count;
    const bool dst_ok = dst_rank >= -1 && dst_rank < world;
    const bool receiver = dst_ok && (dst_rank < 0 || rank == dst_rank);         // dst_rank = -1: every rank receives (all-gather)
    const bool local_ok = dst_ok && n >= 0 && (n == 0 || (local->states && local->pis && local->zs));
    const bool recv_ok = !receiver || (gathered && gathered->states && gathered->pis && gathered->zs && gathered->capacity >= 0);
    const CommHello mine{local_ok ? n : -1, !receiver ? -1 : (recv_ok ? gathered->capacity : -2), dst_rank, 0};
    if (!local_ok) n = 0;
    try {
        HIPCHK(hipSetDevice(e->device));
        hipStream_t s = e->stream;
        // one allocation, kept by the engine and grown on demand (it was five to nine hipMalloc / hipFree pairs per call):
        // [hello x (world + 1)] [st | pi | z | packed] of the local tuples; the receive side is carved once the total is known
        const size_t hello_b = ((size_t)world + 1) * sizeof(CommHello);
        const size_t local_b = (size_t)n * (16 + 28 + 4 + sizeof(PackedSample));
        char* base = nullptr;
        try {
            base = (char*)e->comm_scratch.ensure(hello_b + local_b + 256, s);
        } catch (const HipFail&) {      // in-process the hello needs no device memory: the failure is met again (and published) at step 2
            if (!e->local) throw;
        }
        // 1. all-gather of the per-rank hello records (count, receive capacity, dst_rank)
        std::vector<CommHello> hello;
        az_status st = comm_allgather_hello(e, mine, (CommHello*)base, hello);
        if (st) return st;
        long long total = 0;
        int bad_local = -1, bad_recv = -1, bad_dst = -1;
        for (int r = 0; r < world; ++r) {
            if (hello[r].n < 0) { if (bad_local < 0) bad_local = r; } else total += hello[r].n;
            if (hello[r].dst != hello[0].dst || hello[r].dst < -1 || hello[r].dst >= world) { if (bad_dst < 0) bad_dst = r; }
        }
        for (int r = 0; r < world; ++r) {
            if (counts_out) counts_out[r] = hello[r].n < 0 ? 0 : hello[r].n;
            if (hello[r].cap == -2 || (hello[r].cap >= 0 && hello[r].cap < total)) { if (bad_recv < 0) bad_recv = r; }
        }
        // the same verdict on every rank, before anything is posted
        if (bad_dst >= 0) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_gather_samples: dst_rank outside the communicator or not the same on every rank (rank " + std::to_string(bad_dst) + ")");
        if (bad_local >= 0) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_gather_samples: rank " + std::to_string(bad_local) + "'s local tuples need states, pis and zs");
        if (bad_recv >= 0) return fail(e, AZ_ERR_BAD_ARGUMENT, "az_gather_samples: rank " + std::to_string(bad_recv) + "'s gathered buffers are missing or too small for " + std::to_string(total) + " tuples");
        std::vector<long long> off((size_t)world + 1, 0);           // rank r's tuples start at off[r] of the rank-order result
        for (int r = 0; r < world; ++r) off[(size_t)r + 1] = off[(size_t)r] + hello[r].n;
        // 2. pack this rank's tuples (inputs may be host or device memory).  In-process, a failure here is published at the exchange
        // (the peers are about to wait for this rank there); over RCCL it returns before anything is posted, as it always did.
        const size_t recv_b = receiver ? (size_t)total * (sizeof(PackedSample) + 16 + 28 + 4) : 0;
        char* cur = nullptr;
        auto carve = [&](size_t bytes) { char* q = cur; cur += (bytes + 63) / 64 * 64; return q; };
        PackedSample* d_mine = nullptr;
        bool pack_ok = true;
        try {
            base = (char*)e->comm_scratch.ensure(hello_b + local_b + recv_b + 512, s);      // may move: nothing of step 1 is needed any more
            cur = base + hello_b;
            ulonglong2* d_st = (ulonglong2*)carve((size_t)n * 16);
            float* d_pi = (float*)carve((size_t)n * 28);
            float* d_z = (float*)carve((size_t)n * 4);
            d_mine = (PackedSample*)carve((size_t)n * sizeof(PackedSample));
            if (n > 0) {
                HIPCHK(hipMemcpyAsync(d_st, local->states, (size_t)n * 16, hipMemcpyDefault, s));
                HIPCHK(hipMemcpyAsync(d_pi, local->pis, (size_t)n * 28, hipMemcpyDefault, s));
                HIPCHK(hipMemcpyAsync(d_z, local->zs, (size_t)n * 4, hipMemcpyDefault, s));
                hipLaunchKernelGGL(k_pack_samples, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, d_st, d_pi, d_z, d_mine, n);
            }
        } catch (const HipFail&) {
            if (!e->local) throw;
            pack_ok = false;
        }
        // 3. ONE exchange
        PackedSample* d_all = receiver && pack_ok ? (PackedSample*)carve((size_t)total * sizeof(PackedSample)) : nullptr;
        st = comm_exchange(e, d_mine, pack_ok, off, dst_rank, receiver, d_all);
        if (st) return st;
        // 4. unpack into the caller's buffers
        if (receiver) {
            ulonglong2* o_st = (ulonglong2*)carve((size_t)total * 16);
            float* o_pi = (float*)carve((size_t)total * 28);
            float* o_z = (float*)carve((size_t)total * 4);
            if (total > 0) hipLaunchKernelGGL(k_unpack_samples, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, d_all, o_st, o_pi, o_z, total);
            if (total > 0) {
                HIPCHK(hipMemcpyAsync(gathered->states, o_st, (size_t)total * 16, hipMemcpyDefault, s));
                HIPCHK(hipMemcpyAsync(gathered->pis, o_pi, (size_t)total * 28, hipMemcpyDefault, s));
                HIPCHK(hipMemcpyAsync(gathered->zs, o_z, (size_t)total * 4, hipMemcpyDefault, s));
            }
            HIPCHK(hipStreamSynchronize(s));
            gathered->count = total;
        } else {
            HIPCHK(hipStreamSynchronize(s));
            if (gathered) gathered->count = 0;
        }
        return AZ_OK;
    } catch (const HipFail& f) { return fail_hip(e, f); }
}

#ifdef AZ_DIAG
// Diagnostic library only (not part of the ABI): conv3's output of the last forward on the engine's first stream, `rows` boards of
// [4][5][C] bf16, copied to `out`.  Returns the number of bytes, or -1.
long long az_diag_read_conv3_out(az_engine* e, int rows, void* out) {
    if (!e || !out || rows <= 0 || hipSetDevice(e->device) != hipSuccess || hipStreamSynchronize(e->stream) != hipSuccess) return -1;
    return netws_read_conv3_out(e->ws[0], rows, out);
}
// Diagnostic library only: any layer's activations of the last forward on the engine's first stream (layer 1 act1 .. 6 fc2o, bf16:
// netws_read_act), and rows of a model's conv1 / conv2 tables (convnet_read_conv_table).  Bytes copied, or -1.
long long az_diag_read_act(az_engine* e, int layer, int rows, void* out) {
    if (!e || !out || rows <= 0 || hipSetDevice(e->device) != hipSuccess || hipStreamSynchronize(e->stream) != hipSuccess) return -1;
    return netws_read_act(e->ws[0], layer, rows, out);
}
// Diagnostic library only: ONE forward of a conv model on the engine's first stream with the three numbers a search hands the launchers
// given apart -- the exact row count n (EvalBatch::n, read on the device), the host's bound rows_hint (the grids) and its estimate rows_typ
// (the kernel families; 0 = none) -- where az_net_predict_states can only run rows_hint == n, rows_typ == 0.  Rows in the caller's order, no
// de-duplication, no canonicalisation ("eval_mirror" on: refused).  All rows_hint rows of the device's pi / v are filled with
// AZ_DIAG_HINTED_SENTINEL before the forward and all of them are copied back to the host (pi [rows_hint][7], v [rows_hint]): a row no
// kernel wrote still holds it.  The workspace's act2 .. fc2o rows [0, rows_hint) are filled with NaN bytes first (netws_poison_acts), so
// an element no kernel wrote reads as such and never as an earlier forward's right answer.  The readers above then read this forward's
// layers.  Bytes copied, or -1 and nothing written.
constexpr uint32_t AZ_DIAG_HINTED_SENTINEL = 0x7FC5A5A5u;      // a quiet NaN no kernel computes
long long az_diag_predict_hinted(az_engine* e, int32_t model_id, const uint64_t* states, int n, int rows_hint, int rows_typ, float* pi, float* v) {
    if (!e || !states || !pi || !v || n < 1 || rows_hint < n || rows_hint > e->cfg.max_batch || rows_typ < 0 || e->eval_mirror != 0) return -1;
    auto it = e->nets.find(model_id);
    if (it == e->nets.end() || it->second.kind != AZ_NET_CONV || !it->second.conv) return -1;
    try {
        HIPCHK(hipSetDevice(e->device));
        DeviceMem mem;
        const size_t rows = (size_t)rows_hint;
        EvalBatch eb{};
        eb.cap = rows_hint;
        eb.n = mem.alloc<uint32_t>(1);
        eb.state = mem.alloc<ulonglong2>(rows);
        eb.pi = mem.alloc<float>(rows * 8);
        eb.v = mem.alloc<float>(rows);
        const uint32_t nb = (uint32_t)n;
        std::vector<uint32_t> fill(rows * 8, AZ_DIAG_HINTED_SENTINEL);
        HIPCHK(hipMemcpyAsync(eb.n, &nb, sizeof nb, hipMemcpyHostToDevice, e->stream));
        HIPCHK(hipMemsetAsync(eb.state, 0, rows * 16, e->stream));                       // rows past n: the empty board
        HIPCHK(hipMemcpyAsync(eb.state, states, (size_t)n * 16, hipMemcpyHostToDevice, e->stream));
        HIPCHK(hipMemcpyAsync(eb.pi, fill.data(), rows * 32, hipMemcpyHostToDevice, e->stream));
        HIPCHK(hipMemcpyAsync(eb.v, fill.data(), rows * 4, hipMemcpyHostToDevice, e->stream));
        if (!netws_poison_acts(workspace_for(e, e->stream), rows_hint, e->stream)) return -1;
        net_forward(e, it->second, eb, rows_hint, e->stream, rows_typ, false);
        HIPCHK(hipGetLastError());
        std::vector<float> hp(rows * 8), hv(rows);
        HIPCHK(hipMemcpyAsync(hp.data(), eb.pi, rows * 32, hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipMemcpyAsync(hv.data(), eb.v, rows * 4, hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        for (size_t i = 0; i < rows; ++i)
            for (int a = 0; a < 7; ++a) pi[i * 7 + a] = hp[i * 8 + a];
        std::memcpy(v, hv.data(), rows * 4);
        return (long long)(rows * 32);
    } catch (const HipFail&) { return -1; }
}
long long az_diag_read_conv_table(az_engine* e, int32_t model_id, int which, int first_row, int n_rows, void* out) {
    if (!e || !out || hipSetDevice(e->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return -1;
    auto it = e->nets.find(model_id);
    if (it == e->nets.end() || !it->second.conv) return -1;
    return convnet_read_conv_table(it->second.conv, which, first_row, n_rows, out);
}
// Diagnostic library only: the same for a "net_fp8" engine -- `rows` boards of [4][5][C] e4m3 codes; and a model's (sa2, sa3)
long long az_diag_read_conv3_out_fp8(az_engine* e, int rows, void* out) {
    if (!e || !out || rows <= 0 || hipSetDevice(e->device) != hipSuccess || hipStreamSynchronize(e->stream) != hipSuccess) return -1;
    return netws_read_conv3_out_fp8(e->ws[0], rows, out);
}
long long az_diag_read_conv2_out_fp8(az_engine* e, int rows, void* out) {        // conv2's: `rows` boards of [6][7][C] e4m3 codes
    if (!e || !out || rows <= 0 || hipSetDevice(e->device) != hipSuccess || hipStreamSynchronize(e->stream) != hipSuccess) return -1;
    return netws_read_conv2_out_fp8(e->ws[0], rows, out);
}
int az_diag_fp8_scales(az_engine* e, int32_t model_id, float* out2) {
    if (!e || !out2) return -1;
    auto it = e->nets.find(model_id);
    return it != e->nets.end() && it->second.conv && convnet_fp8_scales(it->second.conv, out2) ? 0 : -1;
}
// Diagnostic library only: k_gemm_skinny_f8 launches the engine has issued since az_create (both streams' workspaces; a launch
// captured into a search graph counts once, at the capture)
long long az_diag_fp8_skinny_launches(az_engine* e) {
    if (!e) return -1;
    long long n = 0;
    for (NetWorkspace* w : e->ws) n += (long long)netws_fp8_skinny_launches(w);
    return n;
}
// Diagnostic library only: the 15-bit counter that hands out evaluation-cache tags (retag_model), so that a test can place its wrap.
// Returns the previous value, or -1 when the value is outside 1 .. 0x8000.
long long az_diag_set_next_cache_tag(az_engine* e, long long next) {
    if (!e || next < 1 || next > 0x8000) return -1;
    const long long was = (long long)e->next_cache_tag;
    e->next_cache_tag = (uint64_t)next;
    return was;
}
// Diagnostic library only: the trainer's workspace after an az_net_train_step (az_train.h TrainDiagBuf: z, a, mean, invstd of a layer,
// the heads' logits / dhead / per-sample losses, and -- from steps taken while keep is on -- every layer's d loss / d a and dz).  keep:
// 0, or -1 refused (no training session yet, "train_fork" 1).  read: bytes copied, or -1 and nothing copied.
int az_diag_train_keep(az_engine* e, int on) {
    if (!e || !e->trainer || hipSetDevice(e->device) != hipSuccess) return -1;
    if (on && e->train_sw.fork) return -1;
    return trainer_diag_set_keep(e->trainer, on != 0) ? 0 : -1;
}
// Diagnostic library only: the plan (csrc/az_train_plan.h train_plan_encode) the trainer would follow for a step of batch b under its
// current switches -> the int32 count, or -1 (no training session yet, b outside 2 .. 256, cap too small).  Host only, launches nothing.
int az_diag_train_plan(az_engine* e, int b, int32_t* out, int cap) {
    return e && e->trainer ? trainer_diag_plan(e->trainer, b, out, cap) : -1;
}
long long az_diag_train_read(az_engine* e, int what, int layer, int rows, void* out) {
    if (!e || !e->trainer || !out || hipSetDevice(e->device) != hipSuccess) return -1;
    return trainer_diag_read(e->trainer, what, layer, rows, out, e->stream);
}
// Diagnostic library only (not part of the ABI): the children of the node reached from tree g's current root by following `path`
// (child indices, not actions).  out rows of 8 u64: slot, a, ctr (resolved through a link), prior bits, link, meta, own ctr, key.
// Returns the number of children, or -1.
int az_diag_tree_children(az_tree* t, int g, const int* path, int depth, unsigned long long* out) {
    if (!t || g < 0 || g >= t->th.d.G) return -1;
    TreeDev& d = t->th.d;
    std::vector<TreeLine> heads(d.G);
    if (hipMemcpy(heads.data(), d.head, heads.size() * sizeof(TreeLine), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    struct Rec { unsigned long long ctr, key; uint32_t prior, meta, link, child_base; };
    auto load = [&](uint32_t slot, Rec* r) {
        uint32_t raw[4];
        if (hipMemcpy(raw, d.node + ((size_t)g * d.R + slot), 16, hipMemcpyDeviceToHost) != hipSuccess) return false;
        if (hipMemcpy(&r->key, d.key + ((size_t)g * d.R + slot), 8, hipMemcpyDeviceToHost) != hipSuccess) return false;
        const uint32_t w = raw[3], kind = (w >> 10) & 3u, payload = w >> 12;
        r->ctr = ((unsigned long long)raw[1] << 32) | raw[0];
        r->prior = raw[2];
        r->meta = (w & 0x3Fu) | (((w >> 6) & 0xFu) << META_ECODE_SHIFT) | (kind == 2u ? META_EXPANDED : 0u);
        r->link = kind == 1u ? payload : NONE;
        r->child_base = kind == 2u ? payload * (uint32_t)BLOCK_SLOTS : 0u;
        if (kind != 2u) r->key = 0;
        return true;
    };
    uint32_t cur = heads[g].head.root;
    Rec pr;
    if (!load(cur, &pr)) return -1;
    for (int i = 0; i < depth; ++i) {
        Rec c;
        if (!load(pr.child_base + (uint32_t)path[i], &c)) return -1;
        cur = c.link != NONE ? c.link : pr.child_base + (uint32_t)path[i];
        if (!load(cur, &pr)) return -1;
    }
    const int n = (int)((pr.meta >> META_NCHILD_SHIFT) & 7u);
    for (int j = 0; j < n; ++j) {
        Rec c, r;
        if (!load(pr.child_base + (uint32_t)j, &c)) return -1;
        r = c;
        if (c.link != NONE && !load(c.link, &r)) return -1;
        unsigned long long* o = out + 8 * j;
        o[0] = pr.child_base + (uint32_t)j; o[1] = c.meta & META_A_MASK; o[2] = r.ctr; o[3] = c.prior; o[4] = c.link; o[5] = r.meta; o[6] = c.ctr; o[7] = r.key;
    }
    out[8 * 7] = pr.ctr; out[8 * 7 + 1] = pr.key; out[8 * 7 + 2] = cur;
    return n;
}
void az_diag_tree_set_sims(az_tree* t, int num_sims) { if (t) t->num_sims = num_sims; }
#endif

}  // extern "C"
