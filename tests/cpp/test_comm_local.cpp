// test_comm_local.cpp -- the in-process communicator (az_comm_local_id) on one device: `world` engines of this process, one host
// thread per rank, through the C ABI.  Run by tests/test_comm_local_gpu.py; prints one JSON line of counts (any violated rule is
// counted, never asserted).  Every mode runs under a watchdog that exits non-zero (without aborting) if a collective deadlocks.
//
//   gather   <world>   ragged counts (a zero-count rank included), dst_rank 0 / last / -1, host and device buffers
//   refuse   <world>   receiver too small, missing local buffers, dst_rank disagreement: every rank refused with one message, then
//                      a correct gather
//   allreduce <world>  n = 0, 3, 64, sums that wrap mod 2^64
//   arena    <world>   az_arena with allreduce_wld on shards of a 24-game arena (an empty shard, a finished start board)
//   misuse             mismatched collectives, a rank that leaves while a peer waits, refused inits, az_destroy of a member
//   time     <world> <tuples per rank> <reps>   wall time of one az_gather_samples (dst_rank -1, device buffers)
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "az_engine.h"

namespace {

std::atomic<long> g_bad{0};
#define EXPECT(c) do { if (!(c)) { g_bad += 1; std::fprintf(stderr, "line %d: %s\n", __LINE__, #c); } } while (0)

az_engine* make_engine() {
    az_config cfg{0, 64, 128, 0, 0};
    az_engine* e = nullptr;
    if (az_create(&cfg, &e) != AZ_OK) { std::fprintf(stderr, "az_create failed\n"); std::exit(1); }
    az_set_option(e, "search_graph", 0);       // engines of one device driven at once (include/az_engine.h)
    az_set_option(e, "train_graph", 0);
    az_set_option(e, "eval_cache_log2", 12);
    return e;
}

// one thread per rank: fn(rank) runs on its own host thread; returns once every rank is done
void per_rank(int world, const std::function<void(int)>& fn) {
    std::vector<std::thread> th;
    for (int r = 0; r < world; ++r) th.emplace_back(fn, r);
    for (auto& t : th) t.join();
}

std::vector<az_engine*> make_world(int world) {
    std::vector<az_engine*> es((size_t)world);
    for (auto& e : es) e = make_engine();
    uint8_t id[AZ_COMM_ID_BYTES];
    if (az_comm_local_id(es[0], world, id) != AZ_OK) { std::fprintf(stderr, "az_comm_local_id: %s\n", az_last_error(es[0])); std::exit(1); }
    per_rank(world, [&](int r) { EXPECT(az_comm_init(es[(size_t)r], r, world, id) == AZ_OK); });
    return es;
}
void end_world(std::vector<az_engine*>& es) {
    for (auto* e : es) { EXPECT(az_comm_destroy(e) == AZ_OK); az_destroy(e); }
    es.clear();
}

uint64_t mix(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// a rank's tuples: states [n,2], pis [n,7], zs [n] (any bits: a gather moves them, it does not look at them)
struct Tuples {
    std::vector<uint64_t> st;
    std::vector<float> pi, z;
    void make(int rank, int c, long long n) {
        st.resize((size_t)n * 2); pi.resize((size_t)n * 7); z.resize((size_t)n);
        for (long long i = 0; i < n; ++i) {
            const uint64_t h = mix(((uint64_t)rank << 40) ^ ((uint64_t)c << 32) ^ (uint64_t)i);
            st[(size_t)i * 2] = h; st[(size_t)i * 2 + 1] = mix(h);
            for (int a = 0; a < 7; ++a) { const uint32_t b = (uint32_t)(mix(h + (uint64_t)a) >> 9); std::memcpy(&pi[(size_t)i * 7 + a], &b, 4); }
            const uint32_t b = (uint32_t)(mix(h ^ 77) >> 9);
            std::memcpy(&z[(size_t)i], &b, 4);
        }
    }
};

// device copies of host arrays (made and read on the main thread, outside the collectives)
struct DevBuf {
    void* p = nullptr;
    explicit DevBuf(size_t bytes) { if (hipMalloc(&p, std::max<size_t>(bytes, 1)) != hipSuccess) { std::fprintf(stderr, "hipMalloc\n"); std::exit(1); } }
    ~DevBuf() { (void)hipFree(p); }
    DevBuf(const DevBuf&) = delete;
};
void up(DevBuf& d, const void* h, size_t bytes) { if (bytes) EXPECT(hipMemcpy(d.p, h, bytes, hipMemcpyHostToDevice) == hipSuccess); }
void down(void* h, const DevBuf& d, size_t bytes) { if (bytes) EXPECT(hipMemcpy(h, d.p, bytes, hipMemcpyDeviceToHost) == hipSuccess); }

long long count_of(int pattern, int world, int r) {
    static const long long A[4] = {517, 0, 1203, 88}, B[4] = {0, 64, 1, 3000};
    return (pattern ? B : A)[(r + pattern * (world - 1)) % 4];
}

int mode_gather(int world) {
    auto es = make_world(world);
    long cases = 0;
    for (int pattern = 0; pattern < 2; ++pattern)
        for (int dst : {0, world - 1, -1})
            for (int dev = 0; dev < 2; ++dev) {           // 0: host buffers, 1: device buffers on both sides
                const int c = pattern * 100 + (dst + 1) * 10 + dev;
                std::vector<Tuples> loc((size_t)world);
                long long total = 0;
                for (int r = 0; r < world; ++r) { loc[(size_t)r].make(r, c, count_of(pattern, world, r)); total += count_of(pattern, world, r); }
                const long long cap = total + 3;
                std::vector<Tuples> got((size_t)world);
                std::vector<std::vector<int64_t>> counts((size_t)world, std::vector<int64_t>((size_t)world, -7));
                std::vector<std::unique_ptr<DevBuf>> dbuf;      // per rank: local st, pi, z, gathered st, pi, z
                for (int r = 0; r < world; ++r) {
                    const long long n = count_of(pattern, world, r);
                    got[(size_t)r].st.assign((size_t)cap * 2, 0); got[(size_t)r].pi.assign((size_t)cap * 7, 0.f); got[(size_t)r].z.assign((size_t)cap, 0.f);
                    if (dev) {
                        for (size_t b : {(size_t)n * 16, (size_t)n * 28, (size_t)n * 4, (size_t)cap * 16, (size_t)cap * 28, (size_t)cap * 4})
                            dbuf.emplace_back(new DevBuf(b));
                        up(*dbuf[(size_t)r * 6], loc[(size_t)r].st.data(), (size_t)n * 16);
                        up(*dbuf[(size_t)r * 6 + 1], loc[(size_t)r].pi.data(), (size_t)n * 28);
                        up(*dbuf[(size_t)r * 6 + 2], loc[(size_t)r].z.data(), (size_t)n * 4);
                    }
                }
                std::vector<int64_t> got_count((size_t)world, -1);
                per_rank(world, [&](int r) {
                    const long long n = count_of(pattern, world, r);
                    az_samples l{}, g{};
                    l.capacity = n; l.count = n;
                    l.states = dev ? (uint64_t*)dbuf[(size_t)r * 6]->p : loc[(size_t)r].st.data();
                    l.pis = dev ? (float*)dbuf[(size_t)r * 6 + 1]->p : loc[(size_t)r].pi.data();
                    l.zs = dev ? (float*)dbuf[(size_t)r * 6 + 2]->p : loc[(size_t)r].z.data();
                    g.capacity = cap; g.count = -5;
                    g.states = dev ? (uint64_t*)dbuf[(size_t)r * 6 + 3]->p : got[(size_t)r].st.data();
                    g.pis = dev ? (float*)dbuf[(size_t)r * 6 + 4]->p : got[(size_t)r].pi.data();
                    g.zs = dev ? (float*)dbuf[(size_t)r * 6 + 5]->p : got[(size_t)r].z.data();
                    const bool receiver = dst < 0 || dst == r;
                    // a non-receiver passes NULL on the host-buffer cases and a buffer it does not need on the device ones
                    az_samples* gp = receiver || dev ? &g : nullptr;
                    EXPECT(az_gather_samples(es[(size_t)r], &l, dst, gp, counts[(size_t)r].data()) == AZ_OK);
                    got_count[(size_t)r] = gp ? g.count : 0;
                });
                for (int r = 0; r < world; ++r) {
                    for (int q = 0; q < world; ++q) EXPECT(counts[(size_t)r][(size_t)q] == count_of(pattern, world, q));
                    const bool receiver = dst < 0 || dst == r;
                    EXPECT(got_count[(size_t)r] == (receiver ? total : 0));
                    if (!receiver) continue;
                    Tuples& o = got[(size_t)r];
                    if (dev) {
                        down(o.st.data(), *dbuf[(size_t)r * 6 + 3], (size_t)total * 16);
                        down(o.pi.data(), *dbuf[(size_t)r * 6 + 4], (size_t)total * 28);
                        down(o.z.data(), *dbuf[(size_t)r * 6 + 5], (size_t)total * 4);
                    }
                    long long at = 0;                          // the rank-order concatenation, bit for bit
                    for (int q = 0; q < world; ++q) {
                        const Tuples& s = loc[(size_t)q];
                        const size_t n = s.z.size();
                        EXPECT(n == 0 || std::memcmp(o.st.data() + at * 2, s.st.data(), n * 16) == 0);
                        EXPECT(n == 0 || std::memcmp(o.pi.data() + at * 7, s.pi.data(), n * 28) == 0);
                        EXPECT(n == 0 || std::memcmp(o.z.data() + at, s.z.data(), n * 4) == 0);
                        at += (long long)n;
                    }
                }
                ++cases;
            }
    end_world(es);
    std::printf("{\"mode\": \"gather\", \"world\": %d, \"cases\": %ld, \"bad\": %ld}\n", world, cases, g_bad.load());
    return 0;
}

// every rank calls az_gather_samples with what prep(rank, l, g) sets; returns the statuses and az_last_error messages
struct Verdict { std::vector<int> st; std::vector<std::string> msg; };
Verdict gather_all(std::vector<az_engine*>& es, int dst, const std::function<void(int, az_samples&, az_samples&)>& prep) {
    const int world = (int)es.size();
    Verdict v{std::vector<int>((size_t)world), std::vector<std::string>((size_t)world)};
    per_rank(world, [&](int r) {
        az_samples l{}, g{};
        prep(r, l, g);
        v.st[(size_t)r] = az_gather_samples(es[(size_t)r], &l, dst, &g, nullptr);
        v.msg[(size_t)r] = az_last_error(es[(size_t)r]);
    });
    return v;
}
bool same_refusal(const Verdict& v, int status, const char* needle) {
    for (size_t r = 0; r < v.st.size(); ++r)
        if (v.st[r] != status || v.msg[r] != v.msg[0]) return false;
    return v.msg[0].find(needle) != std::string::npos;
}

int mode_refuse(int world) {
    auto es = make_world(world);
    std::vector<Tuples> loc((size_t)world);
    for (int r = 0; r < world; ++r) loc[(size_t)r].make(r, 9, 10 + r);
    const long long total = 10LL * world + (long long)world * (world - 1) / 2;
    std::vector<Tuples> out((size_t)world);
    for (auto& o : out) { o.st.resize((size_t)total * 2); o.pi.resize((size_t)total * 7); o.z.resize((size_t)total); }
    auto good = [&](int r, az_samples& l, az_samples& g) {
        l.count = l.capacity = 10 + r; l.states = loc[(size_t)r].st.data(); l.pis = loc[(size_t)r].pi.data(); l.zs = loc[(size_t)r].z.data();
        g.capacity = total; g.states = out[(size_t)r].st.data(); g.pis = out[(size_t)r].pi.data(); g.zs = out[(size_t)r].z.data();
    };
    int refusals = 0, recovered = 0;
    auto recover = [&] {
        const Verdict ok = gather_all(es, -1, good);
        bool all = true;
        for (int r = 0; r < world; ++r) all = all && ok.st[(size_t)r] == AZ_OK && std::memcmp(out[(size_t)r].z.data() + total - (10 + world - 1), loc[(size_t)world - 1].z.data(), (size_t)(10 + world - 1) * 4) == 0;
        recovered += all ? 1 : 0;
    };
    // receiver too small on the last rank
    Verdict v = gather_all(es, -1, [&](int r, az_samples& l, az_samples& g) { good(r, l, g); if (r == world - 1) g.capacity = total - 1; });
    refusals += same_refusal(v, AZ_ERR_BAD_ARGUMENT, "too small") ? 1 : 0;
    recover();
    // missing local buffers on rank 0
    v = gather_all(es, -1, [&](int r, az_samples& l, az_samples& g) { good(r, l, g); if (r == 0) l.states = nullptr; });
    refusals += same_refusal(v, AZ_ERR_BAD_ARGUMENT, "local tuples need") ? 1 : 0;
    recover();
    // ranks that disagree on dst_rank: rank 1 says 0, the others -1 (each rank's own dst goes into its call)
    {
        Verdict w{std::vector<int>((size_t)world), std::vector<std::string>((size_t)world)};
        per_rank(world, [&](int r) {
            az_samples l{}, g{};
            good(r, l, g);
            w.st[(size_t)r] = az_gather_samples(es[(size_t)r], &l, r == 1 ? 0 : -1, &g, nullptr);
            w.msg[(size_t)r] = az_last_error(es[(size_t)r]);
        });
        refusals += same_refusal(w, AZ_ERR_BAD_ARGUMENT, "dst_rank") ? 1 : 0;
    }
    recover();
    end_world(es);
    std::printf("{\"mode\": \"refuse\", \"world\": %d, \"refusals\": %d, \"recovered\": %d, \"bad\": %ld}\n", world, refusals, recovered, g_bad.load());
    return 0;
}

int mode_allreduce(int world) {
    auto es = make_world(world);
    int checked = 0;
    for (int n : {0, 3, 64}) {
        std::vector<std::vector<uint64_t>> v((size_t)world, std::vector<uint64_t>((size_t)std::max(n, 1)));
        for (int r = 0; r < world; ++r)
            for (int i = 0; i < n; ++i) v[(size_t)r][(size_t)i] = (i % 2 ? 0xFFFFFFFFFFFFFFF0ull : mix((uint64_t)(r * 64 + i))) + (uint64_t)r;
        std::vector<uint64_t> want((size_t)std::max(n, 1), 0);
        for (int r = 0; r < world; ++r) for (int i = 0; i < n; ++i) want[(size_t)i] += v[(size_t)r][(size_t)i];    // wraps mod 2^64
        per_rank(world, [&](int r) { EXPECT(az_allreduce_u64(es[(size_t)r], v[(size_t)r].data(), n) == AZ_OK); });
        for (int r = 0; r < world; ++r) { EXPECT(std::equal(want.begin(), want.begin() + n, v[(size_t)r].begin())); ++checked; }
    }
    end_world(es);
    std::printf("{\"mode\": \"allreduce\", \"world\": %d, \"checked\": %d, \"bad\": %ld}\n", world, checked, g_bad.load());
    return 0;
}

int mode_arena(int world) {
    const int total = 24;
    auto es = make_world(world);
    for (auto* e : es) { EXPECT(az_net_set_kind(e, 0, AZ_NET_HASH, 5) == AZ_OK); EXPECT(az_net_set_kind(e, 1, AZ_NET_HASH, 6) == AZ_OK); }
    az_engine* ref = make_engine();
    EXPECT(az_net_set_kind(ref, 0, AZ_NET_HASH, 5) == AZ_OK);
    EXPECT(az_net_set_kind(ref, 1, AZ_NET_HASH, 6) == AZ_OK);
    int cases = 0;
    for (int finished = 0; finished < 2; ++finished)
        for (int split = 0; split < 2; ++split) {                // 0: even shards; 1: rank 0's shard empty, the last rank takes the rest
            az_arena_params a{};
            a.num_games = total; a.num_sims = 25; a.max_depth = 1000; a.cpuct = 1; a.new_model_id = 0; a.old_model_id = 1;
            a.reserve = 1000000; a.seed = 11;
            if (finished) { a.use_start_board = 1; a.start_board[0] = 0; a.start_board[1] = 0b1 | (1 << 7) | (1 << 14) | (1 << 21); }
            uint64_t wld_ref[3];
            std::vector<int8_t> res_ref((size_t)total, 9);
            EXPECT(az_arena(ref, &a, wld_ref, res_ref.data()) == AZ_OK);
            std::vector<int> lo((size_t)world), hi((size_t)world);
            for (int r = 0; r < world; ++r) {
                lo[(size_t)r] = split ? (r == 0 ? 0 : (r - 1) * total / (world - 1)) : r * total / world;
                hi[(size_t)r] = split ? (r == 0 ? 0 : r * total / (world - 1)) : (r + 1) * total / world;
            }
            std::vector<std::array<uint64_t, 3>> wld((size_t)world);
            std::vector<std::vector<int8_t>> res((size_t)world);
            per_rank(world, [&](int r) {
                az_arena_params p = a;
                p.first_game = lo[(size_t)r]; p.num_games = hi[(size_t)r] - lo[(size_t)r]; p.total_games = total; p.allreduce_wld = 1;
                res[(size_t)r].assign((size_t)std::max(p.num_games, 1), 9);
                EXPECT(az_arena(es[(size_t)r], &p, wld[(size_t)r].data(), res[(size_t)r].data()) == AZ_OK);
            });
            for (int r = 0; r < world; ++r) {
                EXPECT(wld[(size_t)r][0] == wld_ref[0] && wld[(size_t)r][1] == wld_ref[1] && wld[(size_t)r][2] == wld_ref[2]);
                for (int gi = lo[(size_t)r]; gi < hi[(size_t)r]; ++gi) EXPECT(res[(size_t)r][(size_t)(gi - lo[(size_t)r])] == res_ref[(size_t)gi]);
            }
            ++cases;
        }
    az_destroy(ref);
    end_world(es);
    std::printf("{\"mode\": \"arena\", \"world\": %d, \"cases\": %d, \"bad\": %ld}\n", world, cases, g_bad.load());
    return 0;
}

int mode_misuse() {
    int checks = 0;
    auto pass = [&](bool ok, const char* what) { if (ok) ++checks; else { g_bad += 1; std::fprintf(stderr, "misuse: %s\n", what); } };
    {   // mismatched collectives, then different n, then a correct gather
        auto es = make_world(2);
        std::vector<int> st(2);
        std::vector<std::string> msg(2);
        Tuples t;
        t.make(0, 1, 4);
        std::vector<uint64_t> gs(16);
        std::vector<float> gp(56), gz(8);
        auto gather = [&](int r) {
            az_samples l{}, g{};
            l.count = l.capacity = 4; l.states = t.st.data(); l.pis = t.pi.data(); l.zs = t.z.data();
            g.capacity = 8; g.states = gs.data(); g.pis = gp.data(); g.zs = gz.data();
            return az_gather_samples(es[(size_t)r], &l, 0, r == 0 ? &g : nullptr, nullptr);
        };
        per_rank(2, [&](int r) {
            uint64_t v[3] = {1, 2, 3};
            st[(size_t)r] = r == 0 ? gather(r) : az_allreduce_u64(es[(size_t)r], v, 3);
            msg[(size_t)r] = az_last_error(es[(size_t)r]);
        });
        pass(st[0] == AZ_ERR_BAD_ARGUMENT && st[1] == AZ_ERR_BAD_ARGUMENT && msg[0] == msg[1] && msg[0].find("mismatched collectives") != std::string::npos &&
             msg[0].find("rank 1 in az_allreduce_u64") != std::string::npos, "mismatched collectives");
        per_rank(2, [&](int r) {
            uint64_t v[4] = {1, 2, 3, 4};
            st[(size_t)r] = az_allreduce_u64(es[(size_t)r], v, 3 + r);
            msg[(size_t)r] = az_last_error(es[(size_t)r]);
        });
        pass(st[0] == AZ_ERR_BAD_ARGUMENT && st[1] == AZ_ERR_BAD_ARGUMENT && msg[0] == msg[1] && msg[0].find("different n") != std::string::npos, "different n");
        per_rank(2, [&](int r) { st[(size_t)r] = gather(r); });
        pass(st[0] == AZ_OK && st[1] == AZ_OK && std::memcmp(gz.data(), t.z.data(), 16) == 0 && std::memcmp(gz.data() + 4, t.z.data(), 16) == 0,
             "a correct gather after the mismatches");
        end_world(es);
    }
    {   // a rank that calls az_comm_destroy while its peers wait in a collective
        auto es = make_world(3);
        std::vector<int> st(3, -1);
        std::vector<std::string> msg(3);
        std::atomic<int> waiting{0};
        per_rank(3, [&](int r) {
            uint64_t v[3] = {1, 2, 3};
            if (r == 2) {
                while (waiting.load() < 2) std::this_thread::sleep_for(std::chrono::milliseconds(1));
                std::this_thread::sleep_for(std::chrono::milliseconds(100));
                st[2] = az_comm_destroy(es[2]);
                return;
            }
            waiting += 1;
            st[(size_t)r] = az_allreduce_u64(es[(size_t)r], v, 3);
            msg[(size_t)r] = az_last_error(es[(size_t)r]);
        });
        pass(st[2] == AZ_OK && st[0] == AZ_ERR_BAD_ARGUMENT && st[1] == AZ_ERR_BAD_ARGUMENT && msg[0] == msg[1] &&
             msg[0].find("rank 2 left") != std::string::npos, "a rank that left wakes its waiting peers");
        uint64_t v[3] = {1, 2, 3};
        pass(az_allreduce_u64(es[0], v, 3) == AZ_ERR_BAD_ARGUMENT && v[0] == 1, "later collectives fail at once");
        end_world(es);
    }
    {   // refused inits: duplicate rank, wrong world, a reused id, an unknown serial, an engine that already has a communicator
        az_engine *a = make_engine(), *b = make_engine(), *c = make_engine();
        uint8_t id[AZ_COMM_ID_BYTES];
        pass(az_comm_local_id(a, 0, id) == AZ_ERR_BAD_ARGUMENT, "world 0");
        pass(az_comm_local_id(a, 2, id) == AZ_OK, "az_comm_local_id");
        int st_a = -1;
        std::thread ta([&] { st_a = az_comm_init(a, 0, 2, id); });      // blocks until rank 1 joins
        std::this_thread::sleep_for(std::chrono::milliseconds(50));
        pass(az_comm_init(c, 0, 2, id) == AZ_ERR_BAD_ARGUMENT && std::string(az_last_error(c)).find("already taken") != std::string::npos, "duplicate rank");
        pass(az_comm_init(c, 1, 3, id) == AZ_ERR_BAD_ARGUMENT && std::string(az_last_error(c)).find("differs") != std::string::npos, "wrong world");
        pass(az_comm_init(b, 1, 2, id) == AZ_OK, "rank 1 joins");
        ta.join();
        pass(st_a == AZ_OK, "rank 0 returned once the world was complete");
        pass(az_comm_init(c, 1, 2, id) == AZ_ERR_BAD_ARGUMENT && std::string(az_last_error(c)).find("already complete") != std::string::npos, "reused id");
        uint8_t bogus[AZ_COMM_ID_BYTES];
        std::memcpy(bogus, id, sizeof bogus);
        bogus[16] ^= 0x55;
        pass(az_comm_init(c, 0, 2, bogus) == AZ_ERR_BAD_ARGUMENT && std::string(az_last_error(c)).find("unknown") != std::string::npos, "unknown serial");
        uint8_t id2[AZ_COMM_ID_BYTES];
        pass(az_comm_local_id(a, 1, id2) == AZ_OK && az_comm_init(a, 0, 1, id2) == AZ_ERR_BAD_ARGUMENT, "an engine that already has a communicator");
        pass(az_comm_init(c, 0, 1, id2) == AZ_OK, "a world of one");
        uint64_t v[2] = {4, 5};
        pass(az_allreduce_u64(c, v, 2) == AZ_OK && v[0] == 4 && v[1] == 5, "world of one all-reduce");
        // az_destroy of a member without az_comm_destroy: the peer's pending collective fails
        std::atomic<int> waiting{0};
        int st_b = -1;
        std::string msg_b;
        std::thread tb([&] { waiting = 1; uint64_t w[3] = {1, 2, 3}; st_b = az_allreduce_u64(b, w, 3); msg_b = az_last_error(b); });
        while (!waiting.load()) std::this_thread::sleep_for(std::chrono::milliseconds(1));
        std::this_thread::sleep_for(std::chrono::milliseconds(100));
        az_destroy(a);
        tb.join();
        pass(st_b == AZ_ERR_BAD_ARGUMENT && msg_b.find("rank 0 left") != std::string::npos, "az_destroy of a member");
        pass(az_comm_destroy(b) == AZ_OK && az_comm_destroy(c) == AZ_OK, "the survivors leave");
        az_destroy(b);
        az_destroy(c);
    }
    std::printf("{\"mode\": \"misuse\", \"checks\": %d, \"bad\": %ld}\n", checks, g_bad.load());
    return 0;
}

int mode_time(int world, long long per_rank_n, int reps) {
    auto es = make_world(world);
    const long long total = per_rank_n * world;
    std::vector<std::unique_ptr<DevBuf>> d;
    for (int r = 0; r < world; ++r) {
        Tuples t;
        t.make(r, 3, per_rank_n);
        for (size_t b : {(size_t)per_rank_n * 16, (size_t)per_rank_n * 28, (size_t)per_rank_n * 4, (size_t)total * 16, (size_t)total * 28, (size_t)total * 4})
            d.emplace_back(new DevBuf(b));
        up(*d[(size_t)r * 6], t.st.data(), (size_t)per_rank_n * 16);
        up(*d[(size_t)r * 6 + 1], t.pi.data(), (size_t)per_rank_n * 28);
        up(*d[(size_t)r * 6 + 2], t.z.data(), (size_t)per_rank_n * 4);
    }
    std::vector<double> ms;
    for (int it = 0; it < reps + 2; ++it) {          // two warm-up calls (they size each engine's staging allocation)
        const auto t0 = std::chrono::steady_clock::now();
        per_rank(world, [&](int r) {
            az_samples l{}, g{};
            l.count = l.capacity = per_rank_n;
            l.states = (uint64_t*)d[(size_t)r * 6]->p; l.pis = (float*)d[(size_t)r * 6 + 1]->p; l.zs = (float*)d[(size_t)r * 6 + 2]->p;
            g.capacity = total;
            g.states = (uint64_t*)d[(size_t)r * 6 + 3]->p; g.pis = (float*)d[(size_t)r * 6 + 4]->p; g.zs = (float*)d[(size_t)r * 6 + 5]->p;
            EXPECT(az_gather_samples(es[(size_t)r], &l, -1, &g, nullptr) == AZ_OK && g.count == total);
        });
        if (it >= 2) ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    std::sort(ms.begin(), ms.end());
    end_world(es);
    std::printf("{\"mode\": \"time\", \"world\": %d, \"tuples_per_call\": %lld, \"reps\": %d, \"median_ms\": %.3f, \"min_ms\": %.3f, \"bad\": %ld}\n",
                world, total, reps, ms[ms.size() / 2], ms[0], g_bad.load());
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    const int world = argc > 2 ? std::atoi(argv[2]) : 2;
    std::thread([] {
        std::this_thread::sleep_for(std::chrono::seconds(150));
        std::fprintf(stderr, "watchdog: a collective deadlocked\n");
        std::fflush(stderr);
        std::_Exit(3);
    }).detach();
    if (mode == "gather") return mode_gather(world);
    if (mode == "refuse") return mode_refuse(world);
    if (mode == "allreduce") return mode_allreduce(world);
    if (mode == "arena") return mode_arena(world);
    if (mode == "misuse") return mode_misuse();
    if (mode == "time") return mode_time(world, argc > 3 ? std::atoll(argv[3]) : 42500, argc > 4 ? std::atoi(argv[4]) : 20);
    std::fprintf(stderr, "usage: test_comm_local gather|refuse|allreduce|arena <world> | misuse | time <world> <tuples per rank> <reps>\n");
    return 2;
}
