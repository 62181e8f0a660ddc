// test_local_comm_cpu.cpp -- the in-process communicator's rendezvous (alphazero-rs_amd/csrc/az_local_comm.h) on the CPU with host
// data only, built with -fsanitize=thread by tests/test_comm_local_cpu.py.  The three collectives are built here on
// LocalGroup::all_gather exactly as az_engine.hip builds them (the hello all-gather, the u64 sum, the exchange between barrier A and
// barrier B), with memcpy in place of the receivers' stream copies.  Prints one JSON line of counts; any violated rule is counted,
// never asserted.  A watchdog exits non-zero (without aborting) if the protocol deadlocks.
//
//   random <world> <rounds> <seed>   every rank joins, then runs the same seeded sequence of random collectives; some rounds are
//                                    deliberately mismatched (other op or other n on one rank): every rank must get the same error
//   leave  <world>                   the last rank leaves while the others wait in a collective: they wake with the same error, and
//                                    later collectives fail at once
//   ids                              refusals of az_comm_init: wrong world, rank taken, complete world, unknown serial, other process
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "az_local_comm.h"

namespace {

using az::LocalGroup;

struct Tuple { uint64_t s0, s1; float pi[7]; float z; };      // a stand-in of the engine's 48-byte packed tuple

uint64_t mix(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
Tuple tuple_of(int rank, uint64_t round, long long i) {
    Tuple t{};
    t.s0 = mix(((uint64_t)rank << 48) ^ (round << 24) ^ (uint64_t)i);
    t.s1 = mix(t.s0);
    for (int a = 0; a < 7; ++a) t.pi[a] = (float)((t.s1 >> (a * 8)) & 0xFF) / 255.f;
    t.z = (float)((int)(t.s0 & 3) - 1);
    return t;
}

// the engine's three primitives on host memory
struct Hello { long long n, cap, dst, pad; };
std::string gather_hello(LocalGroup& g, int rank, const Hello& mine, std::vector<Hello>* out) {
    std::vector<unsigned char> all;
    std::string err = g.all_gather(rank, az::LOCAL_OP_GATHER_HELLO, 0, &mine, sizeof mine, &all);
    if (err.empty()) {
        out->resize((size_t)g.world());
        std::memcpy(out->data(), all.data(), all.size());
    }
    return err;
}
std::string sum_u64(LocalGroup& g, int rank, uint64_t* v, int n) {
    uint64_t rec[65] = {1};
    std::memcpy(rec + 1, v, (size_t)n * 8);
    std::vector<unsigned char> all;
    std::string err = g.all_gather(rank, az::LOCAL_OP_ALLREDUCE, n, rec, sizeof rec, &all);
    if (!err.empty()) return err;
    uint64_t sum[64] = {};
    for (int r = 0; r < g.world(); ++r)
        for (int i = 0; i < n; ++i) {
            uint64_t x;
            std::memcpy(&x, all.data() + (size_t)r * sizeof rec + 8 * (size_t)(1 + i), 8);
            sum[i] += x;
        }
    std::memcpy(v, sum, (size_t)n * 8);
    return err;
}
// one gather (dst = -1: every rank receives); a rank's packed block lives in `mine` until barrier B, and is then overwritten (what
// comm_scratch.ensure may do), so a copy made after a peer's barrier B would read garbage
std::string gather(LocalGroup& g, int rank, std::vector<Tuple>& mine, int dst, std::vector<Tuple>* recv, std::vector<long long>* counts) {
    std::vector<Hello> hello;
    std::string err = gather_hello(g, rank, Hello{(long long)mine.size(), 0, dst, 0}, &hello);
    if (!err.empty()) return err;
    for (int r = 0; r < g.world(); ++r)           // the engine's hello verdict: the same on every rank, before anything is posted
        if (hello[(size_t)r].dst != hello[0].dst) return "dst_rank not the same on every rank (rank " + std::to_string(r) + ")";
    std::vector<long long> off((size_t)g.world() + 1, 0);
    for (int r = 0; r < g.world(); ++r) off[(size_t)r + 1] = off[(size_t)r] + hello[(size_t)r].n;
    *counts = std::vector<long long>(off.size() - 1);
    for (int r = 0; r < g.world(); ++r) (*counts)[(size_t)r] = hello[(size_t)r].n;
    struct Post { unsigned long long ptr; long long n; int32_t ok, pad; };
    const Post p{(unsigned long long)(uintptr_t)mine.data(), (long long)mine.size(), 1, 0};
    std::vector<unsigned char> all;
    err = g.all_gather(rank, az::LOCAL_OP_GATHER_POST, 0, &p, sizeof p, &all);
    if (!err.empty()) return err;
    const bool receiver = dst < 0 || dst == rank;
    if (receiver) {
        recv->assign((size_t)off.back(), Tuple{});
        for (int r = 0; r < g.world(); ++r) {
            Post q;
            std::memcpy(&q, all.data() + (size_t)r * sizeof q, sizeof q);
            if (q.n > 0) std::memcpy(recv->data() + off[(size_t)r], (const void*)(uintptr_t)q.ptr, (size_t)q.n * sizeof(Tuple));
        }
    }
    const int32_t copied = 1;
    err = g.all_gather(rank, az::LOCAL_OP_GATHER_DONE, 0, &copied, sizeof copied, &all);
    std::fill(mine.begin(), mine.end(), Tuple{});          // the sender reuses its buffer
    return err;
}

// every rank's view of the run
struct Census {
    std::atomic<long> rounds{0}, wrong{0}, errors_expected{0}, errors_unexpected{0}, missing_error{0}, message_differs{0};
};

int mode_random(int world, int rounds, uint64_t seed) {
    az::LocalCommRegistry reg(1);
    unsigned char id[az::LOCAL_ID_BYTES];
    if (!reg.create(world, id).empty()) return 2;
    az::LocalId lid;
    if (!az::local_id_decode(id, &lid)) return 2;
    Census c;
    // round k: the error message each rank got ("" = none), to compare across ranks afterwards
    std::vector<std::vector<std::string>> msg((size_t)world, std::vector<std::string>((size_t)rounds));
    std::vector<std::thread> th;
    for (int rank = 0; rank < world; ++rank)
        th.emplace_back([&, rank] {
            std::mt19937_64 jitter(seed * 131 + (uint64_t)rank);
            std::this_thread::sleep_for(std::chrono::microseconds(jitter() % 500));
            std::shared_ptr<LocalGroup> g;
            if (!reg.join(lid, rank, world, rank % 2, &g).empty() || !g) { c.wrong += 1; return; }
            if ((int)g->devices().size() != world || g->devices()[(size_t)rank] != rank % 2) c.wrong += 1;
            std::mt19937_64 plan(seed);                 // the SAME sequence on every rank
            for (int k = 0; k < rounds; ++k) {
                const int op = (int)(plan() % 3);
                const int odd = (int)(plan() % 8) == 0 ? (int)(plan() % (uint64_t)world) : -1;   // the rank that mismatches, or -1
                const int kind = (int)(plan() % 2);      // mismatch: 0 = another collective, 1 = another n / dst
                const int n = (int)(plan() % 65);
                const int dst = (int)(plan() % (uint64_t)(world + 1)) - 1;
                if (jitter() % 4 == 0) std::this_thread::sleep_for(std::chrono::microseconds(jitter() % 200));
                std::string err;
                const bool me_odd = rank == odd;
                int my_op = op;
                if (me_odd && kind == 0) my_op = op == 1 ? 0 : 1;
                if (my_op == 0 || my_op == 2) {                 // u64 sum (op 2: the arena's 3 counters)
                    const int nn = my_op == 2 ? 3 : (me_odd && kind == 1 ? (n + 1) % 65 : n);
                    std::vector<uint64_t> v((size_t)std::max(nn, 1));
                    for (int i = 0; i < nn; ++i) v[(size_t)i] = mix((uint64_t)k * 1000003 + (uint64_t)rank * 64 + (uint64_t)i);
                    err = sum_u64(*g, rank, v.data(), nn);
                    if (err.empty())
                        for (int i = 0; i < nn; ++i) {
                            uint64_t want = 0;
                            for (int r = 0; r < world; ++r) want += mix((uint64_t)k * 1000003 + (uint64_t)r * 64 + (uint64_t)i);
                            if (v[(size_t)i] != want) c.wrong += 1;
                        }
                } else {                                        // a gather of ragged counts (rank r: (k + r * 7) % 23, 0 included)
                    const long long cnt = (k + rank * 7) % 23;
                    std::vector<Tuple> mine((size_t)cnt);
                    for (long long i = 0; i < cnt; ++i) mine[(size_t)i] = tuple_of(rank, (uint64_t)k, i);
                    // a different dst on the odd rank makes the hello verdict fail on every rank (as the engine's does)
                    const int my_dst = me_odd && kind == 1 ? (dst + 2) % (world + 1) - 1 : dst;
                    std::vector<Tuple> recv;
                    std::vector<long long> counts;
                    err = gather(*g, rank, mine, my_dst, &recv, &counts);
                    if (err.empty()) {
                        for (int r = 0; r < world; ++r) if (counts[(size_t)r] != (k + r * 7) % 23) c.wrong += 1;
                        if (dst < 0 || dst == rank) {
                            size_t at = 0;
                            for (int r = 0; r < world; ++r)
                                for (long long i = 0; i < (k + r * 7) % 23; ++i, ++at) {
                                    const Tuple t = tuple_of(r, (uint64_t)k, i);
                                    if (at >= recv.size() || std::memcmp(&recv[at], &t, sizeof t) != 0) c.wrong += 1;
                                }
                            if (at != recv.size()) c.wrong += 1;
                        }
                    }
                }
                const bool should_fail = odd >= 0 && !(kind == 1 && op == 2);   // op 2 always passes n = 3: no mismatch there
                if (!err.empty() && should_fail) c.errors_expected += 1;
                if (!err.empty() && !should_fail) c.errors_unexpected += 1;
                if (err.empty() && should_fail) c.missing_error += 1;
                msg[(size_t)rank][(size_t)k] = err;
                c.rounds += 1;
            }
            g->leave(rank);
        });
    for (auto& t : th) t.join();
    for (int k = 0; k < rounds; ++k)
        for (int r = 1; r < world; ++r)
            if (msg[(size_t)r][(size_t)k] != msg[0][(size_t)k]) c.message_differs += 1;
    std::printf("{\"world\": %d, \"rounds\": %ld, \"wrong\": %ld, \"errors_expected\": %ld, \"errors_unexpected\": %ld, "
                "\"missing_error\": %ld, \"message_differs\": %ld}\n",
                world, c.rounds.load(), c.wrong.load(), c.errors_expected.load(), c.errors_unexpected.load(), c.missing_error.load(),
                c.message_differs.load());
    return 0;
}

int mode_leave(int world) {
    az::LocalCommRegistry reg(1);
    unsigned char id[az::LOCAL_ID_BYTES];
    reg.create(world, id);
    az::LocalId lid;
    az::local_id_decode(id, &lid);
    std::atomic<int> in_wait{0}, woken{0}, later_failed{0}, ok_before{0};
    std::vector<std::string> msg((size_t)world);
    std::vector<std::thread> th;
    for (int rank = 0; rank < world; ++rank)
        th.emplace_back([&, rank] {
            std::shared_ptr<LocalGroup> g;
            if (!reg.join(lid, rank, world, 0, &g).empty()) return;
            uint64_t v[3] = {1, 2, 3};
            if (sum_u64(*g, rank, v, 3).empty() && v[0] == (uint64_t)world) ok_before += 1;      // one good round first
            if (rank == world - 1) {
                while (in_wait.load() < world - 1) std::this_thread::sleep_for(std::chrono::milliseconds(1));
                std::this_thread::sleep_for(std::chrono::milliseconds(50));    // the others are blocked in the round by now
                g->leave(rank);
                return;
            }
            in_wait += 1;
            std::vector<Tuple> mine(5, tuple_of(rank, 0, 0)), recv;
            std::vector<long long> counts;
            msg[(size_t)rank] = gather(*g, rank, mine, -1, &recv, &counts);
            if (!msg[(size_t)rank].empty()) woken += 1;
            if (!sum_u64(*g, rank, v, 3).empty()) later_failed += 1;
        });
    for (auto& t : th) t.join();
    int differs = 0;
    for (int r = 1; r + 1 < world; ++r) differs += msg[(size_t)r] != msg[0];
    const bool names = msg[0].find("rank " + std::to_string(world - 1) + " left") != std::string::npos;
    std::printf("{\"ok_before\": %d, \"woken\": %d, \"later_failed\": %d, \"message_differs\": %d, \"names_the_rank\": %s}\n", ok_before.load(),
                woken.load(), later_failed.load(), differs, names ? "true" : "false");
    return 0;
}

int mode_ids() {
    az::LocalCommRegistry reg(7);
    unsigned char id[az::LOCAL_ID_BYTES];
    int refused = 0, accepted = 0;
    std::string e;
    if (!reg.create(0, id).empty()) refused += 1;                 // world 0
    reg.create(2, id);
    az::LocalId lid;
    const bool decoded = az::local_id_decode(id, &lid) && lid.world == 2 && lid.serial == 1 && lid.pid == 7;
    unsigned char other[az::LOCAL_ID_BYTES] = {1, 2, 3};
    az::LocalId junk;
    const bool rccl_like_rejected = !az::local_id_decode(other, &junk);
    std::shared_ptr<LocalGroup> g0, g1, gx;
    if (!reg.join(lid, 0, 3, 0, &gx).empty()) refused += 1;       // world differs from the id's
    std::thread t0([&] { if (reg.join(lid, 0, 2, 0, &g0).empty()) accepted += 0; });
    std::this_thread::sleep_for(std::chrono::milliseconds(20));
    std::string taken = reg.join(lid, 0, 2, 0, &gx);              // rank 0 is taken (rank 0's join is still waiting for rank 1)
    if (!taken.empty()) refused += 1;
    if (reg.join(lid, 1, 2, 0, &g1).empty()) accepted += 1;
    t0.join();
    if (g0 && g1 && g0.get() == g1.get()) accepted += 1;
    std::string complete = reg.join(lid, 1, 2, 0, &gx);           // the world is complete: the id is spent
    if (!complete.empty()) refused += 1;
    az::LocalId unknown = lid;
    unknown.serial = 99;
    if (!reg.join(unknown, 0, 2, 0, &gx).empty()) refused += 1;
    az::LocalId foreign = lid;
    foreign.pid = 8;
    if (!reg.join(foreign, 0, 2, 0, &gx).empty()) refused += 1;
    std::printf("{\"refused\": %d, \"accepted\": %d, \"decoded\": %s, \"rccl_like_rejected\": %s, \"complete_msg\": \"%s\"}\n", refused,
                accepted, decoded ? "true" : "false", rccl_like_rejected ? "true" : "false", complete.c_str());
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "random";
    std::thread([] {
        std::this_thread::sleep_for(std::chrono::seconds(120));
        std::fprintf(stderr, "watchdog: deadlock\n");
        std::fflush(stderr);
        std::_Exit(3);
    }).detach();
    if (mode == "random")
        return mode_random(argc > 2 ? std::atoi(argv[2]) : 4, argc > 3 ? std::atoi(argv[3]) : 500,
                           argc > 4 ? std::strtoull(argv[4], nullptr, 10) : 1);
    if (mode == "leave") return mode_leave(argc > 2 ? std::atoi(argv[2]) : 3);
    if (mode == "ids") return mode_ids();
    return 2;
}
