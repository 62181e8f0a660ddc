// test_shared_tree.cpp -- the shared tree batch (az_tree_share) driven the way a threaded host drives it: N std::threads, each
// looping Coach::execute_episode (src/coach.rs:104-157) over an AsyncMcts on its own slot of one SharedMcts
// (include/az_host.hpp), episodes handed out from an atomic counter -- so which thread and slot plays an episode, and what shares
// its batches, changes from run to run.  Prints one JSON line; tests/test_shared_tree_gpu.py checks it.
//
//   hash  <threads> <slots> <episodes> <sims> <sim_threads> <window_us>   per-episode moves / tuple count / sums (oracle-checked)
//   conv  <threads> <episodes> <sims>            the same episodes through 1-game trees one at a time: moves and pi bit for bit
//   errors                                       one finished board in a batch fails only its own request
//   contract                                     refused calls and their statuses
//
// Every mode runs under a watchdog that exits non-zero (without aborting) if the run deadlocks.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "az_host.hpp"

using namespace az_host;

namespace {

struct EpisodeOut {
    std::vector<uint8_t> moves;
    std::vector<float> pis;     // every tuple's pi, in order (symmetries included)
    size_t samples = 0;
    double zsum = 0, pisum = 0;
};

EpisodeOut play(const AsyncMcts& m, size_t ep, uint64_t seed) {
    EpisodeOut o;
    auto samples = execute_episode(m, 15, ep, seed, &o.moves);
    o.samples = samples.size();
    for (auto& s : samples) {
        o.zsum += s.v;
        for (float p : s.pi) { o.pisum += p; o.pis.push_back(p); }
    }
    return o;
}

// N threads; each takes the next episode id, builds an AsyncMcts on a slot, plays it, releases the slot (AsyncMcts dies)
std::vector<EpisodeOut> play_shared(SharedMcts& sh, int threads, int episodes, uint64_t seed) {
    std::vector<EpisodeOut> out((size_t)episodes);
    std::atomic<int> next{0};
    std::vector<std::string> errors((size_t)threads);
    std::vector<std::thread> pool;
    for (int w = 0; w < threads; ++w)
        pool.emplace_back([&, w] {
            try {
                for (;;) {
                    const int ep = next.fetch_add(1);
                    if (ep >= episodes) break;
                    AsyncMcts m = sh.mcts();
                    out[(size_t)ep] = play(m, (size_t)ep, seed);
                }
            } catch (const std::exception& ex) { errors[(size_t)w] = ex.what(); }
        });
    for (auto& t : pool) t.join();
    for (auto& e : errors) if (!e.empty()) throw Panic("worker: " + e);
    return out;
}

void print_stats(const SharedMcts& sh) {
    const auto s = sh.stats();
    std::printf("\"share_stats\": [%llu, %llu, %llu, %llu]", (unsigned long long)s[0], (unsigned long long)s[1],
                (unsigned long long)s[2], (unsigned long long)s[3]);
}

int mode_hash(int argc, char** argv) {
    const int threads = argc > 2 ? std::atoi(argv[2]) : 64, slots = argc > 3 ? std::atoi(argv[3]) : 64;
    const int episodes = argc > 4 ? std::atoi(argv[4]) : 128, sims = argc > 5 ? std::atoi(argv[5]) : 25;
    const int sim_threads = argc > 6 ? std::atoi(argv[6]) : 1, window = argc > 7 ? std::atoi(argv[7]) : 0;
    Engine e(0, 256, 128);
    e.check(az_net_set_kind(e.raw(), 10, AZ_NET_HASH, 1234));
    SharedMcts sh(e, (size_t)slots, 1000000, (size_t)sims, (size_t)sim_threads, 1000, 10, 1, window);
    const auto out = play_shared(sh, threads, episodes, 17);
    std::printf("{\"episodes\": [");
    for (int ep = 0; ep < episodes; ++ep) {
        const EpisodeOut& o = out[(size_t)ep];
        std::printf("%s{\"moves\": [", ep ? ", " : "");
        for (size_t i = 0; i < o.moves.size(); ++i) std::printf("%s%d", i ? "," : "", o.moves[i]);
        std::printf("], \"samples\": %zu, \"zsum\": %.9g, \"pisum\": %.9g}", o.samples, o.zsum, o.pisum);
    }
    std::printf("], ");
    print_stats(sh);
    std::printf("}\n");
    return 0;
}

int mode_conv(int argc, char** argv) {
    const int threads = argc > 2 ? std::atoi(argv[2]) : 64, episodes = argc > 3 ? std::atoi(argv[3]) : 64;
    const int sims = argc > 4 ? std::atoi(argv[4]) : 25;
    Engine e(0, 256, 512);
    e.check(az_net_init_random(e.raw(), 1, 3));
    std::vector<EpisodeOut> shared;
    std::array<uint64_t, 4> st{};
    {
        SharedMcts sh(e, (size_t)threads, 1000000, (size_t)sims, 1, 1000, 1, 1, 0);
        shared = play_shared(sh, threads, episodes, 5);
        st = sh.stats();
    }
    // today's path: the same episode ids one at a time, each on its own 1-game az_tree
    int moves_bad = 0, pi_bad = 0;
    size_t moves = 0;
    for (int ep = 0; ep < episodes; ++ep) {
        AsyncMcts m = AsyncMcts::default_(e, 1000000, (size_t)sims, 1, 1000, 1, 1);
        const EpisodeOut one = play(m, (size_t)ep, 5);
        const EpisodeOut& sh = shared[(size_t)ep];
        moves += one.moves.size();
        if (one.moves != sh.moves) ++moves_bad;
        if (one.pis.size() != sh.pis.size() || std::memcmp(one.pis.data(), sh.pis.data(), one.pis.size() * sizeof(float)) != 0) ++pi_bad;
    }
    std::printf("{\"episodes\": %d, \"moves\": %zu, \"moves_mismatch\": %d, \"pi_mismatch\": %d, \"share_stats\": [%llu, %llu, %llu, %llu]}\n",
                episodes, moves, moves_bad, pi_bad, (unsigned long long)st[0], (unsigned long long)st[1], (unsigned long long)st[2],
                (unsigned long long)st[3]);
    return 0;
}

// K threads, one request each, all in ONE batch (window 0: the batch starts when every held slot waits).  Thread 0's board may be
// a finished game; the others' results must not notice.
struct ErrRun { std::vector<int> status; std::vector<std::string> msg; std::vector<std::array<float, 7>> pi; std::vector<std::array<uint16_t, 7>> counts; uint64_t batches = 0; };

// request i plays boards[i] with the temperature and RNG stream of position ids[i]
ErrRun err_run(Engine& e, const std::vector<std::array<uint64_t, 2>>& boards, const std::vector<int>& ids) {
    const int K = (int)boards.size();
    az_tree* t = nullptr;
    e.check(az_tree_create(e.raw(), K, 1000000, 25, 1, 1000, 1, 1, &t));
    e.check(az_tree_share(t, 0));
    ErrRun r;
    r.status.assign((size_t)K, -1); r.msg.resize((size_t)K); r.pi.resize((size_t)K); r.counts.resize((size_t)K);
    std::vector<int32_t> slot((size_t)K, -1);
    for (int i = 0; i < K; ++i) if (az_tree_slot_acquire(t, &slot[(size_t)i]) != AZ_OK) throw Panic("acquire");
    std::vector<std::thread> pool;
    for (int i = 0; i < K; ++i)
        pool.emplace_back([&, i] {
            const int rc = az_tree_slot_get_action_prob(t, slot[(size_t)i], boards[(size_t)i].data(), ids[(size_t)i] % 2 ? 1.0f : 0.0f, 9,
                                                        100 + (uint64_t)ids[(size_t)i],
                                                        r.pi[(size_t)i].data(), r.counts[(size_t)i].data(), nullptr);
            r.status[(size_t)i] = rc;
            r.msg[(size_t)i] = az_tree_slot_error(t, slot[(size_t)i]);
        });
    for (auto& th : pool) th.join();
    uint64_t s[4];
    e.check(az_tree_share_stats(t, s));
    r.batches = s[0];
    for (int i = 0; i < K; ++i) az_tree_slot_release(t, slot[(size_t)i]);
    az_tree_destroy(t);
    return r;
}

int mode_errors() {
    Engine e(0, 256, 512);
    e.check(az_net_init_random(e.raw(), 1, 3));
    // 8 positions a few plies deep (canonical: side to move first), thread 0's is a finished game
    std::vector<std::array<uint64_t, 2>> boards;
    for (int i = 0; i < 8; ++i) {
        ConnectFourGame b = ConnectFourGame::get_init_board();
        int8_t pl = 1;
        for (int k = 0; k < 1 + i % 4; ++k) { auto nx = b.get_next_state(pl, (uint8_t)((i + 3 * k) % 7)); b = nx.first; pl = nx.second; }
        const ConnectFourGame c = b.get_canonical_form(pl);
        boards.push_back({c.plus, c.minus});
    }
    ConnectFourGame fin = ConnectFourGame::get_init_board();
    int8_t pl = 1;
    for (uint8_t a : {0, 1, 0, 1, 0, 1, 0}) { auto nx = fin.get_next_state(pl, a); fin = nx.first; pl = nx.second; }
    const ConnectFourGame fc = fin.get_canonical_form(pl);
    std::vector<std::array<uint64_t, 2>> with = boards;
    with[0] = {fc.plus, fc.minus};
    std::vector<int> ids;
    for (int i = 0; i < 8; ++i) ids.push_back(i);
    const ErrRun a = err_run(e, with, ids);
    const ErrRun b = err_run(e, std::vector<std::array<uint64_t, 2>>(boards.begin() + 1, boards.end()),
                             std::vector<int>(ids.begin() + 1, ids.end()));     // the run without it
    int same = 0, ok = 0;
    for (size_t i = 1; i < boards.size(); ++i) {
        ok += a.status[i] == AZ_OK && b.status[i - 1] == AZ_OK;
        same += std::memcmp(a.pi[i].data(), b.pi[i - 1].data(), sizeof a.pi[i]) == 0 && a.counts[i] == b.counts[i - 1];
    }
    std::printf("{\"terminal_status\": %d, \"terminal_msg_len\": %zu, \"others_ok\": %d, \"others_identical\": %d, \"others\": %zu, "
                "\"batches\": %llu}\n", a.status[0], a.msg[0].size(), ok, same, boards.size() - 1, (unsigned long long)a.batches);
    return 0;
}

int mode_contract() {
    Engine e(0, 256, 128);
    e.check(az_net_set_kind(e.raw(), 10, AZ_NET_HASH, 1234));
    const int G = 4;
    az_tree* plain = nullptr;
    e.check(az_tree_create(e.raw(), G, 100000, 8, 1, 1000, 10, 1, &plain));
    int32_t s0 = -1;
    const int plain_acquire = az_tree_slot_acquire(plain, &s0);     // not shared
    az_tree* t = nullptr;
    e.check(az_tree_create(e.raw(), G, 100000, 8, 1, 1000, 10, 1, &t));
    e.check(az_tree_share(t, 0));
    const uint64_t init[2 * G] = {0, 0, 0, 0, 0, 0, 0, 0};
    float pi[7 * G];
    const int gap = az_tree_get_action_prob(t, init, 1.0f, 0, 0, pi, nullptr, nullptr);
    const int reset = az_tree_reset(t, nullptr);
    std::vector<int32_t> slots;
    int acq_rc = AZ_OK;
    for (int i = 0; i < G; ++i) { int32_t s = -1; acq_rc |= az_tree_slot_acquire(t, &s); slots.push_back(s); }
    int32_t extra = -1;
    const int over = az_tree_slot_acquire(t, &extra);
    const int out_of_range = az_tree_slot_get_action_prob(t, G, init, 1.0f, 0, 0, pi, nullptr, nullptr);
    const int negative = az_tree_slot_get_action_prob(t, -1, init, 1.0f, 0, 0, pi, nullptr, nullptr);
    // release every slot but the last; the last one's own call then runs alone (every held slot is waiting)
    for (int i = 0; i + 1 < G; ++i) e.check(az_tree_slot_release(t, slots[(size_t)i]));
    const int not_held = az_tree_slot_get_action_prob(t, slots[0], init, 1.0f, 0, 0, pi, nullptr, nullptr);
    const int double_release = az_tree_slot_release(t, slots[0]);
    const int release_range = az_tree_slot_release(t, G + 3);
    const int own = az_tree_slot_get_action_prob(t, slots[(size_t)G - 1], init, 1.0f, 0, 0, pi, nullptr, nullptr);
    float sum = 0.f;
    for (int a = 0; a < 7; ++a) sum += pi[a];
    e.check(az_tree_slot_release(t, slots[(size_t)G - 1]));
    az_tree_destroy(t);
    az_tree_destroy(plain);
    std::printf("{\"plain_acquire\": %d, \"get_action_prob\": %d, \"reset\": %d, \"acquire_all\": %d, \"slots\": [%d,%d,%d,%d], "
                "\"acquire_over\": %d, \"out_of_range\": %d, \"negative\": %d, \"not_held\": %d, \"double_release\": %d, "
                "\"release_range\": %d, \"own\": %d, \"own_pi_sum\": %.6f}\n",
                plain_acquire, gap, reset, acq_rc, slots[0], slots[1], slots[2], slots[3], over, out_of_range, negative, not_held,
                double_release, release_range, own, sum);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "hash";
    const int limit_s = std::getenv("AZ_TEST_WATCHDOG_S") ? std::atoi(std::getenv("AZ_TEST_WATCHDOG_S")) : 240;
    std::thread([limit_s] {                 // a deadlocked combiner ends as a failure, not a hang
        std::this_thread::sleep_for(std::chrono::seconds(limit_s));
        std::fprintf(stderr, "watchdog: no result after %d s\n", limit_s);
        std::fflush(stderr);
        std::_Exit(3);
    }).detach();
    try {
        if (mode == "hash") return mode_hash(argc, argv);
        if (mode == "conv") return mode_conv(argc, argv);
        if (mode == "errors") return mode_errors();
        if (mode == "contract") return mode_contract();
        std::fprintf(stderr, "unknown mode %s\n", mode.c_str());
        return 2;
    } catch (const std::exception& ex) {
        std::fprintf(stderr, "FAILED: %s\n", ex.what());
        return 1;
    }
}
