// test_combine_cpu.cpp -- the shared tree batch's request combiner (alphazero-rs_amd/csrc/az_combine.h) on the CPU with a fake
// batch runner, built with -fsanitize=thread by tests/test_shared_tree_cpu.py.  Prints one JSON line of counts; any violated rule
// is counted, never asserted, so the Python side sees every kind of failure at once.  A watchdog exits non-zero (without
// aborting) if the protocol deadlocks.
//
//   random  <threads> <slots> <rounds> <window_us>   threads acquire, submit, release and re-acquire slots at random
//   stall   <window_us>                              one thread holds a slot and never submits: only the window starts batches
//   release                                          waiters of a window-0 batch proceed once the stalled holder releases
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "az_combine.h"

namespace {

struct Req {
    uint64_t id = 0;          // what the caller asked
    uint64_t result = 0;      // what the runner answered
    int answers = 0;
};

uint64_t answer_of(uint64_t id, int slot) { return id * 0x9E3779B97F4A7C15ull ^ (uint64_t)slot; }

struct Census {
    std::atomic<long> batches{0}, dup_slot{0}, not_full{0}, runner_overlap{0}, by_window{0}, requests{0};
    std::atomic<int> in_runner{0};
    int window_us = 0;
};

struct FakeRunner {
    Census* c;
    void operator()(az::CombineBatch<Req>& b) const {
        if (c->in_runner.fetch_add(1) != 0) c->runner_overlap += 1;       // one leader at a time
        std::vector<int> seen;
        for (size_t i = 0; i < b.slots.size(); ++i) {
            for (int s : seen) if (s == b.slots[i]) c->dup_slot += 1;
            seen.push_back(b.slots[i]);
            b.reqs[i]->result = answer_of(b.reqs[i]->id, b.slots[i]);
            b.reqs[i]->answers += 1;
        }
        if (c->window_us == 0 && (int)b.slots.size() != b.held) c->not_full += 1;
        if (b.by_window) c->by_window += 1;
        c->batches += 1;
        c->requests += (long)b.slots.size();
        std::this_thread::sleep_for(std::chrono::microseconds(20));      // a batch takes a while: requests pile up behind it
        c->in_runner.fetch_sub(1);
    }
};
using Combiner = az::SlotCombiner<Req, FakeRunner>;

int mode_random(int threads, int slots, int rounds, int window_us) {
    Census c;
    c.window_us = window_us;
    Combiner comb(slots, FakeRunner{&c});
    comb.set_window_us(window_us);
    std::atomic<long> submitted{0}, wrong{0}, refused{0}, capacity{0};
    std::vector<std::thread> pool;
    for (int w = 0; w < threads; ++w)
        pool.emplace_back([&, w] {
            std::mt19937 rng((unsigned)w * 7919u + 1u);
            int slot = -1;
            for (int r = 0; r < rounds; ++r) {
                if (slot < 0) {
                    slot = comb.acquire();
                    if (slot < 0) { capacity += 1; std::this_thread::yield(); continue; }
                }
                Req q;
                q.id = ((uint64_t)w << 32) | (uint64_t)r;
                if (!comb.submit(slot, &q)) { refused += 1; continue; }
                submitted += 1;
                if (q.answers != 1 || q.result != answer_of(q.id, slot)) wrong += 1;
                if (rng() % 4 == 0) {                         // leave; maybe come back on another slot
                    if (!comb.release(slot)) refused += 1;
                    slot = -1;
                    if (rng() % 2) std::this_thread::sleep_for(std::chrono::microseconds(rng() % 50));
                }
            }
            if (slot >= 0 && !comb.release(slot)) refused += 1;
        });
    for (auto& t : pool) t.join();
    const az::CombineStats st = comb.stats();
    std::printf("{\"submitted\": %ld, \"wrong\": %ld, \"refused\": %ld, \"capacity\": %ld, \"batches\": %ld, \"requests\": %ld, "
                "\"dup_slot\": %ld, \"not_full\": %ld, \"runner_overlap\": %ld, \"by_window\": %ld, \"stats\": [%llu, %llu, %llu, %llu]}\n",
                submitted.load(), wrong.load(), refused.load(), capacity.load(), c.batches.load(), c.requests.load(), c.dup_slot.load(),
                c.not_full.load(), c.runner_overlap.load(), c.by_window.load(), (unsigned long long)st.batches,
                (unsigned long long)st.requests, (unsigned long long)st.largest, (unsigned long long)st.by_window);
    return 0;
}

// Thread 0 holds a slot and sleeps `stall_ms`; threads 1..3 submit `rounds` requests each.  With a window the three go on without
// it; returns when each worker finished relative to the stall's end.
int mode_stall(int window_us, bool release_at_end) {
    Census c;
    c.window_us = window_us;
    Combiner comb(4, FakeRunner{&c});
    comb.set_window_us(window_us);
    const int stall_ms = 300, rounds = 20;
    int held[4];
    for (int i = 0; i < 4; ++i) held[i] = comb.acquire();
    std::atomic<long> done_before{0}, done_after{0}, wrong{0};
    std::atomic<bool> stalled{true};
    std::vector<std::thread> pool;
    pool.emplace_back([&] {
        std::this_thread::sleep_for(std::chrono::milliseconds(stall_ms));
        stalled = false;
        if (release_at_end) comb.release(held[0]);           // a release wakes the waiters
        else {
            Req q; q.id = 99;
            if (!comb.submit(held[0], &q) || q.answers != 1) wrong += 1;
            comb.release(held[0]);
        }
    });
    for (int w = 1; w < 4; ++w)
        pool.emplace_back([&, w] {
            for (int r = 0; r < rounds; ++r) {
                Req q; q.id = (uint64_t)(w * 1000 + r);
                if (!comb.submit(held[w], &q) || q.answers != 1 || q.result != answer_of(q.id, held[w])) wrong += 1;
            }
            (stalled ? done_before : done_after) += 1;
            comb.release(held[w]);
        });
    for (auto& t : pool) t.join();
    std::printf("{\"done_before_stall_end\": %ld, \"done_after\": %ld, \"wrong\": %ld, \"batches\": %ld, \"by_window\": %ld, "
                "\"not_full\": %ld, \"dup_slot\": %ld}\n", done_before.load(), done_after.load(), wrong.load(), c.batches.load(),
                c.by_window.load(), c.not_full.load(), c.dup_slot.load());
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "random";
    std::thread([] {
        std::this_thread::sleep_for(std::chrono::seconds(100));
        std::fprintf(stderr, "watchdog: deadlock\n");
        std::fflush(stderr);
        std::_Exit(3);
    }).detach();
    if (mode == "random")
        return mode_random(argc > 2 ? std::atoi(argv[2]) : 64, argc > 3 ? std::atoi(argv[3]) : 48, argc > 4 ? std::atoi(argv[4]) : 200,
                           argc > 5 ? std::atoi(argv[5]) : 0);
    if (mode == "stall") return mode_stall(argc > 2 ? std::atoi(argv[2]) : 0, false);
    if (mode == "release") return mode_stall(0, true);
    return 2;
}
