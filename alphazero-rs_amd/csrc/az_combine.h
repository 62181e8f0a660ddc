// az_combine.h -- the request combiner of a SHARED tree batch (az_tree_share): many host threads, one per slot, each blocked in
// its own get_action_prob, fed into one batched search.  The reference's `inference_thread` (src/async_mcts.rs:117-189) gathers
// leaf boards from every episode thread and answers them with one predict once `batch_size` are waiting; here the unit is a
// whole get_action_prob and there is no library-owned thread: a waiting caller either becomes the batch's LEADER (it runs the
// batch for everybody) or sleeps on a condition variable until a leader has answered it.
//
// No HIP here: the batch runner is a template parameter, so the protocol is unit-tested on the CPU under ThreadSanitizer with a
// fake runner (tests/test_shared_tree_cpu.py).  The engine's runner (az_engine.hip) makes every HIP call of a batch; only one
// leader runs at a time, so the runner is the tree's one lock around the device.
//
// Rules
//   - A slot has at most one request in flight (its thread blocks in submit).
//   - window_us == 0: a batch starts when every HELD slot has a request waiting (the reference's batch_size rule with
//     batch_size = the threads that play); window_us > 0: also when the oldest waiting request is that old.
//   - release() of a slot wakes the waiters: a batch that waited for that slot may now start.
//   - A batch holds each slot at most once and every request is answered exactly once, by the runner of the batch it was
//     taken into.
#pragma once
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <mutex>
#include <vector>

namespace az {

struct CombineStats {
    uint64_t batches = 0, requests = 0, largest = 0, by_window = 0;
};

// One batch as the runner sees it.  reqs[i] is the request of slot slots[i]; reset[i] != 0: the slot was (re)acquired since its
// last batch, so its tree must be rebuilt first (AsyncMcts::default).  held = slots held when the batch started.
template <class Req>
struct CombineBatch {
    std::vector<int32_t> slots;
    std::vector<Req*> reqs;
    std::vector<uint8_t> reset;
    int held = 0;
    bool by_window = false;
};

// Runner: void(CombineBatch<Req>&), called with the combiner's mutex RELEASED, by one thread at a time; it answers every request of
// the batch (writes the results into them) before it returns.
template <class Req, class Runner>
class SlotCombiner {
  public:
    SlotCombiner(int slots, Runner runner) : runner_(runner), slot_(slots) {}

    void set_window_us(int64_t us) { std::lock_guard<std::mutex> lk(mu_); window_us_ = us; }
    int slots() const { return (int)slot_.size(); }

    // the lowest free slot, or -1 when all are held
    int acquire() {
        std::lock_guard<std::mutex> lk(mu_);
        for (int s = 0; s < (int)slot_.size(); ++s)
            if (!slot_[s].held) {
                slot_[s].held = true;
                slot_[s].fresh = true;
                ++held_;
                return s;
            }
        return -1;
    }
    // false: out of range or not held
    bool release(int s) {
        std::lock_guard<std::mutex> lk(mu_);
        if (!holds_locked(s) || slot_[s].req) return false;
        slot_[s].held = false;
        --held_;
        cv_.notify_all();
        return true;
    }
    bool holds(int s) {
        std::lock_guard<std::mutex> lk(mu_);
        return holds_locked(s);
    }

    // Blocks until the request has been answered.  false: the slot is out of range, not held, or already has a request in flight.
    bool submit(int s, Req* r) {
        std::unique_lock<std::mutex> lk(mu_);
        if (!holds_locked(s) || slot_[s].req) return false;
        Slot& me = slot_[s];
        me.req = r;
        me.done = false;
        me.since = Clock::now();
        pending_.push_back(s);
        // no notify here: if this request completes a batch, this thread sees it below and leads it.  (Waking every waiter on every
        // submit costs N^2 wake-ups per batch: with 256 threads that, not the device, set the pace.)
        for (;;) {
            if (me.done) {
                me.req = nullptr;
                return true;
            }
            bool by_window = false;
            if (!leading_ && ready_locked(Clock::now(), &by_window)) {
                lead_locked(lk, by_window);
                continue;
            }
            if (!leading_ && window_us_ > 0 && !pending_.empty()) {
                // sleep until the oldest request's window closes.  The deadline goes to the condition variable on the system clock
                // (pthread_cond_timedwait); readiness itself is judged on the steady clock above, so a clock step only moves a wake-up
                const auto left = slot_[pending_.front()].since + std::chrono::microseconds(window_us_) - Clock::now();
                cv_.wait_until(lk, std::chrono::system_clock::now() + std::chrono::duration_cast<std::chrono::system_clock::duration>(left));
            } else
                cv_.wait(lk);
        }
    }

    CombineStats stats() {
        std::lock_guard<std::mutex> lk(mu_);
        return stats_;
    }

  private:
    using Clock = std::chrono::steady_clock;
    struct Slot {
        bool held = false, fresh = false, done = false;
        Req* req = nullptr;
        Clock::time_point since{};
    };

    bool holds_locked(int s) const { return s >= 0 && s < (int)slot_.size() && slot_[s].held; }

    bool ready_locked(Clock::time_point now, bool* by_window) const {
        if (pending_.empty()) return false;
        if ((int)pending_.size() >= held_) return true;
        if (window_us_ > 0 && now - slot_[pending_.front()].since >= std::chrono::microseconds(window_us_)) {
            *by_window = true;
            return true;
        }
        return false;
    }

    // take every waiting request, run the batch with the mutex released, hand the answers out
    void lead_locked(std::unique_lock<std::mutex>& lk, bool by_window) {
        leading_ = true;
        CombineBatch<Req> b;
        b.held = held_;
        b.by_window = by_window;
        for (int s : pending_) {
            b.slots.push_back(s);
            b.reqs.push_back(slot_[s].req);
            b.reset.push_back(slot_[s].fresh ? 1 : 0);
            slot_[s].fresh = false;
        }
        pending_.clear();
        stats_.batches += 1;
        stats_.requests += b.slots.size();
        if (b.slots.size() > stats_.largest) stats_.largest = b.slots.size();
        if (by_window) stats_.by_window += 1;
        lk.unlock();
        runner_(b);
        lk.lock();
        for (int s : b.slots) slot_[s].done = true;
        leading_ = false;
        cv_.notify_all();
    }

    Runner runner_;
    std::mutex mu_;
    std::condition_variable cv_;
    std::vector<Slot> slot_;
    std::vector<int> pending_;      // slots with a request waiting, oldest first
    int held_ = 0;
    int64_t window_us_ = 0;
    bool leading_ = false;
    CombineStats stats_;
};

}  // namespace az
