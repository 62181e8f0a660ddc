// az_local_comm.h -- the rendezvous of the IN-PROCESS communicator (az_comm_local_id): the ranks of a world are engines of one
// process, each driven by its own host thread, and the collectives of the sharded Coach loop (az_gather_samples, az_allreduce_u64)
// meet here instead of in RCCL.  The reference is one process (src/coach.rs:241-272 fans episodes out over a rayon pool); this is
// what lets such a host keep its one process and still make one world out of one engine per GPU.
//
// No HIP here: the engine (az_engine.hip) builds its three backend primitives -- the all-gather of a host record, the u64 sum and
// the two barriers around the exchange of packed tuples -- on LocalGroup::all_gather, and tests/test_comm_local_cpu.py drives the
// same calls from 2..8 threads under ThreadSanitizer with host data only.
//
// Rules
//   - An id (128 bytes) = a magic prefix, a process-unique serial, the world size and the process id.  LocalCommRegistry::create
//     issues it; join(serial, world, rank) returns once all `world` ranks have joined (as ncclCommInitRank does).  Refused at once,
//     with a message: a world that differs from the id's, a rank outside it or already taken, an id whose world is already complete
//     (ids are never reused), an unknown serial, an id of another process.
//   - A collective is ONE round: every rank posts (op, n, record); the last rank to arrive decides the round's verdict from all the
//     posts -- the same op and the same n on every rank, else every rank gets the same error naming the ranks -- and wakes the others.
//     Rounds are numbered (generations); round g keeps its records in buffer g & 1, which round g + 2 may only overwrite once every
//     rank has arrived at g + 1, i.e. has read round g.
//   - leave(rank) (az_comm_destroy / az_destroy of a member): the group is broken for good.  Ranks waiting in a round that cannot
//     complete any more are woken with an error naming the ranks that left, and every later round fails at once.  A round that had
//     already completed still returns its result.
//   - A rank that never arrives is waited for (as with RCCL); there is no timeout.
#pragma once
#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

namespace az {

constexpr size_t LOCAL_ID_BYTES = 128;
constexpr unsigned char LOCAL_ID_MAGIC[16] = {'a', 'z', '-', 'l', 'o', 'c', 'a', 'l', '-', 'c', 'o', 'm', 'm', '-', 'v', '1'};

struct LocalId {
    uint64_t serial = 0;
    int32_t world = 0;
    int64_t pid = 0;
};
// [0, 16) magic, [16, 24) serial, [24, 28) world, [32, 40) pid, the rest zero
inline void local_id_encode(const LocalId& id, unsigned char out[LOCAL_ID_BYTES]) {
    std::memset(out, 0, LOCAL_ID_BYTES);
    std::memcpy(out, LOCAL_ID_MAGIC, sizeof LOCAL_ID_MAGIC);
    std::memcpy(out + 16, &id.serial, 8);
    std::memcpy(out + 24, &id.world, 4);
    std::memcpy(out + 32, &id.pid, 8);
}
// false: not an in-process id (an RCCL unique id, or garbage)
inline bool local_id_decode(const unsigned char in[LOCAL_ID_BYTES], LocalId* id) {
    if (std::memcmp(in, LOCAL_ID_MAGIC, sizeof LOCAL_ID_MAGIC) != 0) return false;
    std::memcpy(&id->serial, in + 16, 8);
    std::memcpy(&id->world, in + 24, 4);
    std::memcpy(&id->pid, in + 32, 8);
    return true;
}

// The collectives' steps, as posted to a round (a mismatch names them).
enum LocalOp : int32_t { LOCAL_OP_GATHER_HELLO = 1, LOCAL_OP_GATHER_POST = 2, LOCAL_OP_GATHER_DONE = 3, LOCAL_OP_ALLREDUCE = 4 };
inline const char* local_op_name(int32_t op) {
    switch (op) {
        case LOCAL_OP_GATHER_HELLO: return "az_gather_samples";
        case LOCAL_OP_GATHER_POST: return "az_gather_samples (exchange)";
        case LOCAL_OP_GATHER_DONE: return "az_gather_samples (copies done)";
        case LOCAL_OP_ALLREDUCE: return "az_allreduce_u64";
        default: return "an unknown collective";
    }
}

class LocalGroup {
  public:
    LocalGroup(uint64_t serial, int world) : serial_(serial), world_(world), joined_((size_t)world, 0), device_((size_t)world, -1),
                                             left_((size_t)world, 0) {
        for (auto& r : round_) r.post.resize((size_t)world);
    }
    int world() const { return world_; }
    uint64_t serial() const { return serial_; }

    // the HIP device each rank joined with (valid once join has returned)
    std::vector<int> devices() {
        std::lock_guard<std::mutex> lk(mu_);
        return device_;
    }

    // One round.  Posts (op, n, bytes of `rec`) for `rank` and blocks until every rank has posted (or a rank left).  Returns "" and
    // fills `all` with the world's records in rank order (world x bytes), or the round's error -- the same string on every rank.
    std::string all_gather(int rank, int32_t op, int64_t n, const void* rec, size_t bytes, std::vector<unsigned char>* all) {
        std::unique_lock<std::mutex> lk(mu_);
        if (broken_) return left_message_locked();
        const uint64_t g = done_;
        Round& r = round_[g & 1];
        Post& p = r.post[(size_t)rank];
        p.op = op;
        p.n = n;
        p.data.assign((const unsigned char*)rec, (const unsigned char*)rec + bytes);
        if (++arrived_ == world_) {
            r.verdict = verdict_locked(r);
            arrived_ = 0;
            ++done_;
            cv_.notify_all();
        } else {
            cv_.wait(lk, [&] { return done_ > g || broken_; });
            if (done_ == g) return left_message_locked();       // the round can never complete
        }
        if (!r.verdict.empty()) return r.verdict;
        all->resize((size_t)world_ * bytes);
        for (int q = 0; q < world_; ++q) std::memcpy(all->data() + (size_t)q * bytes, r.post[(size_t)q].data.data(), bytes);
        return std::string();
    }

    // az_comm_destroy / az_destroy of a member: the group is broken; waiters are woken
    void leave(int rank) {
        std::lock_guard<std::mutex> lk(mu_);
        if (rank < 0 || rank >= world_ || left_[(size_t)rank]) return;
        left_[(size_t)rank] = 1;
        broken_ = true;
        cv_.notify_all();
    }

  private:
    friend class LocalCommRegistry;
    struct Post { int32_t op = 0; int64_t n = 0; std::vector<unsigned char> data; };
    struct Round { std::vector<Post> post; std::string verdict; };

    std::string verdict_locked(const Round& r) const {
        bool same_op = true, same_n = true, same_bytes = true;
        for (const Post& p : r.post) {
            same_op = same_op && p.op == r.post[0].op;
            same_n = same_n && p.n == r.post[0].n;
            same_bytes = same_bytes && p.data.size() == r.post[0].data.size();
        }
        if (same_op && same_n && same_bytes) return std::string();
        std::string m = same_op ? std::string(local_op_name(r.post[0].op)) + " with a different n on the ranks of the in-process communicator:"
                                : std::string("mismatched collectives on the in-process communicator:");
        for (int q = 0; q < world_; ++q) {
            const Post& p = r.post[(size_t)q];
            m += (q ? ", rank " : " rank ") + std::to_string(q) + " in " + local_op_name(p.op);
            if (p.op == LOCAL_OP_ALLREDUCE) m += " (n = " + std::to_string(p.n) + ")";
        }
        return m;
    }
    std::string left_message_locked() const {
        std::string who;
        for (int q = 0; q < world_; ++q)
            if (left_[(size_t)q]) who += (who.empty() ? "" : ", ") + std::to_string(q);
        return "in-process communicator: rank " + who + " left (az_comm_destroy / az_destroy); every rank must call az_comm_destroy";
    }

    const uint64_t serial_;
    const int world_;
    std::mutex mu_;
    std::condition_variable cv_;
    // membership (join)
    std::vector<uint8_t> joined_;
    std::vector<int> device_;
    int n_joined_ = 0;
    // rounds
    Round round_[2];
    uint64_t done_ = 0;      // completed rounds; the round being posted to is done_
    int arrived_ = 0;
    std::vector<uint8_t> left_;
    bool broken_ = false;
};

// The process's in-process ids.  A group lives in the registry from create() until its world is complete; the members hold it
// from then on (shared_ptr), so serials are never looked up again.
class LocalCommRegistry {
  public:
    explicit LocalCommRegistry(int64_t pid) : pid_(pid) {}

    // "" and the id, or why not
    std::string create(int world, unsigned char id[LOCAL_ID_BYTES]) {
        if (world < 1) return "az_comm_local_id: world must be at least 1";
        std::lock_guard<std::mutex> lk(mu_);
        const uint64_t serial = ++last_serial_;
        pending_[serial] = std::make_shared<LocalGroup>(serial, world);
        local_id_encode(LocalId{serial, world, pid_}, id);
        return std::string();
    }

    // Joins `rank` (on HIP device `device`) and blocks until the world is complete.  "" and the group, or why it was refused at once.
    std::string join(const LocalId& id, int rank, int world, int device, std::shared_ptr<LocalGroup>* out) {
        std::shared_ptr<LocalGroup> grp;
        {
            std::lock_guard<std::mutex> lk(mu_);
            if (id.pid != pid_) return "az_comm_init: an in-process id of another process";
            auto it = pending_.find(id.serial);
            if (it == pending_.end()) {
                if (id.serial == 0 || id.serial > last_serial_) return "az_comm_init: unknown in-process id";
                return "az_comm_init: the in-process id's world is already complete (an id serves one world; make a new one)";
            }
            grp = it->second;
            if (world != grp->world_)
                return "az_comm_init: world " + std::to_string(world) + " differs from the in-process id's " + std::to_string(grp->world_);
            if (rank < 0 || rank >= world) return "az_comm_init: bad rank / world";
            std::lock_guard<std::mutex> gk(grp->mu_);
            if (grp->joined_[(size_t)rank]) return "az_comm_init: rank " + std::to_string(rank) + " of the in-process id is already taken";
            grp->joined_[(size_t)rank] = 1;
            grp->device_[(size_t)rank] = device;
            if (++grp->n_joined_ == grp->world_) {
                pending_.erase(it);           // complete: the id is spent
                grp->cv_.notify_all();
            }
        }
        std::unique_lock<std::mutex> gk(grp->mu_);
        grp->cv_.wait(gk, [&] { return grp->n_joined_ == grp->world_; });
        *out = grp;
        return std::string();
    }

  private:
    const int64_t pid_;
    std::mutex mu_;
    uint64_t last_serial_ = 0;
    std::map<uint64_t, std::shared_ptr<LocalGroup>> pending_;
};

}  // namespace az
