// test_coach_local.cpp -- az_host::Coach::shard at world > 1 in ONE process: test_coach.cpp's miniature (C = 128, 2 iterations, 48
// episodes, 25 sims, 16 arena games) first unsharded under <dir>/plain, then as worlds of 2, 3 ... ranks under <dir>/w<world>, each
// rank an Engine of its own on device 0 driven by its own thread, joined by one in-process communicator (az_comm_local_id).  Every
// engine has the same options (engines of one device driven at once: "search_graph" 0 and "train_graph" 0).  Prints one JSON line:
// the per-iteration reports of the plain run and of every rank of every world, and the wall times; tests/test_comm_local_gpu.py
// compares them and the files.  Usage: test_coach_local <dir> <seed> <world>...
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <thread>
#include <vector>

#include "az_host.hpp"

using namespace az_host;

namespace {

std::string report_json(const std::vector<Coach::Report>& rep) {
    std::string s = "[";
    char buf[256];
    for (size_t i = 0; i < rep.size(); ++i) {
        const auto& r = rep[i];
        std::snprintf(buf, sizeof buf, "%s{\"iteration\": %zu, \"samples\": %zu, \"nwins\": %zu, \"pwins\": %zu, \"draws\": %zu, \"accepted\": %s, \"model_id\": %zu, \"losses\": [",
                      i ? ", " : "", r.iteration, r.samples, r.nwins, r.pwins, r.draws, r.accepted ? "true" : "false", r.model_id);
        s += buf;
        for (size_t k = 0; k < r.losses.size(); ++k) { std::snprintf(buf, sizeof buf, "%s%.9g", k ? ", " : "", r.losses[k]); s += buf; }
        s += "]}";
    }
    return s + "]";
}

// one rank (world 1 = the plain run, no communicator)
std::vector<Coach::Report> run_rank(const std::string& dir, uint64_t seed, int rank, int world, const uint8_t* id) {
    Engine e(0, 256, 128);
    e.check(az_set_option(e.raw(), "search_graph", 0));
    e.check(az_set_option(e.raw(), "train_graph", 0));
    e.check(az_set_option(e.raw(), "eval_cache_log2", 20));
    e.check(az_net_init_random(e.raw(), 0, 3));
    e.check(az_set_option(e.raw(), "train_epochs", 2));
    Coach coach = Coach::setup(e, dir, 1000000, 0.55f, 15, 3, 100000, 1, 64, 16, 2, 48, 25, 1, 1000, 1);
    if (world > 1) {        // after setup: az_comm_init returns once every rank has joined, so no rank writes before all have set up
        e.check(az_comm_init(e.raw(), rank, world, id));
        coach.shard(rank, world);
    }
    auto rep = coach.learn(false, seed);
    if (world > 1) e.check(az_comm_destroy(e.raw()));
    return rep;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 4) { std::fprintf(stderr, "usage: test_coach_local <dir> <seed> <world>...\n"); return 2; }
    std::thread([] {
        std::this_thread::sleep_for(std::chrono::seconds(400));
        std::fprintf(stderr, "watchdog: the run deadlocked\n");
        std::fflush(stderr);
        std::_Exit(3);
    }).detach();
    const std::string dir = argv[1];
    const uint64_t seed = std::strtoull(argv[2], nullptr, 10);
    try {
        std::string out = "{\"plain\": ";
        auto t0 = std::chrono::steady_clock::now();
        out += report_json(run_rank(dir + "/plain", seed, 0, 1, nullptr));
        out += ", \"seconds\": {\"1\": " + std::to_string(std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
        std::string worlds = "\"worlds\": {";
        for (int a = 3; a < argc; ++a) {
            const int world = std::atoi(argv[a]);
            uint8_t id[AZ_COMM_ID_BYTES];
            {
                Engine maker(0, 64, 128);
                maker.check(az_comm_local_id(maker.raw(), world, id));
            }
            std::vector<std::vector<Coach::Report>> rep((size_t)world);
            std::vector<std::string> err((size_t)world);
            t0 = std::chrono::steady_clock::now();
            std::vector<std::thread> th;
            for (int r = 0; r < world; ++r)
                th.emplace_back([&, r] {
                    try { rep[(size_t)r] = run_rank(dir + "/w" + std::to_string(world), seed, r, world, id); }
                    catch (const std::exception& ex) { err[(size_t)r] = ex.what(); }
                });
            for (auto& t : th) t.join();
            const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            for (int r = 0; r < world; ++r)
                if (!err[(size_t)r].empty()) { std::fprintf(stderr, "world %d rank %d panic: %s\n", world, r, err[(size_t)r].c_str()); return 1; }
            out += ", \"" + std::to_string(world) + "\": " + std::to_string(secs);
            worlds += std::string(a > 3 ? ", " : "") + "\"" + std::to_string(world) + "\": [";
            for (int r = 0; r < world; ++r) worlds += (r ? ", " : "") + report_json(rep[(size_t)r]);
            worlds += "]";
        }
        std::printf("%s}, %s}}\n", out.c_str(), worlds.c_str());
        return 0;
    } catch (const std::exception& ex) {
        std::fprintf(stderr, "panic: %s\n", ex.what());
        return 1;
    }
}
