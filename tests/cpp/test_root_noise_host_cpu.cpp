// CPU-only check that the C++ host (include/az_host.hpp) forwards root noise: Engine::set_root_noise sends the two options, and
// Coach::learn sets them around az_selfplay only -- on before the episodes, off again before training and the arena.  The engine ABI is
// replaced by a recording fake defined here, so nothing references libaz_engine.so (g++ alone builds it).
#include <cstdio>
#include <cstdlib>
#include <filesystem>
#include <string>
#include <vector>

#include "az_host.hpp"

static std::vector<std::string> g_calls;
struct az_engine { int dummy; };

extern "C" {
az_status az_create(const az_config*, az_engine** out) { static az_engine e; *out = &e; return AZ_OK; }
void az_destroy(az_engine*) {}
const char* az_last_error(const az_engine*) { return "fake"; }
az_status az_set_option(az_engine*, const char* key, int64_t value) {
    g_calls.push_back(std::string(key) + "=" + std::to_string((long long)value));
    return AZ_OK;
}
az_status az_selfplay(az_engine*, const az_selfplay_params* p, az_samples* out) {
    g_calls.push_back("selfplay");
    out->count = 2;                                       // one ply, both symmetries: enough for Coach::learn to go on
    for (int i = 0; i < 2 * 84; ++i) out->boards[i] = 0.0f;
    for (int i = 0; i < 2 * 7; ++i) out->pis[i] = 1.0f / 7.0f;
    out->zs[0] = out->zs[1] = 1.0f;
    (void)p;
    return AZ_OK;
}
az_status az_net_save(az_engine*, int32_t, const char*) { return AZ_OK; }
az_status az_net_load(az_engine*, int32_t, const char*) { return AZ_OK; }
az_status az_net_free(az_engine*, int32_t) { return AZ_OK; }
az_status az_net_set_class(az_engine*, int32_t, int32_t) { return AZ_OK; }
az_status az_net_train(az_engine*, int32_t, int32_t, const float*, const float*, const float*, int64_t) { g_calls.push_back("train"); return AZ_OK; }
int32_t az_net_train_history(const az_engine*, float*, int32_t) { return 0; }
az_status az_arena(az_engine*, const az_arena_params*, uint64_t out_wld[3], int8_t*) {
    g_calls.push_back("arena");
    out_wld[0] = 1; out_wld[1] = 0; out_wld[2] = 0;
    return AZ_OK;
}
az_status az_gather_samples(az_engine*, const az_samples*, int32_t, az_samples*, int64_t*) { return AZ_ERR_UNSUPPORTED; }
}

static int fail(const char* what) {
    std::printf("FAILED: %s\ncalls:", what);
    for (auto& c : g_calls) std::printf(" %s", c.c_str());
    std::printf("\n");
    return 1;
}

int main(int argc, char** argv) {
    using namespace az_host;
    Engine e(0, 64, 128);
    e.set_root_noise(0.25, 0.3);
    if (g_calls != std::vector<std::string>{"root_noise_alpha_e6=300000", "root_noise_eps_e6=250000"}) return fail("Engine::set_root_noise");
    if (argc < 2) return fail("usage: test_root_noise_host_cpu <scratch directory>");
    const std::string dir = argv[1];
    int rc = 0;
    for (int on = 1; on >= 0 && rc == 0; --on) {
        g_calls.clear();
        std::filesystem::remove_all(dir);
        Coach c = Coach::setup(e, dir, 1000, 0.55f, 15, 3, 100000, 1, 4, 2, 1, 2, 5, 1, 1000, 1);
        if (on) { c.root_noise_eps = 0.25; c.root_noise_alpha = 1.4; }
        c.learn(false, 3);
        std::vector<std::string> want;
        if (on) { want.push_back("root_noise_alpha_e6=1400000"); want.push_back("root_noise_eps_e6=250000"); }
        want.push_back("selfplay");
        if (on) { want.push_back("root_noise_alpha_e6=1400000"); want.push_back("root_noise_eps_e6=0"); }
        want.push_back("train_seed=3"); want.push_back("train"); want.push_back("arena");
        if (g_calls != want) rc = fail(on ? "Coach::learn with root noise" : "Coach::learn without root noise");
    }
    std::filesystem::remove_all(dir);
    if (rc == 0) std::printf("ok\n");
    return rc;
}
