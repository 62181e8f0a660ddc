// CPU-only check of the host-only paths of Coach::value_target_q / Coach::surprise_share (include/az_host.hpp): "selfplay_record_search"
// holds around az_selfplay only, the record is fetched, blended and resampled before the symmetry expansion, a world of 2 with
// surprise_share panics before the engine is asked, and with both fields 0 none of the new entries is called.  The engine ABI is replaced
// by a recording fake defined here, so nothing references libaz_engine.so (g++ alone builds it).
#include <cstdio>
#include <cstdlib>
#include <filesystem>
#include <string>
#include <vector>

#include "az_host.hpp"

static std::vector<std::string> g_calls;
static int64_t g_train_n = 0;
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
    g_calls.push_back(p->symmetries ? "selfplay(sym)" : "selfplay");
    const int n = p->symmetries ? 2 : 3;                  // the compact path: three plies of the initial board's line 3, 3, 3
    out->count = n;
    for (int i = 0; i < n; ++i) {
        if (out->states) { out->states[2 * i] = 0; out->states[2 * i + 1] = 0; }
        if (out->boards) for (int k = 0; k < 84; ++k) out->boards[i * 84 + k] = 0.0f;
        for (int k = 0; k < 7; ++k) out->pis[i * 7 + k] = 1.0f / 7.0f;
        out->zs[i] = 1.0f;
    }
    return AZ_OK;
}
az_status az_selfplay_get_search(az_engine*, float* root_q, float* root_prior) {
    g_calls.push_back("get_search");
    for (int i = 0; i < 3; ++i) { root_q[i] = 0.5f; for (int k = 0; k < 7; ++k) root_prior[i * 7 + k] = 1.0f / 7.0f; }
    return AZ_OK;
}
az_status az_samples_blend_z(az_engine*, int64_t n, const float* zs, const float* root_q, int64_t lambda_e6, float* zs_out) {
    g_calls.push_back("blend_z(" + std::to_string((long long)n) + "," + std::to_string((long long)lambda_e6) + ")");
    for (int64_t i = 0; i < n; ++i) zs_out[i] = 0.5f * (zs[i] + root_q[i]);
    return AZ_OK;
}
az_status az_samples_surprise(az_engine*, const az_samples* src, const float*, int64_t share_e6, uint64_t seed, az_samples* dst, uint32_t* counts, float* kl) {
    g_calls.push_back("surprise(" + std::to_string((long long)src->count) + "," + std::to_string((long long)share_e6) + "," + std::to_string((unsigned long long)seed) + ")");
    if (dst->capacity < 2 * src->count) return AZ_ERR_BAD_ARGUMENT;
    int64_t m = 0;
    for (int64_t i = 0; i < src->count; ++i) {             // tuple 0 twice, tuple 1 never, the others once
        const uint32_t c = i == 0 ? 2u : (i == 1 ? 0u : 1u);
        counts[i] = c; kl[i] = 0.0f;
        for (uint32_t k = 0; k < c; ++k, ++m) {
            dst->states[2 * m] = src->states[2 * i]; dst->states[2 * m + 1] = src->states[2 * i + 1];
            for (int a = 0; a < 7; ++a) dst->pis[m * 7 + a] = src->pis[i * 7 + a];
            dst->zs[m] = src->zs[i];
        }
    }
    dst->count = m;
    return AZ_OK;
}
az_status az_net_save(az_engine*, int32_t, const char*) { return AZ_OK; }
az_status az_net_load(az_engine*, int32_t, const char*) { return AZ_OK; }
az_status az_net_free(az_engine*, int32_t) { return AZ_OK; }
az_status az_net_set_class(az_engine*, int32_t, int32_t) { return AZ_OK; }
az_status az_net_train(az_engine*, int32_t, int32_t, const float*, const float*, const float* vs, int64_t n) {
    g_calls.push_back("train");
    g_train_n = n;
    for (int64_t i = 0; i < n; ++i) if (vs[i] != 0.75f && vs[i] != 1.0f) g_train_n = -1;
    return AZ_OK;
}
int32_t az_net_train_history(const az_engine*, float*, int32_t) { return 0; }
az_status az_arena(az_engine*, const az_arena_params*, uint64_t out_wld[3], int8_t*) {
    g_calls.push_back("arena");
    out_wld[0] = 1; out_wld[1] = 0; out_wld[2] = 0;
    return AZ_OK;
}
az_status az_gather_samples(az_engine*, const az_samples*, int32_t, az_samples*, int64_t*) { g_calls.push_back("gather"); return AZ_ERR_UNSUPPORTED; }
}

static int fail(const char* what) {
    std::printf("FAILED: %s\ncalls:", what);
    for (auto& c : g_calls) std::printf(" %s", c.c_str());
    std::printf("\n");
    return 1;
}

int main(int argc, char** argv) {
    using namespace az_host;
    if (argc < 2) return fail("usage: test_targets_host_cpu <scratch directory>");
    Engine e(0, 64, 128);
    const std::string dir = argv[1];
    using Calls = std::vector<std::string>;
    const Calls tail = {"train_seed=3", "train", "arena"};
    auto run = [&](double q, double share, int world) {
        g_calls.clear();
        g_train_n = 0;
        std::filesystem::remove_all(dir);
        Coach c = Coach::setup(e, dir, 1000, 0.55f, 15, 3, 100000, 1, 4, 2, 1, 2, 5, 1, 1000, 1);
        c.value_target_q = q; c.surprise_share = share;
        if (world > 1) c.shard(0, world);
        c.learn(false, 3);
    };
    auto with_tail = [&](Calls c) { c.insert(c.end(), tail.begin(), tail.end()); return c; };
    // both off: the path and the calls of a Coach without the fields
    run(0.0, 0.0, 1);
    if (g_calls != with_tail({"selfplay(sym)"}) || g_train_n != 2) return fail("both fields 0");
    // the blend alone: three compact tuples, z' = 0.75, both symmetries
    run(0.5, 0.0, 1);
    if (g_calls != with_tail({"selfplay_record_search=1", "selfplay", "selfplay_record_search=0", "get_search", "blend_z(3,500000)"}) || g_train_n != 6)
        return fail("value_target_q = 0.5");
    // both: the blend first, then the resampling (seed + iteration = 3) of the blended tuples: 2 + 0 + 1 copies, both symmetries
    run(0.5, 0.25, 1);
    if (g_calls != with_tail({"selfplay_record_search=1", "selfplay", "selfplay_record_search=0", "get_search", "blend_z(3,500000)", "surprise(3,250000,3)"}) ||
        g_train_n != 6)
        return fail("value_target_q = 0.5, surprise_share = 0.25");
    // a world of 2 with surprise_share panics before the engine is asked
    bool threw = false;
    try { run(0.0, 0.5, 2); } catch (const Panic&) { threw = true; }
    if (!threw || !g_calls.empty()) return fail("surprise_share with a world of 2");
    threw = false;
    try { run(1.5, 0.0, 1); } catch (const Panic&) { threw = true; }
    if (!threw || !g_calls.empty()) return fail("value_target_q outside 0 .. 1");
    std::filesystem::remove_all(dir);
    std::printf("ok\n");
    return 0;
}
