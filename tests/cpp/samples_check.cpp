// csrc/az_samples.h compiled alone by g++ and run as a stand-alone program under AddressSanitizer and UBSan (tests/test_samples_check_cpu.py):
// sample_check over a window on both routes with one fault of every class, Carve and sample_arrays_overlap.  Prints "ok".
// TEST INFRASTRUCTURE ONLY.  Build: g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I alphazero-rs_amd/csrc
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "az_samples.h"

#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

int main() {
    using namespace az;
    const int64_t n = 300;
    std::vector<SampleState> states((size_t)n);
    std::vector<float> boards((size_t)n * 84, 0.0f), pis((size_t)n * 7), zs((size_t)n);
    for (int64_t i = 0; i < n; ++i) {                 // column i % 7 holds i % 6 stones, alternating from the bottom
        uint64_t side[2] = {0, 0};
        for (int h = 0; h < (int)(i % 6); ++h) {
            const int c = (int)(i % 7);
            side[h & 1] |= 1ull << (c * 7 + h);
            boards[(size_t)i * 84 + (size_t)(h & 1) * 42 + (size_t)(5 - h) * 7 + c] = 1.0f;
        }
        states[(size_t)i] = SampleState{side[0], side[1]};
        for (int a = 0; a < 7; ++a) pis[(size_t)i * 7 + a] = a == (int)(i % 7) ? 0.4f : 0.1f;
        zs[(size_t)i] = (i & 1) ? 1.0f : -1.0f;
    }
    uint64_t mine = 0, theirs = 0;
    const SampleWindow by_states{states.data(), nullptr, pis.data(), zs.data()}, by_boards{nullptr, boards.data(), pis.data(), zs.data()};
    for (int strict = 0; strict < 2; ++strict)
        for (int64_t i = 0; i < n; ++i) {
            CHECK(sample_check(by_states, i, strict != 0, &mine, &theirs) == 0u);
            CHECK(mine == states[(size_t)i].x && theirs == states[(size_t)i].y);
            CHECK(sample_check(by_boards, i, strict != 0, &mine, &theirs) == 0u);
            CHECK(mine == states[(size_t)i].x && theirs == states[(size_t)i].y);
        }
    for (const int64_t at : {(int64_t)0, (int64_t)255, (int64_t)256, n - 1}) {
        const size_t k = (size_t)at;
        auto bits = [&](bool from_boards, bool strict) { return sample_check(from_boards ? by_boards : by_states, at, strict, &mine, &theirs); };
        float& p = pis[k * 7 + 3];
        const float p0 = p;
        p = NAN;   CHECK(bits(false, false) == SAMPLE_BAD_VALUE && bits(true, true) == SAMPLE_BAD_VALUE);
        p = 1.5f;  CHECK(bits(false, false) == SAMPLE_BAD_VALUE && bits(true, true) == SAMPLE_BAD_VALUE);
        p = -0.5f; CHECK(bits(false, false) == 0u && bits(true, false) == 0u && bits(false, true) == SAMPLE_BAD_VALUE && bits(true, true) == SAMPLE_BAD_VALUE);
        p = p0;
        const float z0 = zs[k];
        zs[k] = -1.5f; CHECK(bits(false, false) == SAMPLE_BAD_VALUE && bits(true, true) == SAMPLE_BAD_VALUE);
        zs[k] = NAN;   CHECK(bits(true, false) == SAMPLE_BAD_VALUE && bits(false, true) == SAMPLE_BAD_VALUE);
        zs[k] = z0;
        const SampleState s0 = states[k];
        states[k] = SampleState{s0.x | 1ull, s0.y | 1ull};       CHECK(bits(false, false) == SAMPLE_BAD_STATE);
        states[k] = SampleState{s0.x | (1ull << 6), s0.y};       CHECK(bits(false, true) == SAMPLE_BAD_STATE);
        states[k] = SampleState{s0.x, s0.y | (1ull << 63)};      CHECK(bits(false, false) == SAMPLE_BAD_STATE);
        states[k] = s0;
        float &f0 = boards[k * 84 + 35], &f1 = boards[k * 84 + 42 + 35];      // the bottom-left cell in both planes
        const float a0 = f0, b0 = f1;
        f0 = 0.5f;            CHECK(bits(true, false) == SAMPLE_BAD_FEATURE);
        f0 = 1.0f; f1 = 1.0f; CHECK(bits(true, true) == (SAMPLE_BAD_FEATURE | SAMPLE_BAD_STATE));
        f0 = a0; f1 = b0;
        CHECK(bits(false, false) == 0u && bits(true, true) == 0u);
    }
    CHECK(sample_state_bits(0, 0) == 0u && sample_state_bits(SAMPLE_BOARD, 0) == 0u && sample_state_bits(0, ~SAMPLE_BOARD) == SAMPLE_BAD_STATE);
    CHECK(sample_bad_text(0, false) == nullptr && sample_bad_text(0, true) == nullptr);
    CHECK(std::strstr(sample_bad_text(SAMPLE_BAD_VALUE, true), "[0, 1]") && !std::strstr(sample_bad_text(SAMPLE_BAD_VALUE, false), "[0, 1]"));

    Carve c;
    CHECK(c.need(0) == 0 && c.total == 0);
    CHECK(c.need(1) == 0 && c.total == 256);
    CHECK(c.need(256) == 256 && c.total == 512);
    CHECK(c.need(257) == 512 && c.total == 1024);
    CHECK(c.need(0) == 1024 && c.total == 1024);

    std::vector<char> buf(1024);
    char* b = buf.data();
    {
        const SampleSpan in[2] = {{b, 256}, {nullptr, 99}}, apart[2] = {{b + 256, 256}, {b + 512, 0}}, into[2] = {{nullptr, 1}, {b + 255, 10}};
        const SampleSpan empty[1] = {{b, 0}}, inside[1] = {{b + 10, 1}}, before[1] = {{b, 300}};
        CHECK(!sample_arrays_overlap(in, apart) && sample_arrays_overlap(in, into) && !sample_arrays_overlap(in, empty));
        CHECK(sample_arrays_overlap(in, inside) && sample_arrays_overlap(apart, before) && !sample_arrays_overlap(empty, before));
    }
    std::printf("ok\n");
    return 0;
}
