// csrc/az_reanalyse.h compiled by g++ (tests/test_reanalyse_cpu.py): the position rule of az_reanalyse over positions read from stdin, and the
// Coaches' rule (which history entries, which game ids) as that header and include/az_host.hpp each state it.  TEST INFRASTRUCTURE ONLY.
// Build: g++ -std=c++17 -O1 -I alphazero-rs_amd/csrc tests/cpp/reanalyse_twin.cpp
//   reanalyse_twin positions   stdin: "mine theirs" (hex) per line       stdout: the verdict bits and the refusal sentence per line
//   reanalyse_twin planes      stdin: 84 features per line               stdout: "bits mine theirs" (hex) per line
//   reanalyse_twin rule        stdout: "iteration len entries_csrc entries_host" then "iteration h id_csrc id_host" (hex) lines
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "az_reanalyse.h"
#include "../../include/az_host.hpp"

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    if (!std::strcmp(argv[1], "positions")) {
        uint64_t m, t;
        while (std::scanf("%" SCNx64 " %" SCNx64, &m, &t) == 2) {
            const az::SampleState s{m, t};
            uint64_t mine = 0, theirs = 0;
            const uint32_t b = az::reanalyse_check(&s, nullptr, 0, &mine, &theirs);
            if (b != az::reanalyse_position_bits(m, t) || mine != m || theirs != t) return 3;
            const char* why = az::reanalyse_bad_text(b);
            std::printf("%u %s\n", b, why ? why : "-");
        }
        return 0;
    }
    if (!std::strcmp(argv[1], "planes")) {
        std::vector<float> f(84);
        for (;;) {
            for (int i = 0; i < 84; ++i)
                if (std::scanf("%f", &f[(size_t)i]) != 1) return 0;
            uint64_t mine = 0, theirs = 0;
            const uint32_t b = az::reanalyse_check(nullptr, f.data(), 0, &mine, &theirs);
            std::printf("%u %" PRIx64 " %" PRIx64 "\n", b, mine, theirs);
        }
    }
    if (!std::strcmp(argv[1], "rule")) {
        for (uint64_t it = 0; it < 4; ++it)
            for (int len = 0; len < 6; ++len) {
                std::printf("%" PRIu64 " %d %d %zu\n", it, len, az::reanalyse_entries(len), az_host::reanalyse_entries((size_t)len));
                for (uint64_t h = 0; h < (uint64_t)az::reanalyse_entries(len); ++h)
                    std::printf("id %" PRIu64 " %" PRIu64 " %" PRIx64 " %" PRIx64 "\n", it, h, az::reanalyse_first_game_id(it, h), az_host::reanalyse_first_game_id(it, h));
            }
        std::printf("max %" PRId64 " default %d base %" PRIx64 " %" PRIx64 "\n", az::REANALYSE_MAX_POSITIONS, az::REANALYSE_DEFAULT_CONCURRENT,
                    az::REANALYSE_ID_BASE, az_host::REANALYSE_ID_BASE);
        return 0;
    }
    return 2;
}
