// The g++ build of csrc/az_samples.h behind a C interface (tests/samples_twin.py): the window check that k_merge_keys, k_target_kl,
// k_score_states and k_draw_check_states compile, and the sentences the engine refuses with.  TEST INFRASTRUCTURE ONLY.
// Build: g++ -std=c++17 -O2 -ffp-contract=off -shared -fPIC -I alphazero-rs_amd/csrc
#include <cstdint>

#include "az_samples.h"

extern "C" {

// states [n][2] or (null) boards [n][84], pis [n][7], zs [n]; bits [n] = sample_check per tuple, rebuilt [n][2] = the state it saw.
// Returns the OR of the bits: a window's verdict word
uint32_t twin_sample_check(int64_t n, const uint64_t* states, const float* boards, const float* pis, const float* zs, int32_t strict_pi, uint32_t* bits,
                           uint64_t* rebuilt) {
    const az::SampleWindow w{(const az::SampleState*)states, boards, pis, zs};
    uint32_t all = 0;
    for (int64_t i = 0; i < n; ++i) {
        uint64_t mine = 0, theirs = 0;
        const uint32_t b = az::sample_check(w, i, strict_pi != 0, &mine, &theirs);
        if (bits) bits[i] = b;
        if (rebuilt) { rebuilt[2 * i] = mine; rebuilt[2 * i + 1] = theirs; }
        all |= b;
    }
    return all;
}

const char* twin_sample_bad_text(uint32_t bits, int32_t strict_pi) { return az::sample_bad_text(bits, strict_pi != 0); }

}  // extern "C"
