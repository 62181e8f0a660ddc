// The g++ build of csrc/az_draw.h for tests/train_draw_twin.py: the rule as the engine's host and device code compile it, without HIP.
#include <cstdint>
#include <vector>

#include "az_draw.h"

extern "C" {

// Q [n] and the rows of global steps t0 .. t0 + steps at batch b; returns W
uint64_t twin_train_draw(int64_t n, const uint32_t* weights, int32_t flags, uint64_t seed, uint64_t t0, int64_t steps, int64_t b,
                         int64_t* idx, uint8_t* mir, uint64_t* Q) {
    const uint64_t W = az::draw_prefix(weights, n, Q);
    if (W == 0) return 0;
    for (int64_t k = 0; k < steps * b; ++k) {
        const uint64_t t = t0 + (uint64_t)(k / b), j = (uint64_t)(k % b);
        idx[k] = az::draw_row(weights ? Q : nullptr, n, W, seed, t, j);
        mir[k] = ((flags & az::DRAW_MIRROR) && az::draw_mirrored(seed, t, j)) ? 1 : 0;
    }
    return W;
}

int64_t twin_train_epoch_steps(uint64_t S, int64_t b) { return az::draw_epoch_steps(S, b); }

}
