// az_merge.h -- position averaging (az_samples_merge, include/az_engine.h): one tuple per distinct position of a
// training window, carrying the mean pi and the mean z of its copies.  The kernels are in az_merge.hip; the entry is in az_engine.hip.
//
// Four passes over n tuples, all on the engine's stream, all in a workspace the engine owns:
//   keys        one thread per tuple: the state (given, or rebuilt from its feature planes), validated, canonicalised when asked; the key
//               Game::pack(state) goes into an open-addressing table of T >= 2n slots (64-bit atomicCAS on an empty slot, linear probing) and
//               the slot keeps the LOWEST input index of its key (atomicMin)
//   scan        a prefix scan over "this tuple is its key's first occurrence" gives every key its output rank: group j is the j-th distinct
//               key in input order, whatever the table's layout
//   accumulate  every tuple adds its eight fixed-point values q(x) = llrint(x * 2^38) and a count of one to its group, through a per-workgroup
//               LDS table (and a wave-wide sum where a whole wave holds one group); integer addition is associative, so the sums do not depend
//               on any of that
//   finalise    one thread per group: a group of one copies its tuple's bits, a larger one divides in double and rounds once to f32
#pragma once
#include "az_common.h"
#include "az_samples.h"

namespace az {

constexpr long long MERGE_MAX_TUPLES = 1ll << 24;       // keeps every int64 sum below 2^62
constexpr int MERGE_FRAC_BITS = 38;                     // q(x) = llrint((double)x * 2^38)
constexpr uint32_t MERGE_MIRRORED = 1u << 31;           // bit 31 of slot[i]: the tuple's state is the mirror image of its group's

struct MergeBufs {
    uint32_t n;                     // tuples
    SampleWindow in;                // the inputs on the device
    // per tuple
    ulonglong2* cst;                // [n] the state the tuple is merged under (canonicalised when asked)
    uint32_t* slot;                 // [n] its table slot | MERGE_MIRRORED
    // the table, T = tmask + 1 slots
    unsigned long long* tkey;       // [T] 0 = empty (Game::pack is never 0)
    uint32_t* tmin;                 // [T] lowest input index of the key (0xFFFFFFFF = none yet)
    uint32_t* trank;                // [T] output rank of the key
    uint32_t tmask;
    uint32_t* bsum;                 // [blocks of 256 tuples] first occurrences per block, then their exclusive scan
    // per group (at most n)
    uint32_t* first;                // [m] input index of the group's first occurrence
    unsigned long long* sums;       // [m][8] two's-complement int64 sums of q(pi[0..6]), q(z)
    uint32_t* cnt;                  // [m] multiplicity
    uint32_t* hdr;                  // [0] verdict bits of the keys pass (SAMPLE_BAD_* of az_samples.h), [1] m
    // outputs staged on the device, m rows each (boards may be nullptr)
    ulonglong2* o_states;
    float* o_boards;
    float* o_pis;
    float* o_zs;
};

void launch_merge_keys(int game, const MergeBufs& b, int canonical, hipStream_t s);
void launch_merge_scan(const MergeBufs& b, hipStream_t s);
void launch_merge_accumulate(const MergeBufs& b, hipStream_t s);
void launch_merge_finalise(int game, const MergeBufs& b, uint32_t m, hipStream_t s);

}  // namespace az
