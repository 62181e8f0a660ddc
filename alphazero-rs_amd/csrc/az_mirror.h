// az_mirror.h -- the left-right symmetry of the 7 x 6 board behind the opt-in "eval_mirror" (include/az_engine.h).
// Plain C++ on uint64_t with no HIP in it: hipcc compiles it for the device (az_game.h, az_tree.hip, az_engine.hip) and g++ for the host
// (tests/cpp/test_mirror_cpu.cpp); integer operations only, so both produce the same bits.
//
// Bitboards as in az_game.h: bit(col, row) = col * 7 + row, row 0 = bottom, `mine` = the side to move.
//   mirror      column c <-> column 6 - c of one bitboard (get_symmetries, connect_four_game.rs:205-211)
//   key         the 49-bit pack word of a state (== c4_key of az_game.h): mine + (mine | theirs) + one bit per column bottom
//   canonical   c(s) = s or mirror(s), whichever has the smaller key as an unsigned 64-bit integer; on equal keys (a self-symmetric
//               position, the empty board included) s itself, "not mirrored".  mirrored = 1 <=> c(s) is mirror(s) and differs from s.
// mirror is an involution and key is injective on states, so c(mirror(s)) == c(s) and exactly one of s, mirror(s) is "mirrored" unless
// they are equal.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define AZM_HD __host__ __device__ __forceinline__
#else
#define AZM_HD inline
#endif

namespace az {

constexpr int MIRROR_COLS = 7;
constexpr uint64_t MIRROR_BOTTOM = 1ull | (1ull << 7) | (1ull << 14) | (1ull << 21) | (1ull << 28) | (1ull << 35) | (1ull << 42);

AZM_HD uint64_t mirror_bits(uint64_t b) {
    uint64_t r = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int c = 0; c < MIRROR_COLS; ++c) r |= ((b >> (c * 7)) & 0x7Full) << ((MIRROR_COLS - 1 - c) * 7);
    return r;
}
AZM_HD uint64_t mirror_key(uint64_t mine, uint64_t theirs) { return mine + (mine | theirs) + MIRROR_BOTTOM; }
// the pack word of mirror(s): the key is built column by column without carries between columns, so it mirrors like a bitboard
AZM_HD uint64_t mirror_key_of_mirrored(uint64_t mine, uint64_t theirs) { return mirror_bits(mirror_key(mine, theirs)); }
AZM_HD constexpr int mirror_action_index(int a) { return MIRROR_COLS - 1 - a; }

struct MirrorCanon {
    uint64_t mine, theirs;
    uint32_t mirrored;      // 1: (mine, theirs) is the mirror image of the input
};
AZM_HD MirrorCanon mirror_canonical(uint64_t mine, uint64_t theirs) {
    const uint64_t mm = mirror_bits(mine), mt = mirror_bits(theirs);
    const bool m = mirror_key(mm, mt) < mirror_key(mine, theirs);
    MirrorCanon c;
    c.mine = m ? mm : mine;
    c.theirs = m ? mt : theirs;
    c.mirrored = m ? 1u : 0u;
    return c;
}
// "is s mirrored" from the key alone (one bit reversal instead of two plus a key): equal to mirror_canonical(s).mirrored for every state
// whose stones are stacked from the bottom, i.e. every state a tree node holds (a node's state IS unpack(key))
AZM_HD bool mirror_is_mirrored_key(uint64_t key) { return mirror_bits(key) < key; }

}  // namespace az
