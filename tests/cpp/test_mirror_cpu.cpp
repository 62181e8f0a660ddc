// The g++ build of csrc/az_mirror.h for tests/test_eval_mirror_cpu.py: reads n states (2 x uint64 each) and writes, per state,
// eight uint64 words {mirror(mine), mirror(theirs), key(s), key of mirror(s) by mirror_key_of_mirrored, c(s).mine, c(s).theirs,
// c(s).mirrored, mirror_is_mirrored_key(key(s))}.
//   test_mirror_cpu <in.bin> <out.bin>
#include <cstdio>
#include <vector>

#include "az_mirror.h"

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    std::vector<uint64_t> in;
    uint64_t buf[2];
    while (std::fread(buf, sizeof(uint64_t), 2, f) == 2) { in.push_back(buf[0]); in.push_back(buf[1]); }
    std::fclose(f);
    std::vector<uint64_t> out;
    out.reserve(in.size() * 4);
    for (size_t i = 0; i + 1 < in.size(); i += 2) {
        const uint64_t mine = in[i], theirs = in[i + 1];
        const az::MirrorCanon c = az::mirror_canonical(mine, theirs);
        const uint64_t k = az::mirror_key(mine, theirs);
        out.push_back(az::mirror_bits(mine));
        out.push_back(az::mirror_bits(theirs));
        out.push_back(k);
        out.push_back(az::mirror_key_of_mirrored(mine, theirs));
        out.push_back(c.mine);
        out.push_back(c.theirs);
        out.push_back(c.mirrored);
        out.push_back(az::mirror_is_mirrored_key(k) ? 1u : 0u);
    }
    f = std::fopen(argv[2], "wb");
    if (!f) return 4;
    const bool ok = std::fwrite(out.data(), sizeof(uint64_t), out.size(), f) == out.size();
    std::fclose(f);
    static_assert(az::mirror_action_index(0) == 6 && az::mirror_action_index(3) == 3, "column c <-> 6 - c");
    return ok ? 0 : 5;
}
