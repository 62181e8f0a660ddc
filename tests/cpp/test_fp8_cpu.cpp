// The "net_fp8" quantiser (csrc/az_fp8.h) without a GPU: tests/test_fp8_cpu.py feeds it arrays and compares with torch.float8_e4m3fn
// and with a plain restatement of the scale rules and of the packed copy's index math.
//   quant  in.f32 out.u8     codes of the floats
//   decode out.f32           the values of the 256 codes
//   scales in.f32 out.f32    per input amax: {weight scale, activation scale}
//   offsets C out.i64        fp8_ring_offset(C, n, tap, c) for every (n, tap, c), c fastest
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "az_fp8.h"

template <class T>
static std::vector<T> read_all(const char* path) {
    std::vector<T> v;
    FILE* f = std::fopen(path, "rb");
    if (!f) { std::perror(path); std::exit(2); }
    T buf[4096];
    size_t n;
    while ((n = std::fread(buf, sizeof(T), 4096, f)) > 0) v.insert(v.end(), buf, buf + n);
    std::fclose(f);
    return v;
}
template <class T>
static void write_all(const char* path, const std::vector<T>& v) {
    FILE* f = std::fopen(path, "wb");
    if (!f || std::fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) { std::perror(path); std::exit(2); }
    std::fclose(f);
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    const char* mode = argv[1];
    if (!std::strcmp(mode, "quant") && argc == 4) {
        const std::vector<float> in = read_all<float>(argv[2]);
        std::vector<uint8_t> out(in.size());
        for (size_t i = 0; i < in.size(); ++i) out[i] = az::fp8_e4m3_from_f32(in[i]);
        write_all(argv[3], out);
    } else if (!std::strcmp(mode, "decode")) {
        std::vector<float> out(256);
        for (int c = 0; c < 256; ++c) out[c] = az::fp8_e4m3_to_f32((uint8_t)c);
        write_all(argv[2], out);
    } else if (!std::strcmp(mode, "scales") && argc == 4) {
        const std::vector<float> in = read_all<float>(argv[2]);
        std::vector<float> out(2 * in.size());
        for (size_t i = 0; i < in.size(); ++i) { out[2 * i] = az::fp8_weight_scale(in[i]); out[2 * i + 1] = az::fp8_act_scale(in[i]); }
        write_all(argv[3], out);
    } else if (!std::strcmp(mode, "offsets") && argc == 4) {
        const int C = std::atoi(argv[2]);
        std::vector<int64_t> out;
        out.reserve((size_t)9 * C * C);
        for (int n = 0; n < C; ++n)
            for (int tap = 0; tap < 9; ++tap)
                for (int c = 0; c < C; ++c) out.push_back(az::fp8_ring_offset(C, n, tap, c));
        write_all(argv[3], out);
    } else {
        return 2;
    }
    return 0;
}
