// az_net_diag.inc -- superseded kernel generations of the conv net, kept for A/B measurements (tools/) and for the bit-identity
// tests of the kernel families.  Compiled ONLY with -DAZ_DIAG into libaz_engine_diag.so; the shipped libaz_engine.so does not contain
// them.  Included by az_net.hip after the shipped kernels (everything they use is defined there).

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
__global__ __launch_bounds__(256) void k_conv2_table(const EvalBatch eb, const uint16_t* __restrict__ U /*[19683][9][C] f16*/,
                                                     const float* __restrict__ bias /*[C]*/, uint16_t* __restrict__ out /*[n][42][C] bf16*/,
                                                     int C) {
    extern __shared__ __attribute__((aligned(16))) unsigned char u0_lds[];       // U[0][0..8][C] f16
    for (int i = threadIdx.x; i < 9 * C / 8; i += blockDim.x) ((uint4*)u0_lds)[i] = ((const uint4*)U)[i];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const uint32_t items = *eb.n * 6u;
    const uint32_t wave0 = blockIdx.x * 4u + (threadIdx.x >> 6), nwaves = gridDim.x * 4u;
    const int cg = C / 8;
    for (uint32_t it = wave0; it < items; it += nwaves) {
        const uint32_t b = it / 6u;
        const int y = (int)(it - b * 6u);
        const ulonglong2 sv = eb.state[b];
        const int ly = y - 1 + (lane < 21 ? lane / 7 : 0), lx = lane < 21 ? lane % 7 : 0;
        const uint32_t mypat = (ly >= 0 && ly < 6) ? conv1_pattern(sv.x, sv.y, ly, lx) : 0u;
        for (int x = 0; x < 7; ++x) {
            uint32_t row[9];                       // table row (pattern * 9 + tap) of every in-board tap, else ~0
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int ky = t / 3, qy = y + ky - 1, qx = x + t % 3 - 1;
                const bool in = qy >= 0 && qy < 6 && qx >= 0 && qx < 7;
                const uint32_t pq = (uint32_t)__builtin_amdgcn_readlane((int)mypat, in ? ky * 7 + qx : 0);
                row[t] = in ? pq * 9u + (uint32_t)t : 0xFFFFFFFFu;
            }
            for (int c8 = lane; c8 < cg; c8 += 64) {
                f16x8 u[9];
#pragma unroll
                for (int t = 0; t < 9; ++t) {
                    if (row[t] == 0xFFFFFFFFu) continue;
                    if (row[t] < 9u) u[t] = *(const f16x8*)(u0_lds + ((size_t)row[t] * C + (size_t)c8 * 8) * 2);
                    else u[t] = *(const f16x8*)(U + ((size_t)row[t] * C + (size_t)c8 * 8));
                }
                float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int t = 0; t < 9; ++t)                 // taps in (ky, kx) order: the fixed summation order of a row
                    if (row[t] != 0xFFFFFFFFu) {
#pragma unroll
                        for (int i = 0; i < 8; ++i) acc[i] += (float)u[t][i];
                    }
                const float4 b0 = *(const float4*)(bias + c8 * 8), b1 = *(const float4*)(bias + c8 * 8 + 4);
                uint4 o;
                o.x = pack_bf16x2(fmaxf(acc[0] + b0.x, 0.f), fmaxf(acc[1] + b0.y, 0.f));
                o.y = pack_bf16x2(fmaxf(acc[2] + b0.z, 0.f), fmaxf(acc[3] + b0.w, 0.f));
                o.z = pack_bf16x2(fmaxf(acc[4] + b1.x, 0.f), fmaxf(acc[5] + b1.y, 0.f));
                o.w = pack_bf16x2(fmaxf(acc[6] + b1.z, 0.f), fmaxf(acc[7] + b1.w, 0.f));
                *(uint4*)(out + ((size_t)b * 42 + (size_t)(y * 7 + x)) * C + (size_t)c8 * 8) = o;
            }
        }
    }
}

template <int LAYER, int NS, int BM = 128>
__global__ __launch_bounds__(256, (NS <= 2 ? 2 : 1)) void k_gemm_ring(const GemmDesc d) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[NS * (BM * 128 + 16384)];
    gemm_ring_body<NS, BM>(d, smem, (int)(*d.n_dev) * d.rows_per_sample);
}

// ---- 256x256 tile variant for the big layers (conv2, conv3): LDS-DMA staging ------------------------------
// 8 waves (2 x 4), each wave a 128(m) x 64(n) sub-tile = 8 x 4 accumulators of v_mfma_f32_16x16x32_bf16.
// Both operands go global -> LDS with global_load_lds_dwordx4 (no VGPR staging, no ds_write): one wave-instruction
// writes 1 KiB = 8 tile rows x 128 B linearly, so the XOR swizzle (chunk c of row r at slot c ^ (r&7)) is applied
// to the per-lane SOURCE address and again on the fragment reads.  Two 64 KiB LDS buffers; the next K-step's DMA is
// issued before this K-step's MFMAs and retired by vmcnt(0) + barrier at the end of the step.
// STAMP: the clock-stamp build ("gemm_variant" 13, tools/clock_probe.py): same results, plus per-block {shader cycles, 100 MHz ticks} of the K loop
constexpr int HBM_ = 256;
template <int LAYER, int PIPE, bool STAMP = false>
__global__ __launch_bounds__(512, 2) void k_gemm256(const GemmDesc d) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[2 * (HBM_ + HBN_) * 128];
    const int M = (int)(*d.n_dev) * d.rows_per_sample;
    const int ntaps = d.K / d.cin;
    const int NT = d.N / HBN_;
    // XCD-aware order (blocks b and b+8 share an XCD): the NT column tiles of a row tile run back to back on one XCD
    const int id = blockIdx.x;
    const int xcd = id & 7, j = id >> 3;
    const int ntile = j % NT, mtile = (j / NT) * 8 + xcd;
    const int m0 = mtile * HBM_, n0 = ntile * HBN_;
    if (m0 >= M) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 2, wc = wave & 3;
    // DMA map: instruction q of wave w fills tile rows (q*8+w)*8 .. +7; lane -> row (lane>>3), slot (lane&7)
    const int lrow = lane >> 3;
    const int chunk = (lane & 7) ^ lrow;
    auto row_off = [&](int q) -> uint32_t {
        int m = m0 + (q * 8 + wave) * 8 + lrow;
        m = m < M ? m : M - 1;
        const int b = m / d.rows_per_sample, r = m - b * d.rows_per_sample;
        const int y = r / d.out_w, x = r - y * d.out_w;
        return (uint32_t)(((b * d.in_h + y) * d.in_w + x) * d.in_c + chunk * 8);
    };
    const uint32_t a_off0 = row_off(0), a_off1 = row_off(1), a_off2 = row_off(2), a_off3 = row_off(3);
    const uint32_t b_off0 = (uint32_t)((n0 + wave * 8 + lrow) * d.K + chunk * 8);
    const uint32_t b_step = 64u * (uint32_t)d.K;
    const uint32_t a_ob0 = a_off0 * 2u, a_ob1 = a_off1 * 2u, a_ob2 = a_off2 * 2u, a_ob3 = a_off3 * 2u;     // bytes
    const uint32_t b_ob0 = b_off0 * 2u, b_ob1 = (b_off0 + b_step) * 2u, b_ob2 = (b_off0 + 2u * b_step) * 2u,
                   b_ob3 = (b_off0 + 3u * b_step) * 2u;
    typedef __attribute__((address_space(3))) void* lds_ptr;
    typedef const __attribute__((address_space(1))) void* gbl_ptr;
    // K-step walker (channel block outer, tap inner) kept in scalars and advanced with adds and compares only: the
    // straightforward kt -> (cb, tap, ky, kx) needs two runtime integer divisions per K-step per wave, which showed
    // up as 10x SQ_ACTIVE_INST_SCA (257 cycles per wave per K-step) in the PMC profile.
    int ks_tap = 0, ks_kx = 0;
    uint32_t ks_c0 = 0, ks_toff = 0, ks_kk = 0;
#define AZ_KSTEP_ADVANCE()                                                                              \
    {                                                                                                   \
        ++ks_tap; ++ks_kx; ks_toff += (uint32_t)d.in_c; ks_kk += (uint32_t)d.cin;                       \
        if (ks_kx == d.tap_w) { ks_kx = 0; ks_toff += (uint32_t)((d.in_w - d.tap_w) * d.in_c); }        \
        if (ks_tap == ntaps) { ks_tap = 0; ks_kx = 0; ks_c0 += GBK; ks_toff = ks_c0; ks_kk = ks_c0; }   \
    }
    // DMA of the K-step the walker points at, into LDS buffer buf_; then advance the walker
#define AZ_DMA(kt_, buf_)                                                                               \
    {                                                                                                   \
        /* wave-uniform base (SGPR pair) + 32-bit per-lane byte offset: the saddr form, no 64-bit VALU adds */ \
        const char* abase = (const char*)(d.A + ks_toff);                                               \
        const char* wbase = (const char*)(d.W + ks_kk);                                                 \
        unsigned char* la = smem + (buf_) * 65536 + wave * 1024;                                        \
        unsigned char* lb = la + 32768;                                                                 \
        __builtin_amdgcn_global_load_lds((gbl_ptr)(abase + a_ob0), (lds_ptr)(la), 16, 0, 0);            \
        __builtin_amdgcn_global_load_lds((gbl_ptr)(abase + a_ob1), (lds_ptr)(la + 8192), 16, 0, 0);     \
        __builtin_amdgcn_global_load_lds((gbl_ptr)(abase + a_ob2), (lds_ptr)(la + 16384), 16, 0, 0);    \
        __builtin_amdgcn_global_load_lds((gbl_ptr)(abase + a_ob3), (lds_ptr)(la + 24576), 16, 0, 0);    \
        __builtin_amdgcn_global_load_lds((gbl_ptr)(wbase + b_ob0), (lds_ptr)(lb), 16, 0, 0);            \
        __builtin_amdgcn_global_load_lds((gbl_ptr)(wbase + b_ob1), (lds_ptr)(lb + 8192), 16, 0, 0);     \
        __builtin_amdgcn_global_load_lds((gbl_ptr)(wbase + b_ob2), (lds_ptr)(lb + 16384), 16, 0, 0);    \
        __builtin_amdgcn_global_load_lds((gbl_ptr)(wbase + b_ob3), (lds_ptr)(lb + 24576), 16, 0, 0);    \
        AZ_KSTEP_ADVANCE();                                                                             \
    }
    f32x4 acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int jn = 0; jn < 4; ++jn) acc[i][jn] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int nk = d.K / GBK;
    const int frow = lane & 15, fq = lane >> 4, fsw = lane & 7;
    AZ_DMA(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    unsigned long long st0 = 0, sr0 = 0;
    if constexpr (STAMP) { st0 = __builtin_amdgcn_s_memtime(); sr0 = __builtin_amdgcn_s_memrealtime(); }
    // LDS byte offsets of this lane's fragment rows (row-major 128-B rows, XOR-swizzled 16-B slots)
    const int a_row0 = (wr * 128 + frow) * 128, b_row0 = 32768 + (wc * 64 + frow) * 128;
    const int coff0 = ((0 + fq) ^ fsw) << 4, coff1 = ((4 + fq) ^ fsw) << 4;
#define AZ_LDA(dst_, base_, mt0_, coff_)                                                     \
    _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_)                                         \
        dst_[i_] = *(const bf16x8*)((base_) + a_row0 + ((mt0_) + i_) * 2048 + (coff_));
#define AZ_LDB(dst_, base_, coff_)                                                           \
    _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_)                                         \
        dst_[i_] = *(const bf16x8*)((base_) + b_row0 + i_ * 2048 + (coff_));
#define AZ_MMA(mt0_, fb_, fa_)                                                               \
    _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_)                                         \
        _Pragma("unroll") for (int j_ = 0; j_ < 4; ++j_)                                     \
            acc[(mt0_) + i_][j_] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb_[j_], fa_[i_], acc[(mt0_) + i_][j_], 0, 0, 0);
    for (int kt = 0; kt < nk; ++kt) {
        if (kt + 1 < nk) AZ_DMA(kt + 1, (kt + 1) & 1);
        const unsigned char* sA = smem + (kt & 1) * 65536;
        if constexpr (PIPE == 0) {
            const unsigned char* sB = sA + 32768;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const int coff = ((ks * 4 + fq) ^ fsw) << 4;
                bf16x8 fa[8], fb[4];
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) fb[nt] = *(const bf16x8*)(sB + (wc * 64 + nt * 16 + frow) * 128 + coff);
#pragma unroll
                for (int mt = 0; mt < 8; ++mt) fa[mt] = *(const bf16x8*)(sA + (wr * 128 + mt * 16 + frow) * 128 + coff);
#pragma unroll
                for (int mt = 0; mt < 8; ++mt)
#pragma unroll
                    for (int nt = 0; nt < 4; ++nt)
                        acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[nt], fa[mt], acc[mt][nt], 0, 0, 0);
            }
        } else {
            // 4 phases of 16 MFMAs; the fragments of phase p+1 are requested before the MFMAs of phase p issue,
            // so an LDS round trip is exposed once per K-step (after the barrier) instead of eight times.
            bf16x8 fbX[4] = {}, fbY[4] = {}, faX[4] = {}, faY[4] = {};
            AZ_LDB(fbX, sA, coff0);
            AZ_LDA(faX, sA, 0, coff0);
            __builtin_amdgcn_sched_barrier(0);
            AZ_LDA(faY, sA, 4, coff0);
            __builtin_amdgcn_sched_barrier(0);
            AZ_MMA(0, fbX, faX);
            __builtin_amdgcn_sched_barrier(0);
            AZ_LDB(fbY, sA, coff1);
            AZ_LDA(faX, sA, 0, coff1);
            __builtin_amdgcn_sched_barrier(0);
            AZ_MMA(4, fbX, faY);
            __builtin_amdgcn_sched_barrier(0);
            AZ_LDA(faY, sA, 4, coff1);
            __builtin_amdgcn_sched_barrier(0);
            AZ_MMA(0, fbY, faX);
            __builtin_amdgcn_sched_barrier(0);
            AZ_MMA(4, fbY, faY);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
#undef AZ_LDA
#undef AZ_LDB
#undef AZ_MMA
    if constexpr (STAMP) {
        // in-kernel clock = d(s_memtime) / d(s_memrealtime) x 100 MHz (MI355X_MICROARCH.md, DVFS give-back item 6);
        // the stamps go to a debug buffer nothing else reads
        const unsigned long long st1 = __builtin_amdgcn_s_memtime(), sr1 = __builtin_amdgcn_s_memrealtime();
        if (tid == 0 && d.dbg && blockIdx.x < 1024) { d.dbg[2 * blockIdx.x] = st1 - st0; d.dbg[2 * blockIdx.x + 1] = sr1 - sr0; }
    }
#undef AZ_DMA
#undef AZ_KSTEP_ADVANCE
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        const int n = n0 + wc * 64 + nt * 16 + fq * 4;
        const float4 bv = *(const float4*)(d.bias + n);
#pragma unroll
        for (int mt = 0; mt < 8; ++mt) {
            const int m = m0 + wr * 128 + mt * 16 + frow;
            if (m >= M) continue;
            float r0 = acc[mt][nt][0] + bv.x, r1 = acc[mt][nt][1] + bv.y, r2 = acc[mt][nt][2] + bv.z,
                  r3 = acc[mt][nt][3] + bv.w;
            if (d.relu) { r0 = fmaxf(r0, 0.f); r1 = fmaxf(r1, 0.f); r2 = fmaxf(r2, 0.f); r3 = fmaxf(r3, 0.f); }
            uint2 o;
            o.x = pack_bf16x2(r0, r1);
            o.y = pack_bf16x2(r2, r3);
            *(uint2*)(d.out + (size_t)m * d.N + n) = o;
        }
    }
}

// ---- conv2 as an IMAGE-RESIDENT implicit GEMM ----------------------------------------------------------------
// The 9 filter taps of one 64-channel block read overlapping shifted windows of the same activations.  With an M tile
// of 6 whole boards (252 output rows) the 64-channel slice of those boards is 6 x 42 x 128 B = 31.5 KiB: it is DMA'd
// into LDS ONCE per channel block (double-buffered, landing during the previous block's taps) and the A fragments of
// tap (ky,kx) are read from it at row m + (ky-1)*7 + (kx-1); out-of-board taps read a zero row ('same' padding).
// Only the weight tile (32 KiB) still streams every K-step, so L2->LDS traffic falls from 64 KiB to 35.5 KiB per
// K-step.  Same K order (channel block outer, tap inner) and per-row accumulation order as the other kernels.
template <int LAYER>
__global__ __launch_bounds__(512, 2) void k_conv_img(const GemmDesc d) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[4 * 32768];   // img[2] | w[2]
    const int n_boards = (int)(*d.n_dev);
    const int M = n_boards * 42;
    const int C = d.cin;
    const int NT = d.N / HBN_;
    const int id = blockIdx.x;
    const int xcd = id & 7, j = id >> 3;
    const int ntile = j % NT, mtile = (j / NT) * 8 + xcd;
    const int b0 = mtile * IMG_NB, n0 = ntile * HBN_;
    if (b0 >= n_boards) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 2, wc = wave & 3;
    if (tid < 16) *(uint4*)(smem + (tid >> 3) * 32768 + IMG_ZERO_ROW * 128 + (tid & 7) * 16) = make_uint4(0, 0, 0, 0);
    // image DMA map: item q of this thread = LDS row q*64 + wave*8 + (lane>>3), slot lane&7 (rows >= 252 are not loaded)
    const int lrow = lane >> 3;
    const int chunk = (lane & 7) ^ lrow;
    auto img_off = [&](int q) -> uint32_t {         // byte offset of this lane's 16 bytes of image row q*64 + wave*8 + lrow
        int r = q * 64 + wave * 8 + lrow;
        r = r < IMG_ROWS ? r : IMG_ROWS - 1;
        int b = b0 + r / 42;
        b = b < n_boards ? b : n_boards - 1;
        const int p = r % 42, y = p / 7, x = p - y * 7;
        return (uint32_t)(((b * 8 + y + 1) * 9 + x + 1) * C + chunk * 8) * 2u;
    };
    const uint32_t i_ob0 = img_off(0), i_ob1 = img_off(1), i_ob2 = img_off(2), i_ob3 = img_off(3);
    const bool i_row3 = 192 + wave * 8 + lrow < IMG_ROWS;
    const uint32_t b_ob0 = (uint32_t)((n0 + wave * 8 + lrow) * d.K + chunk * 8) * 2u;
    const uint32_t b_stepb = 128u * (uint32_t)d.K;                       // 64 weight rows, in bytes
    const uint32_t b_ob1 = b_ob0 + b_stepb, b_ob2 = b_ob0 + 2u * b_stepb, b_ob3 = b_ob0 + 3u * b_stepb;
    typedef __attribute__((address_space(3))) void* lds_ptr;
    typedef const __attribute__((address_space(1))) void* gbl_ptr;
    // wave-uniform base + 32-bit per-lane byte offset (the saddr form of global_load_lds)
#define AZ_IDMA_W(kk_, buf_)                                                                                 \
    {                                                                                                        \
        unsigned char* lb = smem + 65536 + (buf_) * 32768 + wave * 1024;                                     \
        const char* wbase = (const char*)(d.W + (kk_));                                                      \
        __builtin_amdgcn_global_load_lds((gbl_ptr)(wbase + b_ob0), (lds_ptr)(lb), 16, 0, 0);                 \
        __builtin_amdgcn_global_load_lds((gbl_ptr)(wbase + b_ob1), (lds_ptr)(lb + 8192), 16, 0, 0);          \
        __builtin_amdgcn_global_load_lds((gbl_ptr)(wbase + b_ob2), (lds_ptr)(lb + 16384), 16, 0, 0);         \
        __builtin_amdgcn_global_load_lds((gbl_ptr)(wbase + b_ob3), (lds_ptr)(lb + 24576), 16, 0, 0);         \
    }
#define AZ_IDMA_IMG(cb_)                                                                                     \
    {                                                                                                        \
        unsigned char* la = smem + ((cb_) & 1) * 32768 + wave * 1024;                                        \
        const char* ibase = (const char*)(d.A + (cb_) * 64);                                                 \
        __builtin_amdgcn_global_load_lds((gbl_ptr)(ibase + i_ob0), (lds_ptr)(la), 16, 0, 0);                 \
        __builtin_amdgcn_global_load_lds((gbl_ptr)(ibase + i_ob1), (lds_ptr)(la + 8192), 16, 0, 0);          \
        __builtin_amdgcn_global_load_lds((gbl_ptr)(ibase + i_ob2), (lds_ptr)(la + 16384), 16, 0, 0);         \
        if (i_row3) __builtin_amdgcn_global_load_lds((gbl_ptr)(ibase + i_ob3), (lds_ptr)(la + 24576), 16, 0, 0); \
    }
    f32x4 acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int jn = 0; jn < 4; ++jn) acc[i][jn] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int frow = lane & 15, fq = lane >> 4, fsw = lane & 7;
    // per-lane fragment rows: low 16 bits = output row inside the tile, bits 16..24 = tap validity ('same' padding)
    uint32_t rowmask[8];
#pragma unroll
    for (int mt = 0; mt < 8; ++mt) {
        const int ml = wr * 128 + mt * 16 + frow;
        const int p = ml % 42, y = p / 7, x = p - y * 7;
        uint32_t mask = 0;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int iy = y + t / 3 - 1, ix = x + t % 3 - 1;
            if (ml < IMG_ROWS && iy >= 0 && iy < 6 && ix >= 0 && ix < 7) mask |= 1u << t;
        }
        rowmask[mt] = (uint32_t)ml | (mask << 16);
    }
    const int b_row0 = 65536 + (wc * 64 + frow) * 128;
    const int coffB0 = ((0 + fq) ^ fsw) << 4, coffB1 = ((4 + fq) ^ fsw) << 4;
    // A fragment (mt, ks) of the current tap: LDS row = m + dt if the tap is inside the board, else the zero row
#define AZ_ILDA(dst_, img_, mt0_, ks_)                                                                       \
    _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_) {                                                       \
        const uint32_t rm_ = rowmask[(mt0_) + i_];                                                           \
        const int r_ = ((rm_ >> tapbit) & 1u) ? (int)(rm_ & 0xFFFFu) + dt : IMG_ZERO_ROW;                    \
        dst_[i_] = *(const bf16x8*)((img_) + r_ * 128 + ((((ks_) * 4 + fq) ^ (r_ & 7)) << 4));               \
    }
#define AZ_ILDB(dst_, wb_, coff_)                                                                            \
    _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_)                                                         \
        dst_[i_] = *(const bf16x8*)((wb_) + b_row0 + i_ * 2048 + (coff_));
#define AZ_IMMA(mt0_, fb_, fa_)                                                                              \
    _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_)                                                         \
        _Pragma("unroll") for (int j_ = 0; j_ < 4; ++j_)                                                     \
            acc[(mt0_) + i_][j_] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb_[j_], fa_[i_], acc[(mt0_) + i_][j_], 0, 0, 0);
    const int ncb = C / 64;
    const int nk = ncb * 9;
    AZ_IDMA_W(0, 0);
    AZ_IDMA_IMG(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    int cb = 0, tap = 0;
    for (int kt = 0; kt < nk; ++kt) {
        const bool new_img = tap == 0 && cb + 1 < ncb;
        if (kt + 1 < nk) {
            const int ntap = tap == 8 ? 0 : tap + 1, ncbi = tap == 8 ? cb + 1 : cb;
            AZ_IDMA_W(ntap * C + ncbi * 64, (kt + 1) & 1);
        }
        if (new_img) AZ_IDMA_IMG(cb + 1);       // issued after the weights: stays in flight over this step's wait
        const unsigned char* sI = smem + (cb & 1) * 32768;
        const unsigned char* sW = smem + (kt & 1) * 32768;       // b_row0 already carries the 64 KiB image offset
        const int ky = tap / 3, kx = tap - ky * 3;
        const int dt = (ky - 1) * 7 + (kx - 1);
        const int tapbit = 16 + tap;
        // 4 clusters of 16 MFMAs; the fragments of the next cluster are requested before the current one issues
        bf16x8 fbX[4], fbY[4], faX[4], faY[4];
        AZ_ILDB(fbX, sW, coffB0);
        AZ_ILDA(faX, sI, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        AZ_ILDA(faY, sI, 4, 0);
        __builtin_amdgcn_sched_barrier(0);
        AZ_IMMA(0, fbX, faX);
        __builtin_amdgcn_sched_barrier(0);
        AZ_ILDB(fbY, sW, coffB1);
        AZ_ILDA(faX, sI, 0, 1);
        __builtin_amdgcn_sched_barrier(0);
        AZ_IMMA(4, fbX, faY);
        __builtin_amdgcn_sched_barrier(0);
        AZ_ILDA(faY, sI, 4, 1);
        __builtin_amdgcn_sched_barrier(0);
        AZ_IMMA(0, fbY, faX);
        __builtin_amdgcn_sched_barrier(0);
        AZ_IMMA(4, fbY, faY);
        // counted wait: the next weight tile must have landed; the next image (issued after it) may stay in flight
        if (new_img) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                                    // raw: __syncthreads() would drain vmcnt to 0
        __builtin_amdgcn_sched_barrier(0);
        if (++tap == 9) { tap = 0; ++cb; }
    }
#undef AZ_IDMA_W
#undef AZ_IDMA_IMG
#undef AZ_ILDA
#undef AZ_ILDB
#undef AZ_IMMA
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        const int n = n0 + wc * 64 + nt * 16 + fq * 4;
        const float4 bv = *(const float4*)(d.bias + n);
#pragma unroll
        for (int mt = 0; mt < 8; ++mt) {
            const int ml = wr * 128 + mt * 16 + frow;
            const int m = b0 * 42 + ml;
            if (ml >= IMG_ROWS || m >= M) continue;
            float r0 = acc[mt][nt][0] + bv.x, r1 = acc[mt][nt][1] + bv.y, r2 = acc[mt][nt][2] + bv.z,
                  r3 = acc[mt][nt][3] + bv.w;
            if (d.relu) { r0 = fmaxf(r0, 0.f); r1 = fmaxf(r1, 0.f); r2 = fmaxf(r2, 0.f); r3 = fmaxf(r3, 0.f); }
            uint2 o;
            o.x = pack_bf16x2(r0, r1);
            o.y = pack_bf16x2(r2, r3);
            *(uint2*)(d.out + (size_t)m * d.N + n) = o;
        }
    }
}

// ---- conv2 image-resident, TWO independent workgroups per CU ---------------------------------------------------------
// k_conv_img's 8 waves share one barrier, so the two waves of every SIMD run in lockstep: both in their MFMA clusters
// (contending for the matrix pipe), then both parked at the wait / barrier (pipe idle; SQ_WAIT_INST_ANY 42 %,
// SQ_WAIT_ANY 38 % of wave cycles).  Here the same per-wave work (128 rows x 64 columns, 8 x 4 accumulators) is packaged
// as workgroups of 4 waves -- tile = 6 boards x 128 channels, LDS = one image buffer (32 KiB) + two weight buffers
// (16 KiB each) = 64 KiB -- so two workgroups fit a CU and every SIMD holds one wave of each: their barriers are
// independent and their phases drift apart.  The price is a single image buffer (the image switch every 9 K-steps is
// exposed inside a workgroup and covered by the other one).  Same K order: bit-identical.
// TABLE: the image rows are gathered from the conv1 table (d.A) by pattern index instead of read from act1.
template <int LAYER, bool TABLE = false>
__global__ __launch_bounds__(256, 2) void k_conv_img2(const GemmDesc d) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[2 * 32768];   // img | w[2] (16 KiB each)
    const int n_boards = (int)(*d.n_dev);
    const int M = n_boards * 42;
    const int C = d.cin;
    const int NT = d.N / HBN2_;
    const int id = blockIdx.x;
    const int xcd = id & 7, j = id >> 3;
    const int ntile = j % NT, mtile = (j / NT) * 8 + xcd;
    const int b0 = mtile * IMG_NB, n0 = ntile * HBN2_;
    if (b0 >= n_boards) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    if (tid < 8) *(uint4*)(smem + IMG_ZERO_ROW * 128 + tid * 16) = make_uint4(0, 0, 0, 0);
    const int lrow = lane >> 3;
    const int chunk = (lane & 7) ^ lrow;
    // image DMA map: piece q (0..7) of wave w = LDS rows (q*4 + w)*8 + lrow; rows >= 252 are not loaded
    uint32_t i_ob[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        int r = (q * 4 + wave) * 8 + lrow;
        r = r < IMG_ROWS ? r : IMG_ROWS - 1;
        int b = b0 + r / 42;
        b = b < n_boards ? b : n_boards - 1;
        const int p = r % 42, y = p / 7, x = p - y * 7;
        if constexpr (TABLE) {
            const ulonglong2 st = d.states[b];
            i_ob[q] = (conv1_pattern(st.x, st.y, y, x) * (uint32_t)C + (uint32_t)chunk * 8u) * 2u;
        } else {
            i_ob[q] = (uint32_t)(((b * 8 + y + 1) * 9 + x + 1) * C + chunk * 8) * 2u;
        }
    }
    const bool i_last_ok = (7 * 4 + wave) * 8 + lrow < IMG_ROWS;          // only piece 7 can run past row 251
    // weight DMA map: piece q (0..3) of wave w = tile rows (q*4 + w)*8 + lrow
    const uint32_t b_ob0 = (uint32_t)((n0 + wave * 8 + lrow) * d.K + chunk * 8) * 2u;
    const uint32_t b_stepb = 64u * (uint32_t)d.K;                        // 32 weight rows, in bytes
    const uint32_t b_ob1 = b_ob0 + b_stepb, b_ob2 = b_ob0 + 2u * b_stepb, b_ob3 = b_ob0 + 3u * b_stepb;
    typedef __attribute__((address_space(3))) void* lds_ptr;
    typedef const __attribute__((address_space(1))) void* gbl_ptr;
#define AZ_2DMA_W(kk_, buf_)                                                                                 \
    {                                                                                                        \
        unsigned char* lb = smem + 32768 + (buf_) * 16384 + wave * 1024;                                     \
        const char* wbase = (const char*)(d.W + (kk_));                                                      \
        __builtin_amdgcn_global_load_lds((gbl_ptr)(wbase + b_ob0), (lds_ptr)(lb), 16, 0, 0);                 \
        __builtin_amdgcn_global_load_lds((gbl_ptr)(wbase + b_ob1), (lds_ptr)(lb + 4096), 16, 0, 0);          \
        __builtin_amdgcn_global_load_lds((gbl_ptr)(wbase + b_ob2), (lds_ptr)(lb + 8192), 16, 0, 0);          \
        __builtin_amdgcn_global_load_lds((gbl_ptr)(wbase + b_ob3), (lds_ptr)(lb + 12288), 16, 0, 0);         \
    }
#define AZ_2DMA_IMG(cb_)                                                                                     \
    {                                                                                                        \
        unsigned char* la = smem + wave * 1024;                                                              \
        const char* ibase = (const char*)(d.A + (cb_) * 64);                                                 \
        _Pragma("unroll") for (int q_ = 0; q_ < 7; ++q_)                                                     \
            __builtin_amdgcn_global_load_lds((gbl_ptr)(ibase + i_ob[q_]), (lds_ptr)(la + q_ * 4096), 16, 0, 0); \
        if (i_last_ok) __builtin_amdgcn_global_load_lds((gbl_ptr)(ibase + i_ob[7]), (lds_ptr)(la + 7 * 4096), 16, 0, 0); \
    }
    f32x4 acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int jn = 0; jn < 4; ++jn) acc[i][jn] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int frow = lane & 15, fq = lane >> 4, fsw = lane & 7;
    uint32_t rowmask[8];
#pragma unroll
    for (int mt = 0; mt < 8; ++mt) {
        const int ml = wr * 128 + mt * 16 + frow;
        const int p = ml % 42, y = p / 7, x = p - y * 7;
        uint32_t mask = 0;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int iy = y + t / 3 - 1, ix = x + t % 3 - 1;
            if (ml < IMG_ROWS && iy >= 0 && iy < 6 && ix >= 0 && ix < 7) mask |= 1u << t;
        }
        rowmask[mt] = (uint32_t)ml | (mask << 16);
    }
    const int b_row0 = 32768 + (wc * 64 + frow) * 128;
    const int coffB0 = ((0 + fq) ^ fsw) << 4, coffB1 = ((4 + fq) ^ fsw) << 4;
#define AZ_2LDA(dst_, mt0_, ks_)                                                                             \
    _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_) {                                                       \
        const uint32_t rm_ = rowmask[(mt0_) + i_];                                                           \
        const int r_ = ((rm_ >> tapbit) & 1u) ? (int)(rm_ & 0xFFFFu) + dt : IMG_ZERO_ROW;                    \
        dst_[i_] = *(const bf16x8*)(smem + r_ * 128 + ((((ks_) * 4 + fq) ^ (r_ & 7)) << 4));                 \
    }
#define AZ_2LDB(dst_, wb_, coff_)                                                                            \
    _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_)                                                         \
        dst_[i_] = *(const bf16x8*)((wb_) + b_row0 + i_ * 2048 + (coff_));
#define AZ_2MMA(mt0_, fb_, fa_)                                                                              \
    _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_)                                                         \
        _Pragma("unroll") for (int j_ = 0; j_ < 4; ++j_)                                                     \
            acc[(mt0_) + i_][j_] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb_[j_], fa_[i_], acc[(mt0_) + i_][j_], 0, 0, 0);
    const int ncb = C / 64;
    const int nk = ncb * 9;
    AZ_2DMA_W(0, 0);
    AZ_2DMA_IMG(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    int cb = 0, tap = 0;
    for (int kt = 0; kt < nk; ++kt) {
        if (kt + 1 < nk) {
            const int ntap = tap == 8 ? 0 : tap + 1, ncbi = tap == 8 ? cb + 1 : cb;
            AZ_2DMA_W(ntap * C + ncbi * 64, (kt + 1) & 1);
        }
        const unsigned char* sW = smem + (kt & 1) * 16384;       // b_row0 already carries the 32 KiB image offset
        const int ky = tap / 3, kx = tap - ky * 3;
        const int dt = (ky - 1) * 7 + (kx - 1);
        const int tapbit = 16 + tap;
        bf16x8 fbX[4], fbY[4], faX[4], faY[4];
        AZ_2LDB(fbX, sW, coffB0);
        AZ_2LDA(faX, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        AZ_2LDA(faY, 4, 0);
        __builtin_amdgcn_sched_barrier(0);
        AZ_2MMA(0, fbX, faX);
        __builtin_amdgcn_sched_barrier(0);
        AZ_2LDB(fbY, sW, coffB1);
        AZ_2LDA(faX, 0, 1);
        __builtin_amdgcn_sched_barrier(0);
        AZ_2MMA(4, fbX, faY);
        __builtin_amdgcn_sched_barrier(0);
        AZ_2LDA(faY, 4, 1);
        __builtin_amdgcn_sched_barrier(0);
        AZ_2MMA(0, fbY, faX);
        __builtin_amdgcn_sched_barrier(0);
        AZ_2MMA(4, fbY, faY);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (++tap == 9) {
            tap = 0;
            ++cb;
            if (cb < ncb) {                    // image switch: everybody is past the barrier, i.e. done with image cb-1
                AZ_2DMA_IMG(cb);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();
            }
        }
    }
#undef AZ_2DMA_W
#undef AZ_2DMA_IMG
#undef AZ_2LDA
#undef AZ_2LDB
#undef AZ_2MMA
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        const int n = n0 + wc * 64 + nt * 16 + fq * 4;
        const float4 bv = *(const float4*)(d.bias + n);
#pragma unroll
        for (int mt = 0; mt < 8; ++mt) {
            const int ml = wr * 128 + mt * 16 + frow;
            const int m = b0 * 42 + ml;
            if (ml >= IMG_ROWS || m >= M) continue;
            float r0 = acc[mt][nt][0] + bv.x, r1 = acc[mt][nt][1] + bv.y, r2 = acc[mt][nt][2] + bv.z,
                  r3 = acc[mt][nt][3] + bv.w;
            if (d.relu) { r0 = fmaxf(r0, 0.f); r1 = fmaxf(r1, 0.f); r2 = fmaxf(r2, 0.f); r3 = fmaxf(r3, 0.f); }
            uint2 o;
            o.x = pack_bf16x2(r0, r1);
            o.y = pack_bf16x2(r2, r3);
            *(uint2*)(d.out + (size_t)m * d.N + n) = o;
        }
    }
}

// ---- 'valid' 3x3 convs (conv3: [6][7][C] -> [4][5][C], conv4: [4][5][C] -> [2][3][C]) image-resident, two 4-wave
// workgroups per CU ---------------------------------------------------------------------------------------------------
// The lockstep argument of k_conv_img2 for the 'valid' convs.  Tile = NB boards (NB*OH*OW output rows, padded to 128 or
// 256) x NCOL channels; every wave owns 128 rows x 64 columns (8 x 4 accumulators, 64 MFMAs per K-step):
//   conv3: NB = 12 (240 of 256 rows), NCOL = 128, waves 2 x 2; LDS = 63 KiB image + 16 KiB weights
//   (conv4: NB = 19 (114 of 128 rows), NCOL = 256, waves 1 x 4, 47.5 KiB image + 32 KiB weights -- measured neutral, not used)
// i.e. 80 KiB = the boards' input image (one buffer) + ONE weight buffer: both 32-deep halves of the step's weight
// fragments are read into registers first, a barrier behind those reads frees the buffer, and the next weight tile is
// DMA'd under the rest of the step.  A 'valid' conv needs no padding logic: output (y, x) of a board reads image row
// (y+ky)*IW + (x+kx).  Same K order: bit-identical.
template <int LAYER, int NB, int IH, int IW, int WN>
__global__ __launch_bounds__(256, 2) void k_conv_valid_img2(const GemmDesc d) {
    constexpr int OH = IH - 2, OW = IW - 2, OUT_PER = OH * OW, IN_PER = IH * IW;
    constexpr int OUT_ROWS = NB * OUT_PER, IMG_R = NB * IN_PER;
    constexpr int NCOL = WN == 4 ? 256 : 128;
    constexpr int IMG_BYTES = (IMG_R * 128 + 1023) / 1024 * 1024;
    constexpr int IPIECES = (IMG_R + 31) / 32, WPIECES = NCOL / 32;       // 1 KiB DMA pieces per wave
    static_assert(IMG_BYTES + NCOL * 128 <= 81920, "two workgroups must fit a CU's 160 KiB");
    __shared__ __attribute__((aligned(16))) unsigned char smem[IMG_BYTES + NCOL * 128];   // img | w
    const int n_boards = (int)(*d.n_dev);
    const int M = n_boards * OUT_PER;
    const int C = d.cin;
    const int NT = d.N / NCOL;
    const int id = blockIdx.x;
    const int xcd = id & 7, j = id >> 3;
    const int ntile = j % NT, mtile = (j / NT) * 8 + xcd;
    const int b0 = mtile * NB, n0 = ntile * NCOL;
    if (b0 >= n_boards) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = WN == 4 ? 0 : wave >> 1, wc = WN == 4 ? wave : wave & 1;
    const int lrow = lane >> 3;
    const int chunk = (lane & 7) ^ lrow;
    // image DMA: piece q of wave w = LDS rows (q*4 + w)*8 + lrow of the NB boards' IN_PER input rows each
    uint32_t i_ob[IPIECES];
#pragma unroll
    for (int q = 0; q < IPIECES; ++q) {
        int r = (q * 4 + wave) * 8 + lrow;
        r = r < IMG_R ? r : IMG_R - 1;
        int g = b0 * IN_PER + r;
        g = g < n_boards * IN_PER ? g : n_boards * IN_PER - 1;
        i_ob[q] = (uint32_t)(g * C + chunk * 8) * 2u;
    }
    // weight DMA: piece q of wave w = tile rows (q*4 + w)*8 + lrow
    const uint32_t b_ob0 = (uint32_t)((n0 + wave * 8 + lrow) * d.K + chunk * 8) * 2u;
    const uint32_t b_stepb = 64u * (uint32_t)d.K;                        // 32 weight rows, in bytes
    typedef __attribute__((address_space(3))) void* lds_ptr;
    typedef const __attribute__((address_space(1))) void* gbl_ptr;
#define AZ_3DMA_W(kk_)                                                                                       \
    {                                                                                                        \
        unsigned char* lb = smem + IMG_BYTES + wave * 1024;                                                  \
        const char* wbase = (const char*)(d.W + (kk_));                                                      \
        _Pragma("unroll") for (int q_ = 0; q_ < WPIECES; ++q_)                                               \
            __builtin_amdgcn_global_load_lds((gbl_ptr)(wbase + b_ob0 + (uint32_t)q_ * b_stepb), (lds_ptr)(lb + q_ * 4096), 16, 0, 0); \
    }
#define AZ_3DMA_IMG(cb_)                                                                                     \
    {                                                                                                        \
        unsigned char* la = smem + wave * 1024;                                                              \
        const char* ibase = (const char*)(d.A + (cb_) * 64);                                                 \
        _Pragma("unroll") for (int q_ = 0; q_ < IPIECES; ++q_)                                               \
            if ((q_ * 4 + wave) * 8 + lrow < IMG_R)                                                          \
                __builtin_amdgcn_global_load_lds((gbl_ptr)(ibase + i_ob[q_]), (lds_ptr)(la + q_ * 4096), 16, 0, 0); \
    }
    f32x4 acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int jn = 0; jn < 4; ++jn) acc[i][jn] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int frow = lane & 15, fq = lane >> 4, fsw = lane & 7;
    int rbase[8];                       // image row of tap (0,0) for this lane's row of each of the 8 row tiles
#pragma unroll
    for (int mt = 0; mt < 8; ++mt) {
        int ml = wr * 128 + mt * 16 + frow;
        ml = ml < OUT_ROWS ? ml : 0;
        const int bl = ml / OUT_PER, p = ml - bl * OUT_PER, y = p / OW, x = p - y * OW;
        rbase[mt] = bl * IN_PER + y * IW + x;
    }
    const int b_row0 = IMG_BYTES + (wc * 64 + frow) * 128;
    const int coffB0 = ((0 + fq) ^ fsw) << 4, coffB1 = ((4 + fq) ^ fsw) << 4;
#define AZ_3LDA(dst_, mt0_, ks_)                                                                             \
    _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_) {                                                       \
        const int r_ = rbase[(mt0_) + i_] + dt;                                                              \
        dst_[i_] = *(const bf16x8*)(smem + r_ * 128 + ((((ks_) * 4 + fq) ^ (r_ & 7)) << 4));                 \
    }
#define AZ_3LDB(dst_, coff_)                                                                                 \
    _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_)                                                         \
        dst_[i_] = *(const bf16x8*)(smem + b_row0 + i_ * 2048 + (coff_));
#define AZ_3MMA(mt0_, fb_, fa_)                                                                              \
    _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_)                                                         \
        _Pragma("unroll") for (int j_ = 0; j_ < 4; ++j_)                                                     \
            acc[(mt0_) + i_][j_] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb_[j_], fa_[i_], acc[(mt0_) + i_][j_], 0, 0, 0);
    const int ncb = C / 64;
    const int nk = ncb * 9;
    AZ_3DMA_W(0);
    AZ_3DMA_IMG(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    int cb = 0, tap = 0;
    for (int kt = 0; kt < nk; ++kt) {
        const int ky = tap / 3, kx = tap - ky * 3;
        const int dt = ky * IW + kx;
        bf16x8 fbX[4], fbY[4], faX[4], faY[4];
        AZ_3LDB(fbX, coffB0);
        AZ_3LDB(fbY, coffB1);
        AZ_3LDA(faX, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");       // the step's weight fragments are in registers: free the buffer
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        if (kt + 1 < nk) {
            const int ntap = tap == 8 ? 0 : tap + 1, ncbi = tap == 8 ? cb + 1 : cb;
            AZ_3DMA_W(ntap * C + ncbi * 64);
        }
        AZ_3LDA(faY, 4, 0);
        __builtin_amdgcn_sched_barrier(0);
        AZ_3MMA(0, fbX, faX);
        __builtin_amdgcn_sched_barrier(0);
        AZ_3LDA(faX, 0, 1);
        __builtin_amdgcn_sched_barrier(0);
        AZ_3MMA(4, fbX, faY);
        __builtin_amdgcn_sched_barrier(0);
        AZ_3LDA(faY, 4, 1);
        __builtin_amdgcn_sched_barrier(0);
        AZ_3MMA(0, fbY, faX);
        __builtin_amdgcn_sched_barrier(0);
        AZ_3MMA(4, fbY, faY);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        if (++tap == 9) {
            tap = 0;
            ++cb;
            if (cb < ncb) {                    // image switch (single buffer): covered by the CU's other workgroup
                AZ_3DMA_IMG(cb);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();
            }
        }
    }
#undef AZ_3DMA_W
#undef AZ_3DMA_IMG
#undef AZ_3LDA
#undef AZ_3LDB
#undef AZ_3MMA
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        const int n = n0 + wc * 64 + nt * 16 + fq * 4;
        const float4 bv = *(const float4*)(d.bias + n);
#pragma unroll
        for (int mt = 0; mt < 8; ++mt) {
            const int ml = wr * 128 + mt * 16 + frow;
            const int m = b0 * OUT_PER + ml;
            if (ml >= OUT_ROWS || m >= M) continue;
            float r0 = acc[mt][nt][0] + bv.x, r1 = acc[mt][nt][1] + bv.y, r2 = acc[mt][nt][2] + bv.z,
                  r3 = acc[mt][nt][3] + bv.w;
            if (d.relu) { r0 = fmaxf(r0, 0.f); r1 = fmaxf(r1, 0.f); r2 = fmaxf(r2, 0.f); r3 = fmaxf(r3, 0.f); }
            uint2 o;
            o.x = pack_bf16x2(r0, r1);
            o.y = pack_bf16x2(r2, r3);
            *(uint2*)(d.out + (size_t)m * d.N + n) = o;
        }
    }
}

// ---- the same tile with the LDS-DMA issued from inline asm and a software-pipelined K-step ---------------------------
// hipcc models `__builtin_amdgcn_global_load_lds` as a FLAT access that may touch LDS and global memory at once: while one
// is pending EVERY s_waitcnt it inserts is vmcnt(0) / lgkmcnt(0), so in k_conv_valid_img2 each MFMA cluster waits for the
// fragment reads issued just before it (meant for the NEXT cluster) -- three exposed LDS latencies per K-step.  Issued
// from inline asm (saddr form: uniform base in SGPRs + one loop-invariant 32-bit offset VGPR per piece, LDS base in M0)
// the compiler does not see the DMA, its own lgkmcnt waits become counted, and the waits for the DMA are the explicit
// vmcnt(0) + barrier pairs below.  K-step schedule (fbX / faX of step k were requested under step k-1's last cluster):
//   reads fbY, faY(ks0) | MFMA fbX x faX(ks0) | lgkmcnt(0), barrier: W(k) is in registers everywhere | DMA W(k+1)
//   reads faX(ks1) | MFMA fbX x faY(ks0) | reads faY(ks1) | MFMA fbY x faX(ks1) | vmcnt(0), barrier: W(k+1) landed
//   reads fbX, faX(ks0) of step k+1 | MFMA fbY x faY(ks1)
// Same K order per accumulator as k_conv_valid_img2 (and every other conv3 kernel): bit-identical.

template <int LAYER, int NB, int IH, int IW, bool STAMP = false, bool IL = false>   // IL: fragment reads interleaved into the MFMA clusters (sched_group_barrier); STAMP: per-segment s_memtime sums of wave 0 into d.dbg (same results)
__global__ __launch_bounds__(256, 2) void k_conv_valid_pipe(const GemmDesc d) {
    constexpr int OH = IH - 2, OW = IW - 2, OUT_PER = OH * OW, IN_PER = IH * IW;
    constexpr int OUT_ROWS = NB * OUT_PER, IMG_R = NB * IN_PER;
    constexpr int NCOL = 128;
    constexpr int IMG_BYTES = (IMG_R * 128 + 1023) / 1024 * 1024;
    constexpr int IPIECES = (IMG_R + 31) / 32, WPIECES = NCOL / 32;       // 1 KiB DMA pieces per wave
    static_assert(IMG_BYTES + NCOL * 128 <= 81920, "two workgroups must fit a CU's 160 KiB");
    static_assert(IMG_R % 8 == 0 && NB <= 16, "whole 8-row DMA sub-pieces; NetWorkspace keeps 16 boards of slack");
    __shared__ __attribute__((aligned(16))) unsigned char smem[IMG_BYTES + NCOL * 128];   // img | w
    const int n_boards = (int)(*d.n_dev);
    const int M = n_boards * OUT_PER;
    if (M <= d.m_min) return;                          // the small-batch kernel launched beside this one takes the batch
    const int C = d.cin;
    const int NT = d.N / NCOL;
    const int id = blockIdx.x;
    const int xcd = id & 7, j = id >> 3;
    const int ntile = j % NT, mtile = (j / NT) * 8 + xcd;
    const int b0 = mtile * NB, n0 = ntile * NCOL;
    if (b0 >= n_boards) return;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    const int lrow = lane >> 3;
    const int chunk = (lane & 7) ^ lrow;
    typedef __attribute__((address_space(3))) void* lds_ptr;
    // DMA addresses: one loop-invariant 32-bit lane offset per operand; piece q adds a uniform stride to the SGPR base.  Image rows
    // past the batch's last board are read unclamped (the workspace keeps 16 boards of slack; their output rows are never stored).
    const uint32_t i_ob = (uint32_t)((b0 * IN_PER + wave * 8 + lrow) * C + chunk * 8) * 2u;
    const uint32_t w_ob = (uint32_t)((n0 + wave * 8 + lrow) * d.K + chunk * 8) * 2u;
    const uint32_t lds_img = (uint32_t)(uintptr_t)(lds_ptr)(smem + wave * 1024);
    const uint32_t lds_w = (uint32_t)(uintptr_t)(lds_ptr)(smem + IMG_BYTES + wave * 1024);
    const size_t i_stride = (size_t)64 * C, w_stride = (size_t)64 * d.K;          // 32 rows, in bytes
#define AZ_PDMA_W(kk_)                                                                                       \
    {                                                                                                        \
        const char* wbase = (const char*)(d.W + (kk_));                                                      \
        _Pragma("unroll") for (int q_ = 0; q_ < WPIECES; ++q_) lds_dma16(wbase + q_ * w_stride, w_ob, lds_w + q_ * 4096); \
    }
#define AZ_PDMA_IMG(cb_)                                                                                     \
    {                                                                                                        \
        const char* ibase = (const char*)(d.A + (cb_) * 64);                                                 \
        _Pragma("unroll") for (int q_ = 0; q_ < IPIECES; ++q_)                                               \
            if ((q_ * 4 + 3) * 8 + 7 < IMG_R || (q_ * 4 + wave) * 8 + 7 < IMG_R)                             \
                lds_dma16(ibase + q_ * i_stride, i_ob, lds_img + q_ * 4096);                                 \
    }
    f32x4 acc[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int jn = 0; jn < 4; ++jn) acc[i][jn] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int frow = lane & 15, fq = lane >> 4, fsw = lane & 7;
    int rbase[8];
#pragma unroll
    for (int mt = 0; mt < 8; ++mt) {
        int ml = wr * 128 + mt * 16 + frow;
        ml = ml < OUT_ROWS ? ml : 0;
        const int bl = ml / OUT_PER, p = ml - bl * OUT_PER, y = p / OW, x = p - y * OW;
        rbase[mt] = bl * IN_PER + y * IW + x;
    }
    const int b_row0 = IMG_BYTES + (wc * 64 + frow) * 128;
    const int coffB0 = ((0 + fq) ^ fsw) << 4, coffB1 = ((4 + fq) ^ fsw) << 4;
#define AZ_PLDA(dst_, mt0_, ks_, dt_)                                                                        \
    _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_) {              \
        const int r_ = rbase[(mt0_) + i_] + (dt_);                                                           \
        dst_[i_] = *(const bf16x8*)(smem + r_ * 128 + ((((ks_) * 4 + fq) ^ (r_ & 7)) << 4));                 \
    }
#define AZ_PLDB(dst_, coff_)                                                                                 \
    _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_)                               \
        dst_[i_] = *(const bf16x8*)(smem + b_row0 + i_ * 2048 + (coff_));
#define AZ_PMMA(mt0_, fb_, fa_)                                                                              \
    _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_)                                                         \
        _Pragma("unroll") for (int j_ = 0; j_ < 4; ++j_)                                                     \
            acc[(mt0_) + i_][j_] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb_[j_], fa_[i_], acc[(mt0_) + i_][j_], 0, 0, 0);
#define AZ_PSB __builtin_amdgcn_sched_barrier(0)
#define AZ_PFENCE if constexpr (!IL) __builtin_amdgcn_sched_barrier(0)
    // IL: the region's reads (for the NEXT cluster) go between this cluster's MFMAs: rep_ x { nmf_ MFMAs, 1 LDS read }
#define AZ_PMIX(nmf_, rep_, tail_)                                                                           \
    if constexpr (IL) {                                                                                      \
        _Pragma("unroll") for (int g_ = 0; g_ < (rep_); ++g_) {                                              \
            __builtin_amdgcn_sched_group_barrier(0x008, (nmf_), 0);                                          \
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);                                               \
        }                                                                                                    \
        if ((tail_) > 0) __builtin_amdgcn_sched_group_barrier(0x008, (tail_), 0);                            \
    }
    AZ_PDMA_W(0);
    AZ_PDMA_IMG(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    bf16x8 fbX[4], fbY[4], faX[4], faY[4];
    AZ_PLDB(fbX, coffB0);
    AZ_PLDA(faX, 0, 0, 0);
    const int ncb = C / 64;
    const int nk = ncb * 9;
    int cb = 0, tap = 0, dt = 0;
    unsigned long long seg[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tprev = 0, t_begin = 0, r_begin = 0;
    if constexpr (STAMP) { t_begin = tprev = __builtin_amdgcn_s_memtime(); r_begin = __builtin_amdgcn_s_memrealtime(); }
#define AZ_PSTAMP(i_) if constexpr (STAMP) { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); seg[i_] += t_ - tprev; tprev = t_; }
    for (int kt = 0; kt < nk; ++kt) {
        const bool sw = tap == 8;
        const int ntap = sw ? 0 : tap + 1, ncbi = sw ? cb + 1 : cb;
        const int nky = ntap / 3, ndt = nky * IW + (ntap - nky * 3);
        const int kk = kt + 1 < nk ? ntap * C + ncbi * 64 : 8 * C + cb * 64;      // last step: re-fetch its own tile (unused)
        AZ_PLDB(fbY, coffB1);
        AZ_PLDA(faY, 4, 0, dt);
        AZ_PFENCE;
        AZ_PMMA(0, fbX, faX);
        AZ_PMIX(1, 8, 8);
        AZ_PSB;
        AZ_PSTAMP(0);
        __builtin_amdgcn_s_waitcnt(0xC07F);                      // lgkmcnt(0): this step's weight fragments are in registers
        __builtin_amdgcn_s_barrier();
        AZ_PSB;
        AZ_PSTAMP(1);
        AZ_PDMA_W(kk);
        AZ_PSTAMP(2);
        AZ_PLDA(faX, 0, 1, dt);
        AZ_PFENCE;
        AZ_PMMA(4, fbX, faY);
        AZ_PMIX(2, 4, 8);
        AZ_PSB;
        AZ_PSTAMP(3);
        AZ_PLDA(faY, 4, 1, dt);
        AZ_PFENCE;
        AZ_PMMA(0, fbY, faX);
        AZ_PMIX(2, 4, 8);
        AZ_PSB;
        AZ_PSTAMP(4);
        __builtin_amdgcn_s_waitcnt(0xC07F);                      // my reads of the image slice are done (they are: one cluster old)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");         // the next weight tile has landed
        __builtin_amdgcn_s_barrier();
        AZ_PSB;
        AZ_PSTAMP(5);
        if (sw && ncbi < ncb) {                                  // single image buffer: the switch is covered by the CU's other workgroup
            AZ_PDMA_IMG(ncbi);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
        }
        AZ_PSB;
        AZ_PSTAMP(6);
        AZ_PLDB(fbX, coffB0);                                    // next step's first fragments, under this step's last cluster
        AZ_PLDA(faX, 0, 0, ndt);
        AZ_PFENCE;
        AZ_PMMA(4, fbY, faY);
        AZ_PMIX(1, 8, 8);
        AZ_PSB;
        AZ_PSTAMP(7);
        tap = ntap; cb = ncbi; dt = ndt;
    }
    if constexpr (STAMP) {
        if (tid == 0 && d.dbg && blockIdx.x < 128) {
            for (int i = 0; i < 8; ++i) d.dbg[16 * blockIdx.x + i] = seg[i];
            d.dbg[16 * blockIdx.x + 8] = __builtin_amdgcn_s_memtime() - t_begin;
            d.dbg[16 * blockIdx.x + 9] = __builtin_amdgcn_s_memrealtime() - r_begin;
        }
    }
#undef AZ_PSTAMP
#undef AZ_PDMA_W
#undef AZ_PDMA_IMG
#undef AZ_PLDA
#undef AZ_PLDB
#undef AZ_PMMA
#undef AZ_PSB
#undef AZ_PFENCE
#undef AZ_PMIX
    // Epilogue through LDS: a lane holds 4 consecutive channels of 32 (row tile, column tile) pairs -- stored directly that is 32
    // eight-byte stores per lane in 32-byte pieces of 16 different rows each (7 % of the kernel at 3072 rows).  The image and weight
    // buffers are dead now: the tile (+ bias, ReLU, bf16) goes to LDS as [240 rows][128 channels] with a 272-byte row stride
    // (conflict-free for both directions), and leaves as whole 256-byte row segments, 16 bytes per lane.
    constexpr int EP_STRIDE = NCOL * 2 + 16;
    static_assert(OUT_ROWS * EP_STRIDE <= IMG_BYTES + NCOL * 128, "the output tile must fit the dead buffers");
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_s_barrier();                     // every wave is past its last fragment read (and the unused last DMA has landed)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        const int nl = wc * 64 + nt * 16 + fq * 4;
        const float4 bv = *(const float4*)(d.bias + n0 + nl);
#pragma unroll
        for (int mt = 0; mt < 8; ++mt) {
            const int ml = wr * 128 + mt * 16 + frow;
            if (ml >= OUT_ROWS) continue;
            float r0 = acc[mt][nt][0] + bv.x, r1 = acc[mt][nt][1] + bv.y, r2 = acc[mt][nt][2] + bv.z,
                  r3 = acc[mt][nt][3] + bv.w;
            if (d.relu) { r0 = fmaxf(r0, 0.f); r1 = fmaxf(r1, 0.f); r2 = fmaxf(r2, 0.f); r3 = fmaxf(r3, 0.f); }
            uint2 o;
            o.x = pack_bf16x2(r0, r1);
            o.y = pack_bf16x2(r2, r3);
            *(uint2*)(smem + ml * EP_STRIDE + nl * 2) = o;
        }
    }
    __syncthreads();
    constexpr int EP_CHUNKS = OUT_ROWS * (NCOL / 8);        // 16-byte chunks of the tile
#pragma unroll
    for (int it = 0; it < (EP_CHUNKS + 255) / 256; ++it) {
        const int idx = it * 256 + tid;
        const int ml = idx / (NCOL / 8), c = idx - ml * (NCOL / 8);
        const int m = b0 * OUT_PER + ml;
        if (idx >= EP_CHUNKS || m >= M) continue;
        *(uint4*)(d.out + (size_t)m * d.N + n0 + c * 8) = *(const uint4*)(smem + ml * EP_STRIDE + c * 16);
    }
}
