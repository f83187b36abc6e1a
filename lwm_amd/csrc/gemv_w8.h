// gemv_w8.h -- 8-bit (OCP e4m3fn) decode weights: the quantiser and the weight format of the GEMV that streams them.
// Requires wave_ops.h + gemv.h (GemvParams, gemv_body, gemv_by_rows, gemv_reduce_kernel) + attn_decode.h (unpack_bf16x8,
// f32x2, fma2, global_load_b64) + attn_decode_kv8.h (cvt_e4m3x2_lo/hi, pack_e4m3x4).
//
// Why: the projections of a cached-decode step stream every weight once per token (gemv.h); the bf16 kernel is
// HBM-bound, so the lever left is the number of bytes.  Per (K, N) kernel the pack holds K * N e4m3 bytes and one f32
// scale per 128 rows of K and column: 0.516 of the bf16 bytes.
//
// Format (include/lwm_hip.h, "8-bit decode weights"):
//   q      uint8 (K, N)             e4m3fn bit patterns, row-major as the GEMV reads W
//   scale  f32   (ceil(K/128), N)   one power-of-two scale per K tile of one GEMV partial (kGemvKT rows) and column
//   amax over the rows of the group that exist; s = the smallest power of two with amax / s <= 448, clamped to
//   [2^-126, 2^127] (amax == 0: s = 1); q = e4m3(w / s), round to nearest even.
//
// Why the bits agree with the bf16 kernel on the rounded weights e4m3(q) * s: both kernels are gemv_body (one K partition,
// one order of every fmaf chain and of the wave sum), and with a power-of-two s (no overflow, no underflow)
// fmaf(x, q * s, a * s) == s * fmaf(x, q, a) -- so multiplying the summed tile by s once gives the bf16 kernel's partial.
#pragma once

namespace lwm {

// Column tile: gemv.h's -- lane l owns columns 8l..8l+7, now one 8-byte load per row.  16 columns per lane (16-byte loads,
// 1 KiB per wave load) was built first: 64 accumulators + 32 load registers at four rows came to 123 VGPRs (4 waves per
// SIMD, under the bf16 kernel's 5) and 48 KiB of LDS per workgroup (3 workgroups per CU), i.e. the SAME bytes in flight per
// CU as this tile at its occupancy, from half as many workgroups (wo: 128 for 256 CUs).
constexpr int kGemvW8CPL = 8;                   // columns per lane = bytes per load
constexpr int kGemvW8NT = 64 * kGemvW8CPL;      // columns of W per workgroup (= kGemvNT)

static_assert(kGemvW8NT == kGemvNT && kGemvW8CPL == 8, "gemv_body's column tile");

struct GemvW8Params {
    GemvParams g;                          // w[] unused; everything else as the bf16 kernel has it (the reduce kernel takes g)
    const uint8_t* q[kGemvMaxMats];        // [K, N_i] e4m3 bytes
    const float* scale[kGemvMaxMats];      // [KS, N_i]
};

// The e4m3 weight format of gemv_body (gemv.h): one 8-byte load per row, the accumulators as pairs (columns 2j, 2j+1 of the
// lane's 8) for the packed FMAs, one multiply by the group's scale when the partial is finished.
struct GemvW8Format {
    using Params = GemvW8Params;
    using Elem = uint8_t;
    using Load = u32x2;
    using Acc = f32x2[4];
    static constexpr bool kScaled = true, kWaveScaled = false;
    static constexpr int kRows = 1;
    LWM_DEVICE static const GemvParams& g(const Params& p) { return p.g; }
    LWM_DEVICE static const Elem* matrix(const Params& p, int mi) { return p.q[mi]; }
    LWM_DEVICE static int64_t offset(int k, int n, int N) { return (int64_t)k * N + n; }
    LWM_DEVICE static Load load(const Elem* at) { return global_load_b64(at); }
    LWM_DEVICE static void zero(Acc& a) {
        for (int j = 0; j < 4; ++j) a[j] = f32x2{0.0f, 0.0f};
    }
    template <int R>
    LWM_DEVICE static void fma(Acc (&a)[R], const Load& w, const float (&xv)[R], int i) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const f32x2 lo = cvt_e4m3x2_lo(w[c]), hi = cvt_e4m3x2_hi(w[c]);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const float xs = lane_value(xv[r], i);
                const f32x2 x2 = {xs, xs};
                a[r][2 * c] = fma2(x2, lo, a[r][2 * c]);
                a[r][2 * c + 1] = fma2(x2, hi, a[r][2 * c + 1]);
            }
        }
    }
    LWM_DEVICE static f32x4 quad(const Acc& a, int j) { return f32x4{a[2 * j][0], a[2 * j][1], a[2 * j + 1][0], a[2 * j + 1][1]}; }
    LWM_DEVICE static f32x4 scale(const Params& p, int mi, int64_t at) { return global_load_f32x4(p.scale[mi] + at); }
};

// dynamic LDS: 3 * R * kGemvW8NT * 4 bytes (the host sizes it by the row count)
LWM_KERNEL(kGemvThreads) void gemv_w8_kernel(GemvW8Params p) { gemv_by_rows<GemvW8Format>(p); }

// ------------------------------------------------------------------ quantiser
struct W8QuantParams {
    const bf16_t* w;           // [K, N] bf16
    uint8_t* q;                // [K, N] e4m3 bytes
    float* scale;              // [ceil(K / 128), N]
    bf16_t* rounded;           // [K, N] bf16(e4m3(q) * s); may be w itself
    int32_t K, N;              // K % 32 == 0, N % 8 == 0
};

constexpr int kW8QuantNT = 512;        // columns per workgroup: lane l owns columns 8l..8l+7 (one 16-byte load per row)

// Workgroup = one scale group (128 rows of K) x 512 columns; wave w holds rows 32w..32w+31 of its lanes' columns in
// registers (W is read once), the four waves' column maxima meet in LDS, every thread derives the scales of its 8 columns
// and converts the rows it holds.  K % 32 == 0: a wave's rows exist or do not as a whole.  Every thread loads all its rows
// before it stores any, so `rounded` may be `w`.
LWM_KERNEL(256) void w8_quantise_kernel(W8QuantParams p) {
    const lds_t lds = dyn_lds();
    const int tid = thread_idx();
    const int wave = wave_uniform(tid >> 6), lane = tid & 63;
    const int nbn = (p.N + kW8QuantNT - 1) / kW8QuantNT;
    const int grp = block_idx_x() / nbn, nb = block_idx_x() % nbn;
    const int k0 = grp * kGemvKT + wave * kGemvRPW;
    const bool k_ok = k0 < p.K;
    int n = nb * kW8QuantNT + lane * 8;
    const bool n_ok = n < p.N;
    n = n_ok ? n : p.N - 8;                        // (clamped: the loads stay inside the matrix)
    const int64_t base = (int64_t)(k_ok ? k0 : 0) * p.N + n;
    u32x4 wv[kGemvRPW];
#pragma unroll
    for (int i = 0; i < kGemvRPW; ++i) wv[i] = global_load_b128(p.w + base + (int64_t)i * p.N);
    // |w| as integers: bf16 magnitudes order like their bit patterns (and no denormal mode has a say)
    int am[8];
    for (int j = 0; j < 8; ++j) am[j] = 0;
#pragma unroll
    for (int i = 0; i < kGemvRPW; ++i)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int lo = (int)(wv[i][c] & 0x7fffu), hi = (int)((wv[i][c] >> 16) & 0x7fffu);
            am[2 * c] = lo > am[2 * c] ? lo : am[2 * c];
            am[2 * c + 1] = hi > am[2 * c + 1] ? hi : am[2 * c + 1];
        }
    const lds_t mine = lds + (uint32_t)(wave * 64 + lane) * 32;
    lds_write_b128(mine, k_ok ? u32x4{(uint32_t)am[0], (uint32_t)am[1], (uint32_t)am[2], (uint32_t)am[3]} : u32x4{0, 0, 0, 0});
    lds_write_b128(mine + 16, k_ok ? u32x4{(uint32_t)am[4], (uint32_t)am[5], (uint32_t)am[6], (uint32_t)am[7]} : u32x4{0, 0, 0, 0});
    block_sync();
    for (int j = 0; j < 8; ++j) am[j] = 0;
    for (int w = 0; w < 4; ++w) {
        const u32x4 a = lds_read_u32x4(lds + (uint32_t)(w * 64 + lane) * 32), b = lds_read_u32x4(lds + (uint32_t)(w * 64 + lane) * 32 + 16);
        for (int j = 0; j < 4; ++j) {
            am[j] = (int)a[j] > am[j] ? (int)a[j] : am[j];
            am[4 + j] = (int)b[j] > am[4 + j] ? (int)b[j] : am[4 + j];
        }
    }
    // amax = 1.m * 2^e: the smallest power of two s with amax / s <= 448 = 1.75 * 2^8 is 2^(e-8) when 1.m <= 1.75 and
    // 2^(e-7) otherwise.  Biased exponent of s, clamped to 2^-126 below (finite bf16 inputs stay under the upper clamp of
    // 2^127 by themselves: e <= 127 gives s <= 2^120).
    float s[8], inv[8];
    for (int j = 0; j < 8; ++j) {
        int se = 127;
        if (am[j] != 0) {
            se = (am[j] >> 7) - 8 + ((am[j] & 0x7f) > 0x60 ? 1 : 0);
            se = se < 1 ? 1 : se;
        }
        s[j] = __builtin_bit_cast(float, (uint32_t)se << 23);
        inv[j] = __builtin_bit_cast(float, (uint32_t)(254 - se) << 23);
    }
    if (n_ok && wave == 0) {
        float* sp = p.scale + (int64_t)grp * p.N + n;
        global_store_f32x4(sp, f32x4{s[0], s[1], s[2], s[3]});
        global_store_f32x4(sp + 4, f32x4{s[4], s[5], s[6], s[7]});
    }
    if (!(n_ok && k_ok)) return;
#pragma unroll
    for (int i = 0; i < kGemvRPW; ++i) {
        float x[8];
        unpack_bf16x8(wv[i], x);
        u32x2 b;
        b[0] = pack_e4m3x4(x[0] * inv[0], x[1] * inv[1], x[2] * inv[2], x[3] * inv[3]);
        b[1] = pack_e4m3x4(x[4] * inv[4], x[5] * inv[5], x[6] * inv[6], x[7] * inv[7]);
        global_store_b64(p.q + base + (int64_t)i * p.N, b);
        u32x4 o;
        for (int c = 0; c < 2; ++c) {
            const f32x2 lo = cvt_e4m3x2_lo(b[c]), hi = cvt_e4m3x2_hi(b[c]);
            o[2 * c] = pack_bf16x2(lo[0] * s[4 * c], lo[1] * s[4 * c + 1]);
            o[2 * c + 1] = pack_bf16x2(hi[0] * s[4 * c + 2], hi[1] * s[4 * c + 3]);
        }
        global_store_b128(p.rounded + base + (int64_t)i * p.N, o);
    }
}

}  // namespace lwm
