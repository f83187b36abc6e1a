// gemv_w4.h -- 4-bit (OCP MXFP4: e2m1 codes, one e8m0 scale per 32 rows of K) decode weights: the quantiser and the weight
// format of the GEMV that streams them.  Requires wave_ops.h + gemv.h (GemvParams, gemv_body, gemv_by_rows,
// gemv_reduce_kernel) + attn_decode.h (unpack_bf16x8, f32x2, fma2, global_load_b64) + attn_decode_kv4.h (cvt_e2m1x2,
// e8m0_to_f32, Kv4Format: encode, kExpDrop, kMantTop).
//
// Why: gemv_w8.h halved the bytes a cached-decode step streams; this pack halves them again.  Per (K, N) kernel it holds
// K * N / 2 bytes of codes and one scale byte per 32 rows of K and column: 4.25 bits per weight, 0.266 of the bf16 bytes.
//
// Format (include/lwm_hip.h, "4-bit decode weights"):
//   q      uint8 (K/4, N/8, 16)   e2m1 codes, two per byte.  Slot [k4][n8] is 16 bytes = rows 4 k4 .. 4 k4 + 3 of columns
//                                 8 n8 .. 8 n8 + 7: dword j of the slot is row 4 k4 + j, byte b of that dword holds column
//                                 8 n8 + 2b in its low nibble and column 8 n8 + 2b + 1 in its high nibble
//   scale  uint8 (K/32, N)        one e8m0 byte b per MX block = 32 consecutive rows of K of one column: the scale 2^(b-127)
//   amax over the block; s = the smallest power of two with amax / s <= 6, its exponent byte clamped to [1, 254]
//   (amax == 0: byte 127); q = e2m1(w / s), round to nearest, ties to the even code -- attn_decode_kv4.h's rule.
//
// The slot is what one lane of gemv_body loads at a time (lane l owns columns 8l..8l+7): one 16-byte load brings four rows,
// a wave load is still 1 KiB contiguous, and the wave's 32 rows are the 8 loads the bf16 kernel keeps in flight.
//
// Why the bits agree with the bf16 kernel on the rounded weights e2m1(q) * s: the MX block is the 32 rows one wave walks
// (kGemvRPW), so each column of a wave's sum sees ONE scale.  Both kernels are gemv_body (one K partition, one order of
// every fmaf chain), and with a power-of-two s (no overflow, no underflow) fmaf(x, q * s, a * s) == s * fmaf(x, q, a) --
// so multiplying the finished wave sum by s once, before the sums meet in LDS, gives the bf16 kernel's wave sum.
#pragma once

namespace lwm {

static_assert(kGemvRPW == 32, "an MX block is the rows of one wave of gemv_body");

struct GemvW4Params {
    GemvParams g;                          // w[] unused; everything else as the bf16 kernel has it (the reduce kernel takes g)
    const uint8_t* q[kGemvMaxMats];        // [K/4, N_i/8, 16] e2m1 nibble pairs
    const uint8_t* scale[kGemvMaxMats];    // [K/32, N_i] e8m0 bytes
};

// The e2m1 weight format of gemv_body (gemv.h): one 16-byte load per four rows, the conversions with scale 1, the
// accumulators as pairs (columns 2j, 2j+1 of the lane's 8) for the packed FMAs as GemvW8Format has them, and one multiply
// by the block's scale per finished wave sum.
struct GemvW4Format {
    using Params = GemvW4Params;
    using Elem = uint8_t;
    using Load = u32x4;
    using Acc = f32x2[4];
    static constexpr bool kScaled = false, kWaveScaled = true;
    static constexpr int kRows = 4;
    LWM_DEVICE static const GemvParams& g(const Params& p) { return p.g; }
    LWM_DEVICE static const Elem* matrix(const Params& p, int mi) { return p.q[mi]; }
    // bytes: slot [k / 4][n / 8] of 16 (k % 4 == 0, n % 8 == 0)
    LWM_DEVICE static int64_t offset(int k, int n, int N) { return ((int64_t)k * N >> 1) + 2 * n; }
    LWM_DEVICE static Load load(const Elem* at) { return global_load_b128(at); }
    LWM_DEVICE static void zero(Acc& a) {
        for (int j = 0; j < 4; ++j) a[j] = f32x2{0.0f, 0.0f};
    }
    template <int R>
    LWM_DEVICE static void row(Acc (&a)[R], uint32_t w, const float (&xv)[R], int i) {
        const f32x2 c[4] = {cvt_e2m1x2<0>(w), cvt_e2m1x2<1>(w), cvt_e2m1x2<2>(w), cvt_e2m1x2<3>(w)};
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float xs = lane_value(xv[r], i);
            const f32x2 x2 = {xs, xs};
#pragma unroll
            for (int j = 0; j < 4; ++j) a[r][j] = fma2(x2, c[j], a[r][j]);
        }
    }
    template <int R>
    LWM_DEVICE static void fma(Acc (&a)[R], const Load& w, const float (&xv)[R], int i) {
#pragma unroll
        for (int j = 0; j < kRows; ++j) row(a, w[j], xv, i + j);
    }
    LWM_DEVICE static f32x4 quad(const Acc& a, int j) { return f32x4{a[2 * j][0], a[2 * j][1], a[2 * j + 1][0], a[2 * j + 1][1]}; }
    LWM_DEVICE static u32x2 wave_scale(const Params& p, int mi, int64_t at) { return global_load_b64(p.scale[mi] + at); }
    LWM_DEVICE static void scale_wave(Acc& a, const u32x2& b) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t two = b[j >> 1] >> (16 * (j & 1));
            a[j] = a[j] * f32x2{e8m0_to_f32(two & 255u), e8m0_to_f32((two >> 8) & 255u)};
        }
    }
};

// dynamic LDS: 3 * R * kGemvNT * 4 bytes (the host sizes it by the row count)
LWM_KERNEL(kGemvThreads) void gemv_w4_kernel(GemvW4Params p) { gemv_by_rows<GemvW4Format>(p); }

// ------------------------------------------------------------------ quantiser (the 4-bit and the 6-bit one: gemv_w6.h)
struct MxQuantParams {
    const bf16_t* w;           // [K, N] bf16
    uint8_t* q;                // [K/4, N/8, slot bytes] codes: 16 bytes of e2m1 nibble pairs, 24 bytes of e2m3 codes
    uint8_t* scale;            // [K/32, N] e8m0 bytes
    bf16_t* rounded;           // [K, N] bf16(code(q) * s); may be w itself
    int32_t K, N;              // K % 32 == 0, N % 8 == 0
};
typedef MxQuantParams W4QuantParams;

constexpr int kW4QuantNT = 512;        // columns per workgroup: lane l owns columns 8l..8l+7 (one 16-byte load per row)

// x = one row of the lane's 8 columns over its blocks' scales
LWM_DEVICE void mx_quant_scaled(const u32x4& w, const float (&inv)[8], float (&x)[8]) {
    unpack_bf16x8(w, x);
    for (int c = 0; c < 8; ++c) x[c] *= inv[c];
}

// one row of `rounded`: the decoded codes of columns 2h, 2h + 1 in c[h], times the blocks' scales
LWM_DEVICE void mx_quant_store_rounded(bf16_t* at, const f32x2& c0, const f32x2& c1, const f32x2& c2, const f32x2& c3, const float (&s)[8]) {
    global_store_b128(at, u32x4{pack_bf16x2(c0[0] * s[0], c0[1] * s[1]), pack_bf16x2(c1[0] * s[2], c1[1] * s[3]),
                                pack_bf16x2(c2[0] * s[4], c2[1] * s[5]), pack_bf16x2(c3[0] * s[6], c3[1] * s[7])});
}

// Workgroup = 128 rows of K x 512 columns; wave w holds rows 32w..32w+31 of its lanes' columns in registers (W is read
// once).  Those 32 rows of a column are one MX block, so a lane has the whole block of each of its 8 columns: no LDS, no
// shuffles.  K % 32 == 0: a wave's rows exist or do not as a whole.  Every thread loads all its rows before it stores any,
// so `rounded` may be `w`.  F: kExpDrop / kMantTop of the scale rule, offset() of a slot, and step(): four rows encoded,
// their `rounded` rows written, their slot stored.
template <typename F>
LWM_DEVICE void mx_quantise_body(const MxQuantParams& p) {
    const int tid = thread_idx();
    const int wave = wave_uniform(tid >> 6), lane = tid & 63;
    const int nbn = (p.N + kW4QuantNT - 1) / kW4QuantNT;
    const int grp = block_idx_x() / nbn, nb = block_idx_x() % nbn;
    const int k0 = grp * kGemvKT + wave * kGemvRPW;
    const int n = nb * kW4QuantNT + lane * 8;
    if (k0 >= p.K || n >= p.N) return;
    const int64_t base = (int64_t)k0 * p.N + n;
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
    // amax = 1.m * 2^e: the smallest power of two s with amax / s <= the format's largest code (6 = 1.5 * 2^2; 7.5 =
    // 1.875 * 2^2) is 2^(e-2) when 1.m <= 1.5 (1.875) and 2^(e-1) otherwise (Kv4Format's / Kv6Format's rule).  Biased
    // exponent of s, clamped to 1 below; finite bf16 inputs stay under 254 by themselves.
    float s[8], inv[8];
    uint32_t se8[8];
    for (int j = 0; j < 8; ++j) {
        int se = 127;
        if (am[j] != 0) {
            se = (am[j] >> 7) - F::kExpDrop + ((am[j] & 0x7f) > F::kMantTop ? 1 : 0);
            se = se < 1 ? 1 : se;
        }
        se8[j] = (uint32_t)se;
        s[j] = __builtin_bit_cast(float, (uint32_t)se << 23);
        inv[j] = __builtin_bit_cast(float, (uint32_t)(254 - se) << 23);
    }
    global_store_b64(p.scale + (int64_t)(k0 / kGemvRPW) * p.N + n,
                     u32x2{se8[0] | se8[1] << 8 | se8[2] << 16 | se8[3] << 24, se8[4] | se8[5] << 8 | se8[6] << 16 | se8[7] << 24});
    uint8_t* qp = p.q + F::offset(k0, n, p.N);
#pragma unroll
    for (int i0 = 0; i0 < kGemvRPW; i0 += 4) F::step(wv, i0, inv, s, p.rounded + base, qp, p.N);
}

struct W4Quant {
    static constexpr int kExpDrop = Kv4Format::kExpDrop, kMantTop = Kv4Format::kMantTop;
    LWM_DEVICE static int64_t offset(int k, int n, int N) { return GemvW4Format::offset(k, n, N); }
    // rows i0 .. i0 + 3 of the wave's 32: `rounded` at the first of the 32, qp at their first slot
    LWM_DEVICE static void step(const u32x4 (&wv)[kGemvRPW], int i0, const float (&inv)[8], const float (&s)[8], bf16_t* rounded,
                                uint8_t* qp, int N) {
        u32x4 slot;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float x[8];
            mx_quant_scaled(wv[i0 + j], inv, x);
            const uint32_t codes = Kv4Format::encode(x);
            slot[j] = codes;
            mx_quant_store_rounded(rounded + (int64_t)(i0 + j) * N, cvt_e2m1x2<0>(codes), cvt_e2m1x2<1>(codes), cvt_e2m1x2<2>(codes),
                                   cvt_e2m1x2<3>(codes), s);
        }
        global_store_b128(qp + (int64_t)(i0 >> 2) * N * 2, slot);
    }
};

LWM_KERNEL(256) void w4_quantise_kernel(W4QuantParams p) { mx_quantise_body<W4Quant>(p); }

}  // namespace lwm
