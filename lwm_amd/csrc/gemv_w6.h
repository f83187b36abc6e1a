// gemv_w6.h -- 6-bit (OCP MXFP6: e2m3 codes, one e8m0 scale per 32 rows of K) decode weights: the quantiser and the weight
// format of the GEMV that streams them.  Requires wave_ops.h + gemv.h (GemvParams, gemv_body, gemv_by_rows) + attn_decode.h
// (unpack_bf16x8, f32x2, fma2, global_load_b64) + attn_decode_kv4.h (e8m0_to_f32) + attn_decode_kv6.h (u32x6, f32_to_e2m3,
// cvt_e2m3x32_f32, Kv6Format: encode, kExpDrop, kMantTop) + gemv_w4.h (GemvW4Params, GemvW4Format: the accumulators and the
// per-wave scale are the 4-bit format's).
//
// Why: gemv_w8.h streams 0.516 of the bf16 bytes and leaves a model nearly where it was; gemv_w4.h streams 0.266 and moves
// its logits four times as far.  e2m3 keeps e4m3's three mantissa bits: per (K, N) kernel this pack holds 3 K N / 4 bytes
// of codes and one scale byte per 32 rows of K and column, 6.25 bits per weight, 0.391 of the bf16 bytes and 0.757 of the
// 8-bit pack's.
//
// Format (include/lwm_hip.h, "6-bit decode weights"):
//   q      uint8 (K/4, N/8, 24)   e2m3 codes.  Slot [k4][n8] is 24 bytes = rows 4 k4 .. 4 k4 + 3 of columns 8 n8 .. 8 n8 + 7:
//                                 code 8 j + c is row 4 k4 + j, column 8 n8 + c, and code i is bits [6i, 6i + 6) of the
//                                 slot read as one little-endian 192-bit integer (the block of the 6-bit KV cache, and
//                                 the element order of v_cvt_scalef32_pk32_f32_fp6)
//   scale  uint8 (K/32, N)        one e8m0 byte b per MX block = 32 consecutive rows of K of one column: the scale 2^(b-127)
//   amax over the block; s = the smallest power of two with amax / s <= 7.5, its exponent byte clamped to [1, 254]
//   (amax == 0: byte 127); q = e2m3(w / s), round to nearest, ties to the even code -- attn_decode_kv6.h's rule.
//
// The slot is what one lane of gemv_body loads at a time (lane l owns columns 8l..8l+7): four rows in 24 bytes, a wave
// load is 1536 bytes contiguous, and the wave's 32 rows are the 8 loads the bf16 kernel keeps in flight.  A slot starts at a
// multiple of 8, not of 16: it is loaded as three 8-byte words, as the 6-bit cache's blocks are (a 16-byte and an 8-byte
// load ordered by the slot's parity was not measured: profiles/r26_w6_decode.md).
//
// Why the bits agree with the bf16 kernel on the rounded weights e2m3(q) * s: gemv_w4.h's argument.  The MX block is the 32
// rows one wave walks, each column of a wave's sum sees ONE scale, both kernels are gemv_body, e2m3(q) * s has 4
// significant bits (exact in bf16), and with a power-of-two s (no overflow, no underflow)
// fmaf(x, q * s, a * s) == s * fmaf(x, q, a).
#pragma once

namespace lwm {

typedef GemvW4Params GemvW6Params;     // q: [K/4, N_i/8, 24] e2m3 codes; scale: [K/32, N_i] e8m0 bytes

// The e2m3 weight format of gemv_body (gemv.h): GemvW4Format with a 24-byte slot -- one conversion of its 32 codes with
// scale 1 per load, then the packed FMAs; the accumulators (pairs of columns) and the multiply by the block's scale per
// finished wave sum are inherited.
struct GemvW6Format : GemvW4Format {
    using Load = u32x6;
    // bytes: slot [k / 4][n / 8] of 24 (k % 4 == 0, n % 8 == 0)
    LWM_DEVICE static int64_t offset(int k, int n, int N) { return ((int64_t)k * N >> 2) * 3 + 3 * n; }
    LWM_DEVICE static Load load(const Elem* at) {
        const u32x2 a = global_load_b64(at), b = global_load_b64(at + 8), c = global_load_b64(at + 16);
        return u32x6{a[0], a[1], b[0], b[1], c[0], c[1]};
    }
    template <int R>
    LWM_DEVICE static void fma(Acc (&a)[R], const Load& w, const float (&xv)[R], int i) {
        f32x2 c[16];                               // c[4 j + h]: row j, columns 2h, 2h + 1
        cvt_e2m3x32_f32(w, c);
#pragma unroll
        for (int j = 0; j < kRows; ++j)
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const float xs = lane_value(xv[r], i + j);
                const f32x2 x2 = {xs, xs};
#pragma unroll
                for (int h = 0; h < 4; ++h) a[r][h] = fma2(x2, c[4 * j + h], a[r][h]);
            }
    }
};

// dynamic LDS: 3 * R * kGemvNT * 4 bytes (the host sizes it by the row count)
LWM_KERNEL(kGemvThreads) void gemv_w6_kernel(GemvW6Params p) { gemv_by_rows<GemvW6Format>(p); }

// ------------------------------------------------------------------ quantiser
typedef MxQuantParams W6QuantParams;   // q: [K/4, N/8, 24] e2m3 codes

// mx_quantise_body (gemv_w4.h) with the e2m3 encoder and the 24-byte slot
struct W6Quant {
    static constexpr int kExpDrop = Kv6Format::kExpDrop, kMantTop = Kv6Format::kMantTop;
    LWM_DEVICE static int64_t offset(int k, int n, int N) { return GemvW6Format::offset(k, n, N); }
    LWM_DEVICE static void step(const u32x4 (&wv)[kGemvRPW], int i0, const float (&inv)[8], const float (&s)[8], bf16_t* rounded,
                                uint8_t* qp, int N) {
        u32x2 h[4];                                // row j of the slot: 8 codes = 48 bits (32 + 16)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float x[8];
            mx_quant_scaled(wv[i0 + j], inv, x);
            h[j] = Kv6Format::encode(x);
        }
        // the slot's 192 bits: row j at bits [48 j, 48 j + 48)
        const u32x6 slot = {h[0][0], h[0][1] | (h[1][0] << 16), (h[1][0] >> 16) | (h[1][1] << 16),
                            h[2][0], h[2][1] | (h[3][0] << 16), (h[3][0] >> 16) | (h[3][1] << 16)};
        f32x2 c[16];
        cvt_e2m3x32_f32(slot, c);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            mx_quant_store_rounded(rounded + (int64_t)(i0 + j) * N, c[4 * j], c[4 * j + 1], c[4 * j + 2], c[4 * j + 3], s);
        uint8_t* sp = qp + (int64_t)(i0 >> 2) * N * 3;
        global_store_b64(sp, u32x2{slot[0], slot[1]});
        global_store_b64(sp + 8, u32x2{slot[2], slot[3]});
        global_store_b64(sp + 16, u32x2{slot[4], slot[5]});
    }
};

LWM_KERNEL(256) void w6_quantise_kernel(W6QuantParams p) { mx_quantise_body<W6Quant>(p); }

}  // namespace lwm
