// attn_decode_kv4.h -- a 4-bit (OCP MXFP4: e2m1 codes, one e8m0 scale per 32 elements) KV cache: the quantising cache
// write and the cached-decode attention kernel that streams it.  Requires wave_ops.h + attn_common.h + attn_decode.h
// (f32x2, global_load_u8, global_store_b32) + attn_decode_kvq.h (the write and the kernel, over Kv4Format below).
//
// Why: at a million tokens the cache is the memory.  Per key row and head this cache holds 64 bytes of nibbles and
// 4 scale bytes instead of 256 (bf16) or 132 (attn_decode_kv8.h): 0.27 of the bf16 bytes, held and read per token.
//
// Format (per layer, four tensors):
//   cached_key, cached_value           uint8 (B, max_length, H, 64)  two e2m1 codes per byte: element 2i in the low nibble,
//                                                                    element 2i+1 in the high nibble; heads of a row contiguous
//   key_scale_e8m0, value_scale_e8m0   uint8 (B, max_length, H, 4)   one e8m0 byte b per block of 32 consecutive elements
//                                                                    of a head: the scale 2^(b - 127)
// e2m1: sign in bit 3, magnitudes 0, 0.5, 1, 1.5, 2, 3, 4, 6 for the codes 0..7.
// Quantising one block of 32 bf16 values x:
//   amax = max |x|;  s = the smallest power of two with amax / s <= 6, its biased exponent clamped to [1, 254]
//   (amax == 0: s = 1, byte 127);  q = e2m1(x / s), round to nearest, ties to the even code.
// x / s is exact in f32 and |x / s| <= 6, so nothing saturates.  -0 keeps its sign.  q * s has at most 2 significant
// bits times a power of two: it is exactly representable in bf16, a normal number whenever s >= 2^-125.  A bf16 cache
// that holds q * s is the same numbers.  Non-finite inputs are NOT supported (nor is a block whose amax exceeds 3.5 * 2^126,
// about 2.98e38: its largest element rounds up to 4 * 2^126 = 2^128, past the top of bf16 and f32).
// (This is the rule of attn_decode_kv8.h with 6 in place of 448 -- not the OCP "floor(log2 amax) - 2", which saturates.)
#pragma once

namespace lwm {

// ---- the e2m1 / e8m0 codec
#ifdef LWM_EMU
LWM_DEVICE float e2m1_to_f32(uint32_t c) {
    const float mag[8] = {0.0f, 0.5f, 1.0f, 1.5f, 2.0f, 3.0f, 4.0f, 6.0f};
    return (c & 8) ? -mag[c & 7] : mag[c & 7];
}
// the two codes of byte `Byte` of a dword -> (low nibble, high nibble) as f32
template <int Byte>
LWM_DEVICE f32x2 cvt_e2m1x2(uint32_t w) {
    const uint32_t b = (w >> (8 * Byte)) & 255;
    return f32x2{e2m1_to_f32(b & 15), e2m1_to_f32(b >> 4)};
}
#else
// v_cvt_scalef32_pk_f32_fp4 with a scale of 1: the block scale enters once per 32 elements, not per pair
template <int Byte>
LWM_DEVICE f32x2 cvt_e2m1x2(uint32_t w) {
    auto r = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, 1.0f, Byte);
    return f32x2{r[0], r[1]};
}
#endif
// e8m0 byte -> f32: 2^(b - 127); byte 0 is 2^-127, an f32 subnormal (the write never emits 0 or 255)
LWM_DEVICE float e8m0_to_f32(uint32_t b) { return __builtin_bit_cast(float, b ? b << 23 : 0x00400000u); }
// f32 y, |y| <= 6 -> e2m1 code, round to nearest, ties to the even code: the midpoints 0.25, 1.25, 2.5, 5 belong to the
// code below them (even), 0.75, 1.75, 3.5 to the code above.  Integer arithmetic on comparisons; no conversion
// instruction, no rounding mode.
LWM_DEVICE uint32_t f32_to_e2m1(float y) {
    const uint32_t bits = __builtin_bit_cast(uint32_t, y);
    const float a = __builtin_bit_cast(float, bits & 0x7fffffffu);
    const uint32_t c = (uint32_t)(a > 0.25f) + (uint32_t)(a >= 0.75f) + (uint32_t)(a > 1.25f) + (uint32_t)(a >= 1.75f) +
                       (uint32_t)(a > 2.5f) + (uint32_t)(a >= 3.5f) + (uint32_t)(a > 5.0f);
    return ((bits >> 28) & 8u) | c;
}

// The format for attn_decode_kvq.h.  Write: 4 consecutive lanes of the 16 of a head hold one block of 32 and share its
// scale byte; amax = 1.m * 2^e: the smallest power of two s with amax / s <= 6 = 1.5 * 2^2 is 2^(e-2) when 1.m <= 1.5
// (seven mantissa bits: m <= 0x40) and 2^(e-1) otherwise (e <= 254 gives at most 253: under the upper clamp).  Decode: a
// head row is 64 B, so 4 lanes x 16 B own it: lane i holds d = 32i..32i+31, which is exactly one MX block and one scale
// byte, and the workgroup has 128 head slots (four keys per pass at H = 32).  The block scale enters per lane, before
// the lane reduction: score = sum over the blocks of scale_b * (q_b . k_b), block b in lane b.
struct Kv4Format {
    typedef uint8_t scale_t;
    static constexpr int kHeadBytes = kHeadDim / 2;
    static constexpr int kAmaxLanes = 4, kExpDrop = 2, kMantTop = 0x40;
    LWM_FORMAT_FN uint8_t scale_of(int se) { return (uint8_t)se; }
    LWM_FORMAT_FN uint32_t encode(const float (&y)[8]) {
        uint32_t w = 0;
        for (int j = 0; j < 8; ++j) w |= f32_to_e2m1(y[j]) << (4 * j);
        return w;
    }
    LWM_FORMAT_FN void store(uint8_t* head, int li, uint32_t w, bool ok) { store_lane_codes<Kv4Format>(head, li, w, ok); }
    static constexpr int kLanes = 4, kLaneDwords = 4;
    typedef u32x4 codes_t;
    LWM_FORMAT_FN u32x4 load_lane(const uint8_t* p) { return global_load_b128(p); }
    LWM_FORMAT_FN int scale_index(int h, int li) { return h * 4 + li; }
    LWM_FORMAT_FN uint32_t load_scale(const uint8_t* p) { return global_load_u8(p); }
    LWM_FORMAT_FN float scale_f32(uint32_t bits) { return e8m0_to_f32(bits); }
    LWM_FORMAT_FN void cvt_lane(u32x4 w, f32x2 (&f)[16]) {
        for (int i = 0; i < 4; ++i) {
            f[4 * i] = cvt_e2m1x2<0>(w[i]);
            f[4 * i + 1] = cvt_e2m1x2<1>(w[i]);
            f[4 * i + 2] = cvt_e2m1x2<2>(w[i]);
            f[4 * i + 3] = cvt_e2m1x2<3>(w[i]);
        }
    }
    LWM_FORMAT_FN float scale_lane(float a, float ks) { return a * ks; }
    LWM_FORMAT_FN float scale_head(float a, float) { return a; }
};

struct Kv4WriteParams : KvqWriteParams<Kv4Format> {};
struct Kv4DecodeParams : KvqDecodeParams<Kv4Format> {};

LWM_KERNEL(256) void kv4_quant_write_kernel(Kv4WriteParams p) { kv_quant_rows<Kv4Format>(p, p.dst_row0); }
// The destination row from DEVICE memory, as kv8_quant_write_at_kernel: a decode step that a hipGraph replays.
LWM_KERNEL(256) void kv4_quant_write_at_kernel(Kv4WriteParams p) { kv_quant_rows<Kv4Format>(p, (int64_t)p.row0_dev[0] + p.dst_row0); }
LWM_KERNEL(kDecThreads) void attn_decode_kv4_kernel(Kv4DecodeParams p) { attn_decode_kvq<Kv4Format>(p); }

}  // namespace lwm
