// attn_decode_kv8.h -- an 8-bit (OCP e4m3fn) KV cache: the quantising cache write and the
// cached-decode attention kernel that streams it.  Requires wave_ops.h + attn_common.h +
// attn_decode.h (unpack_bf16x8, kDecThreads).
//
// Why: cached decode is HBM-bound and reads the whole cache once per token and layer
// (attn_decode.h); the bf16 kernel already streams near what the memory system gives, so the
// lever left is the number of bytes.  Per key row and head the cache holds 128 e4m3 bytes and one
// f32 scale instead of 256 bytes: 0.516 of the traffic and of the footprint.
//
// Format (per layer, four tensors):
//   cached_key, cached_value  uint8 (B, max_length, H, 128)  e4m3fn bit patterns, heads of a row contiguous
//   key_scale, value_scale    f32   (B, max_length, H)       one scale per row and head
// Quantising the 128 bf16 values x of one head of one row:
//   amax = max |x|;  s = the smallest power of two with amax / s <= 448, clamped to [2^-126, 2^127]
//   (amax == 0: s = 1);  q = e4m3(x / s), round to nearest even.
// x / s is exact in f32 (s is a power of two) and |x / s| <= 448, so nothing saturates and the
// result does not depend on the hardware's clamp mode.  q * s is exactly representable in bf16
// (4 significant bits times a power of two): a bf16 cache that holds q * s is the same numbers (for s >= 2^-117,
// i.e. amax >= 2^-108, every product is a normal number; below that the smallest ones are bf16 subnormals or vanish).
// Non-finite inputs (Inf, NaN) are NOT supported: their row's scale and bytes are unspecified.
#pragma once

namespace lwm {

// ---- the e4m3 codec
#ifdef LWM_EMU
// OCP e4m3fn: 1 sign, 4 exponent (bias 7), 3 mantissa bits; exponent 0 = subnormal (m * 2^-9); 0x7f / 0xff = NaN
LWM_DEVICE float e4m3_to_f32(uint32_t b) {
    const uint32_t e = (b >> 3) & 15, m = b & 7;
    float v;
    if (e == 15 && m == 7) v = __builtin_nanf("");
    else if (e == 0) v = ldexpf((float)m, -9);
    else v = ldexpf((float)(8 + m), (int)e - 10);
    return (b & 0x80) ? -v : v;
}
// f32 -> e4m3fn, round to nearest even, saturating at +-448 (callers stay in range)
LWM_DEVICE uint32_t f32_to_e4m3(float x) {
    uint32_t bits = __builtin_bit_cast(uint32_t, x);
    const uint32_t sign = (bits >> 24) & 0x80;
    bits &= 0x7fffffffu;
    if (bits > 0x7f800000u) return sign | 0x7f;                         // NaN
    const float ax = __builtin_bit_cast(float, bits);
    if (ax < 0.015625f) return sign | (uint32_t)nearbyintf(ax * 512.0f);  // below 2^-6: multiples of 2^-9 (8 = the least normal)
    bits += 0x7ffffu + ((bits >> 20) & 1);                              // to 3 mantissa bits, ties to even
    const int e = (int)(bits >> 23) - 127 + 7;
    const uint32_t m = (bits >> 20) & 7;
    if (e > 15 || (e == 15 && m == 7)) return sign | 0x7e;              // 448
    return sign | ((uint32_t)e << 3) | m;
}
LWM_DEVICE f32x2 cvt_e4m3x2_lo(uint32_t w) { return f32x2{e4m3_to_f32(w & 255), e4m3_to_f32((w >> 8) & 255)}; }
LWM_DEVICE f32x2 cvt_e4m3x2_hi(uint32_t w) { return f32x2{e4m3_to_f32((w >> 16) & 255), e4m3_to_f32(w >> 24)}; }
LWM_DEVICE uint32_t pack_e4m3x4(float a, float b, float c, float d) {
    return f32_to_e4m3(a) | (f32_to_e4m3(b) << 8) | (f32_to_e4m3(c) << 16) | (f32_to_e4m3(d) << 24);
}
#else
// v_cvt_pk_f32_fp8: two e4m3 bytes of one 16-bit half of a dword -> two f32 in a register pair (OCP on gfx950)
LWM_DEVICE f32x2 cvt_e4m3x2_lo(uint32_t w) {
    auto r = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false);
    return f32x2{r[0], r[1]};
}
LWM_DEVICE f32x2 cvt_e4m3x2_hi(uint32_t w) {
    auto r = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
    return f32x2{r[0], r[1]};
}
// v_cvt_pk_fp8_f32 twice: four f32 -> four e4m3 bytes, round to nearest even
LWM_DEVICE uint32_t pack_e4m3x4(float a, float b, float c, float d) {
    int w = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, w, true);
    return (uint32_t)w;
}
#endif

// The format for attn_decode_kvq.h.  Write: the 16 lanes of a head share one scale; amax = 1.m * 2^e: the smallest power of
// two s with amax / s <= 448 = 1.75 * 2^8 is 2^(e-8) when 1.m <= 1.75 (seven mantissa bits: m <= 0x60) and 2^(e-7)
// otherwise (e <= 127 gives s <= 2^120: under the upper clamp).  Decode: a head row is 128 B, so 8 lanes x 16 B own it,
// lane i holds d = 16i..16i+15, and the workgroup has 64 head slots (two keys per pass at H = 32).  The two scales of a
// (key, head) enter as scalars after the lane reduction: score = (q . k_q) * key_scale.
struct Kv8Format {
    typedef float scale_t;
    static constexpr int kHeadBytes = kHeadDim;
    static constexpr int kAmaxLanes = 16, kExpDrop = 8, kMantTop = 0x60;
    LWM_FORMAT_FN float scale_of(int se) { return __builtin_bit_cast(float, (uint32_t)se << 23); }
    LWM_FORMAT_FN u32x2 encode(const float (&y)[8]) {
        return u32x2{pack_e4m3x4(y[0], y[1], y[2], y[3]), pack_e4m3x4(y[4], y[5], y[6], y[7])};
    }
    LWM_FORMAT_FN void store(uint8_t* head, int li, u32x2 w, bool ok) { store_lane_codes<Kv8Format>(head, li, w, ok); }
    static constexpr int kLanes = 8, kLaneDwords = 4;
    typedef u32x4 codes_t;
    LWM_FORMAT_FN u32x4 load_lane(const uint8_t* p) { return global_load_b128(p); }
    LWM_FORMAT_FN int scale_index(int h, int) { return h; }
    LWM_FORMAT_FN uint32_t load_scale(const float* p) { return __builtin_bit_cast(uint32_t, global_load_f32(p)); }
    LWM_FORMAT_FN float scale_f32(uint32_t bits) { return __builtin_bit_cast(float, bits); }
    LWM_FORMAT_FN void cvt_lane(u32x4 w, f32x2 (&f)[8]) {
        for (int i = 0; i < 4; ++i) {
            f[2 * i] = cvt_e4m3x2_lo(w[i]);
            f[2 * i + 1] = cvt_e4m3x2_hi(w[i]);
        }
    }
    LWM_FORMAT_FN float scale_lane(float a, float) { return a; }
    LWM_FORMAT_FN float scale_head(float a, float ks) { return a * ks; }
};

// (types of their own, so that the kernels' symbols do not depend on how the parameters are spelled)
struct Kv8WriteParams : KvqWriteParams<Kv8Format> {};
struct Kv8DecodeParams : KvqDecodeParams<Kv8Format> {};

LWM_KERNEL(256) void kv8_quant_write_kernel(Kv8WriteParams p) { kv_quant_rows<Kv8Format>(p, p.dst_row0); }
// The destination row from DEVICE memory, as kv_cache_write_at_kernel: nothing about a decode step depends on a host
// value, so the step can be captured in a hipGraph and replayed while the index advances on the device.
LWM_KERNEL(256) void kv8_quant_write_at_kernel(Kv8WriteParams p) { kv_quant_rows<Kv8Format>(p, (int64_t)p.row0_dev[0] + p.dst_row0); }
LWM_KERNEL(kDecThreads) void attn_decode_kv8_kernel(Kv8DecodeParams p) { attn_decode_kvq<Kv8Format>(p); }

}  // namespace lwm
