// attn_decode_kv6.h -- a 6-bit (OCP MXFP6: e2m3 codes, one e8m0 scale per 32 elements) KV cache: the quantising cache
// write and the cached-decode attention kernel that streams it.  Requires wave_ops.h + attn_common.h + attn_decode.h
// (f32x2, global_load_u8, global_load_b64) + attn_decode_kvq.h (the write and the kernel, over Kv6Format below) +
// attn_decode_kv4.h (e8m0_to_f32 and the scale half of Kv4Format: the scale tensors of the two caches are the same).
//
// Why: the 8-bit cache does not hold a million tokens on one GPU and the 4-bit cache pays for it in precision.  Per key
// row and head this cache holds 96 bytes of codes and 4 scale bytes: 100 against 132 (attn_decode_kv8.h) and 68
// (attn_decode_kv4.h), 0.39 of the bf16 bytes, held and read per token.
//
// Format (per layer, four tensors):
//   cached_key, cached_value           uint8 (B, max_length, H, 96)  four blocks of 24 bytes; element j of a block is bits
//                                                                    [6j, 6j + 6) of the block's bytes read as one
//                                                                    little-endian 192-bit integer; heads of a row contiguous
//   key_scale_e8m0, value_scale_e8m0   uint8 (B, max_length, H, 4)   one e8m0 byte b per block of 32 consecutive elements
//                                                                    of a head: the scale 2^(b - 127)
// e2m3: sign in bit 5, exponent (bias 1) in bits 4-3, mantissa in bits 2-0.  Magnitude code c = 0..31: c / 8 below 8,
// (1 + (c & 7) / 8) * 2^((c >> 3) - 1) from 8 on; the largest is 7.5; magnitudes are monotone in c.
// Quantising one block of 32 bf16 values x:
//   amax = max |x|;  s = the smallest power of two with amax / s <= 7.5, its biased exponent clamped to [1, 254]
//   (amax == 0: s = 1, byte 127);  q = e2m3(x / s), round to nearest, ties to the even code.
// x / s is exact in f32 and |x / s| <= 7.5, so nothing saturates.  -0 keeps its sign.  q * s has at most 4 significant
// bits times a power of two: it is exactly representable in bf16, a normal number whenever s >= 2^-123.  A bf16 cache
// that holds q * s is the same numbers.  Non-finite inputs are NOT supported (nor is a block whose amax reaches 1.9375 * 2^127,
// about 3.30e38: its largest element rounds up to 4 * 2^126 = 2^128, past the top of bf16 and f32).
// (This is the rule of attn_decode_kv4.h with 7.5 in place of 6.)
#pragma once

namespace lwm {

typedef uint32_t u32x6 __attribute__((ext_vector_type(6)));

// ---- the e2m3 codec
#ifdef LWM_EMU
LWM_DEVICE float e2m3_to_f32(uint32_t c) {
    const uint32_t m = c & 31;
    // below 8: m / 8; from 8 on the f32 with exponent (m >> 3) - 1 and the three mantissa bits on top
    const float v = m < 8 ? (float)m * 0.125f : __builtin_bit_cast(float, (m + (126u << 3)) << 20);
    return (c & 32) ? -v : v;
}
// code j of the lane's 192 bits
LWM_DEVICE uint32_t e2m3_code_at(u32x6 w, int j) {
    const int bit = 6 * j, d = bit >> 5, sh = bit & 31;
    uint32_t c = w[d] >> sh;
    if (sh > 26) c |= w[d + 1] << (32 - sh);
    return c & 63;
}
LWM_DEVICE void cvt_e2m3x32_f32(u32x6 w, f32x2 (&f)[16]) {
    for (int j = 0; j < 16; ++j) f[j] = f32x2{e2m3_to_f32(e2m3_code_at(w, 2 * j)), e2m3_to_f32(e2m3_code_at(w, 2 * j + 1))};
}
// 32 codes times one power-of-two scale -> 32 bf16 (64 bytes), exactly wherever the products are normal numbers
LWM_DEVICE void cvt_e2m3x32_bf16(u32x6 w, float s, u32x4 (&o)[4]) {
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j)
            o[i][j] = pack_bf16x2(e2m3_to_f32(e2m3_code_at(w, 8 * i + 2 * j)) * s, e2m3_to_f32(e2m3_code_at(w, 8 * i + 2 * j + 1)) * s);
}
#else
// v_cvt_scalef32_pk32_f32_fp6 with a scale of 1: the block scale enters once per lane and key, not per element
LWM_DEVICE void cvt_e2m3x32_f32(u32x6 w, f32x2 (&f)[16]) {
    const auto r = __builtin_amdgcn_cvt_scalef32_pk32_f32_fp6(w, 1.0f);
    for (int j = 0; j < 16; ++j) f[j] = f32x2{r[2 * j], r[2 * j + 1]};
}
// v_cvt_scalef32_pk32_bf16_fp6: the block of a staged row in one instruction
LWM_DEVICE void cvt_e2m3x32_bf16(u32x6 w, float s, u32x4 (&o)[4]) {
    typedef uint32_t u32x16 __attribute__((ext_vector_type(16)));
    const u32x16 r = __builtin_bit_cast(u32x16, __builtin_amdgcn_cvt_scalef32_pk32_bf16_fp6(w, s));
    for (int i = 0; i < 4; ++i) o[i] = u32x4{r[4 * i], r[4 * i + 1], r[4 * i + 2], r[4 * i + 3]};
}
#endif
// f32 y, |y| <= 7.5 -> e2m3 code, round to nearest, ties to the even code (the mantissa's last bit is the code's last
// bit, and a carry out of the mantissa lands in the exponent: IEEE rounding on the code).  Integer arithmetic on the bits
// of y; no conversion instruction, no rounding mode.  From 1 on the code is the f32's exponent and top three mantissa
// bits; below 1 it is y * 8 rounded to an integer (8 = the code of 1).
LWM_DEVICE uint32_t f32_to_e2m3(float y) {
    const uint32_t bits = __builtin_bit_cast(uint32_t, y);
    const uint32_t sign = (bits >> 26) & 32u, a = bits & 0x7fffffffu;
    if (a >= 0x3f800000u) return sign | (((a + 0x7ffffu + ((a >> 20) & 1u)) >> 20) - (126u << 3));
    const uint32_t sh = 147u - (a >> 23);              // y * 8 = 1.m * 2^(e - 124) = (2^23 + m) >> sh
    if (sh > 25u) return sign;                         // below 2^-2 / 8 ... (f32 subnormals included): nearer to 0 than to 1 / 8
    const uint32_t man = (a & 0x7fffffu) | 0x800000u, q = man >> sh, rem = man & ((1u << sh) - 1u), half = 1u << (sh - 1u);
    return sign | (q + (uint32_t)(rem > half || (rem == half && (q & 1u))));
}

// The format for attn_decode_kvq.h.  The scale tensors are the 4-bit cache's (one e8m0 byte per block of 32, the block
// scale entering per lane before the lane reduction), so that half of the description is inherited; the codes differ.
// Write: 4 consecutive lanes of the 16 of a head hold one block of 32 and share its scale byte; amax = 1.m * 2^e: the
// smallest power of two s with amax / s <= 7.5 = 1.875 * 2^2 is 2^(e-2) when 1.m <= 1.875 (seven mantissa bits:
// m <= 0x70) and 2^(e-1) otherwise.  A lane's 8 codes are 48 bits, which no aligned store takes: the four lanes of a
// block hand their halves round and lanes 0..2 store the block's 24 bytes as three 8-byte words.  Decode: a head row is
// 96 B, so 4 lanes x 24 B own it: lane i holds d = 32i..32i+31, one MX block and one scale byte, loaded as three 8-byte
// words (a block starts at a multiple of 8, not of 16), and the workgroup has 128 head slots as over the 4-bit cache.
struct Kv6Format : Kv4Format {
    static constexpr int kHeadBytes = kHeadDim * 3 / 4;
    static constexpr int kMantTop = 0x70;
    LWM_FORMAT_FN u32x2 encode(const float (&y)[8]) {
        uint32_t c[8];
        for (int j = 0; j < 8; ++j) c[j] = f32_to_e2m3(y[j]);
        return u32x2{c[0] | (c[1] << 6) | (c[2] << 12) | (c[3] << 18) | (c[4] << 24) | (c[5] << 30),
                     (c[5] >> 2) | (c[6] << 4) | (c[7] << 10)};
    }
    // w = the lane's 48 bits (32 + 16).  The block's 192 bits are the chunks of its lanes t = 0..3 in order; word t of
    // the three takes the rest of chunk t and the start of chunk t + 1, which is lane t ^ 1 for even t and t ^ 3 for t = 1.
    LWM_FORMAT_FN void store(uint8_t* head, int li, u32x2 w, bool ok) {
        const int t = li & 3;
        const uint32_t lo1 = (uint32_t)shfl_xor_i((int)w[0], 1), hi1 = (uint32_t)shfl_xor_i((int)w[1], 1);
        const uint32_t lo3 = (uint32_t)shfl_xor_i((int)w[0], 3), hi3 = (uint32_t)shfl_xor_i((int)w[1], 3);
        const uint32_t nlo = t == 1 ? lo3 : lo1, nhi = t == 1 ? hi3 : hi1;
        u32x2 o;
        if (t == 0) o = u32x2{w[0], w[1] | (nlo << 16)};
        else if (t == 1) o = u32x2{(w[0] >> 16) | (w[1] << 16), nlo};
        else o = u32x2{w[1] | (nlo << 16), (nlo >> 16) | (nhi << 16)};
        if (ok && t < 3) global_store_b64(head + (li >> 2) * 24 + t * 8, o);
    }
    static constexpr int kLaneDwords = 6;
    typedef u32x6 codes_t;
    LWM_FORMAT_FN u32x6 load_lane(const uint8_t* p) {
        const u32x2 a = global_load_b64(p), b = global_load_b64(p + 8), c = global_load_b64(p + 16);
        return u32x6{a[0], a[1], b[0], b[1], c[0], c[1]};
    }
    LWM_FORMAT_FN void cvt_lane(u32x6 w, f32x2 (&f)[16]) { cvt_e2m3x32_f32(w, f); }
};

struct Kv6WriteParams : KvqWriteParams<Kv6Format> {};
struct Kv6DecodeParams : KvqDecodeParams<Kv6Format> {};

LWM_KERNEL(256) void kv6_quant_write_kernel(Kv6WriteParams p) { kv_quant_rows<Kv6Format>(p, p.dst_row0); }
// The destination row from DEVICE memory, as kv8_quant_write_at_kernel: a decode step that a hipGraph replays.
LWM_KERNEL(256) void kv6_quant_write_at_kernel(Kv6WriteParams p) { kv_quant_rows<Kv6Format>(p, (int64_t)p.row0_dev[0] + p.dst_row0); }
LWM_KERNEL(kDecThreads) void attn_decode_kv6_kernel(Kv6DecodeParams p) { attn_decode_kvq<Kv6Format>(p); }

}  // namespace lwm
