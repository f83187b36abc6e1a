// attn_decode_kv4.h -- a 4-bit (OCP MXFP4: e2m1 codes, one e8m0 scale per 32 elements) KV cache: the quantising cache
// write and the cached-decode attention kernel that streams it.  Requires wave_ops.h + attn_common.h + attn_decode.h
// (unpack_bf16x8, kDecThreads, kDecUnroll) + attn_decode_kv8.h (f32x2, fma2, issue_fence, global_load_u8).
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

// ---- primitives of this header
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
LWM_DEVICE void global_store_b32(void* p, uint32_t v) { memcpy(p, &v, 4); }
#else
// v_cvt_scalef32_pk_f32_fp4 with a scale of 1: the block scale enters once per 32 elements, not per pair
template <int Byte>
LWM_DEVICE f32x2 cvt_e2m1x2(uint32_t w) {
    auto r = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, 1.0f, Byte);
    return f32x2{r[0], r[1]};
}
LWM_DEVICE void global_store_b32(void* p, uint32_t v) { *(uint32_t*)p = v; }
#endif
LWM_DEVICE void global_store_u8(uint8_t* p, uint8_t v) { *p = v; }
// the eight codes of a dword, element order
LWM_DEVICE void cvt_e2m1x8(uint32_t w, f32x2 (&f)[4]) {
    f[0] = cvt_e2m1x2<0>(w);
    f[1] = cvt_e2m1x2<1>(w);
    f[2] = cvt_e2m1x2<2>(w);
    f[3] = cvt_e2m1x2<3>(w);
}
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

// ------------------------------------------------------------------ quantising cache write
struct Kv4WriteParams {
    uint8_t* cache;            // (B, cache_rows, H, 64) nibble bytes
    uint8_t* scale;            // (B, cache_rows, H, 4) e8m0 bytes
    const bf16_t* src;         // (B, *, H, 128) bf16
    int64_t cache_sb, scale_sb, src_sb;     // batch strides: bytes, bytes, bf16 elements
    const int32_t* row0_dev;   // the _at form: destination row = *row0_dev + dst_row0 + i
    int64_t dst_row0;          // destination row of source row src_row0 (the _at form: the offset added to *row0_dev)
    int64_t cache_rows;        // rows outside [0, cache_rows) are skipped
    int64_t src_row0, nrows;
    int32_t B, H;
};

// 16 lanes own one head of one row: lane i holds elements 8i..8i+7 (one 16-byte load), so 4 consecutive lanes hold one
// block of 32.  The integer amax of the bf16 bit patterns is reduced over them with two xor-shuffles; each lane packs its
// 8 codes into one dword and the first lane of a block stores the scale byte.  Every lane of a wave runs every shuffle
// (the trip count is uniform over the workgroup; what a lane may not do is decided at the loads and stores).
LWM_DEVICE void kv4_quant_rows(const Kv4WriteParams& p, int64_t dst_row0) {
    const int64_t total = (int64_t)p.B * p.nrows * p.H * 16;
    for (int64_t base = (int64_t)block_idx_x() * 256; base < total; base += (int64_t)grid_dim_x() * 256) {
        const int64_t i = base + thread_idx();
        const bool in = i < total;                         // (total is a multiple of 16: a group is in or out as a whole)
        const int64_t hh = (in ? i : total - 1) >> 4;
        const int li = (int)(i & 15);
        const int h = (int)(hh % p.H);
        const int64_t r = (hh / p.H) % p.nrows;
        const int64_t b = hh / ((int64_t)p.H * p.nrows);
        const int64_t dr = dst_row0 + r;
        const u32x4 raw = global_load_b128(p.src + b * p.src_sb + ((p.src_row0 + r) * p.H + h) * kHeadDim + li * 8);
        // |x| as integers: bf16 magnitudes order like their bit patterns
        int am = 0;
        for (int c = 0; c < 4; ++c) {
            const int lo = (int)(raw[c] & 0x7fffu), hi = (int)((raw[c] >> 16) & 0x7fffu);
            am = lo > am ? lo : am;
            am = hi > am ? hi : am;
        }
        for (int msk = 1; msk < 4; msk <<= 1) {
            const int o = shfl_xor_i(am, msk);
            am = o > am ? o : am;
        }
        // amax = 1.m * 2^e: the smallest power of two s with amax / s <= 6 = 1.5 * 2^2 is 2^(e-2) when 1.m <= 1.5 (seven
        // mantissa bits: m <= 0x40) and 2^(e-1) otherwise.  Biased exponent of s, clamped to 1 below; finite bf16 inputs
        // stay under the upper clamp by themselves (e <= 254 gives at most 253).
        int se = 127;
        if (am != 0) {
            se = (am >> 7) - 2 + ((am & 0x7f) > 0x40 ? 1 : 0);
            se = se < 1 ? 1 : se;
        }
        const float inv = __builtin_bit_cast(float, (uint32_t)(254 - se) << 23);
        float x[8];
        unpack_bf16x8(raw, x);
        uint32_t w = 0;
        for (int j = 0; j < 8; ++j) w |= f32_to_e2m1(x[j] * inv) << (4 * j);
        if (in && dr >= 0 && dr < p.cache_rows) {
            global_store_b32(p.cache + b * p.cache_sb + (dr * p.H + h) * (kHeadDim / 2) + li * 4, w);
            if ((li & 3) == 0) global_store_u8(p.scale + b * p.scale_sb + (dr * p.H + h) * 4 + (li >> 2), (uint8_t)se);
        }
    }
}

LWM_KERNEL(256) void kv4_quant_write_kernel(Kv4WriteParams p) { kv4_quant_rows(p, p.dst_row0); }
// The destination row from DEVICE memory, as kv8_quant_write_at_kernel: a decode step that a hipGraph replays.
LWM_KERNEL(256) void kv4_quant_write_at_kernel(Kv4WriteParams p) { kv4_quant_rows(p, (int64_t)p.row0_dev[0] + p.dst_row0); }

// ------------------------------------------------------------------ decode attention over the 4-bit cache
struct Kv4DecodeParams {
    const bf16_t* q;           // (B, 1, H, 128) bf16
    const uint8_t* k;          // nibble bytes
    const uint8_t* v;
    const uint8_t* k_scale;    // e8m0 bytes
    const uint8_t* v_scale;
    int64_t q_sb, q_sh;
    int64_t k_sb, k_ss, k_sh;  // bytes
    int64_t v_sb, v_ss, v_sh;
    int64_t ks_sb, ks_ss;      // scales: bytes; the 4 bytes of a head and the heads of a row contiguous
    int64_t vs_sb, vs_ss;
    const uint8_t* dense_mask; // (B, Sk) u8 or null
    int64_t msk_sb;
    int32_t B, Sk, H, k_splits;
    float scale;
    float* out_acc;            // [k_splits, B, 1, H, 128] f32 normalised partials
    float* lse_acc;            // [k_splits, B, H, 1]
};

constexpr int kDec4Slots = kDecThreads / 4;                           // 128 head slots of 4 lanes
constexpr int kDec4LdsBytes = (kDec4Slots / 2) * (kHeadDim + 2) * 4;  // the merge of the key lanes: half the slots leave o[128], m, l

// The contract of attn_decode_kv8_kernel -- one workgroup per (batch row, piece of the VISIBLE key range), holes handled
// per key, per-piece phase rotation, normalised partials merged by attn_combine_kernel, nothing visible = (0, -inf) --
// over rows of a quarter of the bf16 size.  A head row is 64 B, so 4 lanes x 16 B own it: lane i holds d = 32i..32i+31 of
// q, of the running output and of each K/V row, which is exactly one MX block and one scale byte.  The workgroup has 128
// head slots.  Where H < 128 the slots beyond the first HS = H rounded up to a power of two take further KEYS:
// slot = kl * HS + head, the workgroup walks KP = 128 / HS keys per pass (four at H = 32), each key lane kl keeps its own
// online-softmax state over the keys = kl (mod KP) of the piece.  The KP states of a head are merged through LDS by
// halving: the upper half of the key lanes leaves (o, m, l), the lower half folds it in, until key lane 0 holds the
// piece -- a fixed order.  Keys are taken kDecUnroll passes at a time; every load of a step -- rows, scale bytes, mask
// byte -- is issued before anything waits.  score = sum over the blocks of scale_b * (q_b . k_b), block b in lane b, summed
// by two xor-shuffles.  A masked key contributes exactly nothing whatever its nibbles and scale bytes hold: its score
// is -inf by selection, and its bytes and scale bytes are cleared by bit masks before they are converted.
LWM_KERNEL(kDecThreads) void attn_decode_kv4_kernel(Kv4DecodeParams p) {
    const int tid = thread_idx();
    const int slot = tid >> 2, li = tid & 3;
    const int nsplit = p.k_splits > 1 ? p.k_splits : 1;
    const int b = block_idx_x() / nsplit, split = block_idx_x() % nsplit;
    const int per = (p.Sk + nsplit - 1) / nsplit;
    const int k0 = split * per;
    const int k1 = k0 + per < p.Sk ? k0 + per : p.Sk;
    const float c = p.scale * kLog2e;
    const uint8_t* mrow = p.dense_mask ? p.dense_mask + (int64_t)b * p.msk_sb : nullptr;
    const lds_t lds = dyn_lds();

    // visible key range [first, last] of the mask row, partitioned over the pieces (attn_decode.h has the reasoning)
    int ka = k0, kz = k1;
    if (mrow) {
        int first = 0x7fffffff, last = -1;
        const int nvec = (((uintptr_t)mrow & 15) == 0) ? (p.Sk >> 4) : 0;
        for (int i = tid; i < nvec; i += kDecThreads) {
            const u32x4 w = global_load_b128(mrow + 16 * i);
#pragma unroll
            for (int cc = 0; cc < 4; ++cc)
                if (w[cc] != 0u) {
                    const int lo = 16 * i + 4 * cc + (__builtin_ctz(w[cc]) >> 3);
                    const int hi = 16 * i + 4 * cc + ((31 - __builtin_clz(w[cc])) >> 3);
                    first = lo < first ? lo : first;
                    last = hi > last ? hi : last;
                }
        }
        for (int j = 16 * nvec + tid; j < p.Sk; j += kDecThreads)
            if (mrow[j] != 0) {
                first = j < first ? j : first;
                last = j > last ? j : last;
            }
        for (int msk = 1; msk < 64; msk <<= 1) {
            const int of = shfl_xor_i(first, msk), ol = shfl_xor_i(last, msk);
            first = of < first ? of : first;
            last = ol > last ? ol : last;
        }
        if ((tid & 63) == 0) {
            lds_write_i32(lds + (tid >> 6) * 8, first);
            lds_write_i32(lds + (tid >> 6) * 8 + 4, last);
        }
        block_sync();
        for (int w = 0; w < kDecThreads / 64; ++w) {
            const int of = lds_read_i32(lds + w * 8), ol = lds_read_i32(lds + w * 8 + 4);
            first = of < first ? of : first;
            last = ol > last ? ol : last;
        }
        block_sync();                                  // (the merge below reuses these bytes)
        if (last < 0) {
            ka = kz = 0;
        } else {
            const int nv = last - first + 1;
            const int pv = (nv + nsplit - 1) / nsplit;
            ka = first + split * pv;
            kz = ka + pv < last + 1 ? ka + pv : last + 1;
            if (ka > kz) ka = kz;
        }
    }

    int HS = 1;
    while (HS < p.H && HS < kDec4Slots) HS <<= 1;
    const int KP = kDec4Slots / HS;                    // keys per pass
    const int kl = slot / HS, hs = slot % HS;
    const int span = KP * kDecUnroll;                  // keys per step of the workgroup

    for (int h0 = 0; h0 < p.H; h0 += HS) {
        const int h = h0 + hs;
        const bool h_ok = h < p.H;
        const int hc = h_ok ? h : p.H - 1;             // clamped: loads stay in bounds
        f32x2 qf[16], o[16];
        {
            const bf16_t* qp = p.q + (int64_t)b * p.q_sb + (int64_t)hc * p.q_sh + li * 32;
            for (int w = 0; w < 4; ++w) {
                float t[8];
                unpack_bf16x8(global_load_b128(qp + 8 * w), t);
                for (int j = 0; j < 4; ++j) qf[4 * w + j] = f32x2{t[2 * j] * c, t[2 * j + 1] * c};   // scores in log2 units
            }
            for (int j = 0; j < 16; ++j) o[j] = f32x2{0.0f, 0.0f};
        }
        float m = -INFINITY, l = 0.0f;
        const uint8_t* kb = p.k + (int64_t)b * p.k_sb + (int64_t)hc * p.k_sh + li * 16;
        const uint8_t* vb = p.v + (int64_t)b * p.v_sb + (int64_t)hc * p.v_sh + li * 16;
        const uint8_t* ksb = p.k_scale + (int64_t)b * p.ks_sb + hc * 4 + li;
        const uint8_t* vsb = p.v_scale + (int64_t)b * p.vs_sb + hc * 4 + li;
        // every piece starts at a different phase of its key range (see attn_decode.h)
        const int nq = (kz - ka + span - 1) / span;
        const int rot = nq > 0 ? (int)(((uint32_t)block_idx_x() * 2654435761u) >> 8) % nq : 0;
        for (int g = 0; g < nq; ++g) {
            const int gq = g + rot < nq ? g + rot : g + rot - nq;
            const int j0 = ka + gq * span + kl;
            u32x4 kr[kDecUnroll], vr[kDecUnroll];
            uint32_t kse[kDecUnroll], vse[kDecUnroll];
            uint8_t mb[kDecUnroll];
            bool vis[kDecUnroll];
            // every load of the step before anything waits; the mask byte unconditionally (attn_decode_kv8.h): without a
            // mask it comes from the key row, which is valid memory, and is ignored
            for (int u = 0; u < kDecUnroll; ++u) {
                const int jj = j0 + u * KP;
                const int j = jj < kz ? jj : kz - 1;                 // clamped: loads stay in bounds
                const uint8_t* kp = kb + (int64_t)j * p.k_ss;
                kr[u] = global_load_b128(kp);
                vr[u] = global_load_b128(vb + (int64_t)j * p.v_ss);
                kse[u] = global_load_u8(ksb + (int64_t)j * p.ks_ss);
                vse[u] = global_load_u8(vsb + (int64_t)j * p.vs_ss);
                mb[u] = global_load_u8(mrow ? mrow + j : kp);
            }
            issue_fence();
            // a masked key enters as zero nibbles with zero scale bytes and a score of -inf
            float ks[kDecUnroll], vs[kDecUnroll];
            for (int u = 0; u < kDecUnroll; ++u) {
                vis[u] = (j0 + u * KP < kz) & (!mrow | (mb[u] != 0));
                const uint32_t keep = 0u - (uint32_t)vis[u];
                for (int w = 0; w < 4; ++w) {
                    kr[u][w] &= keep;
                    vr[u][w] &= keep;
                }
                ks[u] = e8m0_to_f32(kse[u] & keep);
                vs[u] = e8m0_to_f32(vse[u] & keep);
            }
            float s[kDecUnroll];
            float mx = -INFINITY;
            for (int u = 0; u < kDecUnroll; ++u) {
                f32x2 a2 = {0.0f, 0.0f};
                for (int w = 0; w < 4; ++w) {
                    f32x2 kf[4];
                    cvt_e2m1x8(kr[u][w], kf);
                    for (int j = 0; j < 4; ++j) a2 = fma2(qf[4 * w + j], kf[j], a2);
                }
                float a = (a2[0] + a2[1]) * ks[u];
                a += shfl_xor_f(a, 1);
                a += shfl_xor_f(a, 2);
                s[u] = a + (vis[u] ? 0.0f : -INFINITY);
                mx = fmaxf(mx, s[u]);
            }
            const float m_new = fmaxf(m, mx);
            const float m_safe = m_new == -INFINITY ? 0.0f : m_new;
            const float alpha = fast_exp2(m - m_safe);
            l *= alpha;
            for (int j = 0; j < 16; ++j) o[j] *= alpha;
            for (int u = 0; u < kDecUnroll; ++u) {
                const float pu = fast_exp2(s[u] - m_safe);     // 0 for a masked key
                l += pu;
                const float pv = pu * vs[u];
                const f32x2 pv2 = {pv, pv};
                for (int w = 0; w < 4; ++w) {
                    f32x2 vf[4];
                    cvt_e2m1x8(vr[u][w], vf);
                    for (int j = 0; j < 4; ++j) o[4 * w + j] = fma2(pv2, vf[j], o[4 * w + j]);
                }
            }
            m = m_new;
        }
        // merge the KP key lanes of each head by halving: key lanes [half, 2 half) leave (o, m, l), unnormalised, in LDS;
        // key lanes [0, half) fold in the state of key lane kl + half
        for (int half = KP >> 1; half >= 1; half >>= 1) {
            const bool give = kl >= half && kl < 2 * half, take = kl < half;
            const uint32_t idx = (uint32_t)(give ? slot - half * HS : slot) & (kDec4Slots / 2 - 1);
            const lds_t so = lds + idx * (kHeadDim * 4) + (uint32_t)li * 128;
            const lds_t sm = lds + (kDec4Slots / 2) * kHeadDim * 4 + idx * 8;
            if (give) {
                for (int w = 0; w < 8; ++w)
                    lds_write_f32x4(so + 16 * w, f32x4{o[2 * w][0], o[2 * w][1], o[2 * w + 1][0], o[2 * w + 1][1]});
                if (li == 0) {
                    lds_write_f32(sm, m);
                    lds_write_f32(sm + 4, l);
                }
            }
            block_sync();
            if (take) {
                const float m2 = lds_read_f32(sm), l2 = lds_read_f32(sm + 4);
                const float m_new = fmaxf(m, m2);
                const float m_safe = m_new == -INFINITY ? 0.0f : m_new;
                const float a1 = fast_exp2(m - m_safe), a2 = fast_exp2(m2 - m_safe);
                l = l * a1 + l2 * a2;
                for (int w = 0; w < 8; ++w) {
                    const f32x4 ov = lds_read_f32x4(so + 16 * w);
                    o[2 * w] = o[2 * w] * a1 + f32x2{ov[0], ov[1]} * a2;
                    o[2 * w + 1] = o[2 * w + 1] * a1 + f32x2{ov[2], ov[3]} * a2;
                }
                m = m_new;
            }
            block_sync();                              // (the next round, and the next pass over heads, write the same bytes)
        }
        if (h_ok && kl == 0) {
            const float inv = l > 0.0f ? 1.0f / l : 0.0f;
            float* op = p.out_acc + (((int64_t)split * p.B + b) * p.H + h) * kHeadDim + li * 32;
            for (int w = 0; w < 8; ++w)
                global_store_f32x4(op + 4 * w, f32x4{o[2 * w][0] * inv, o[2 * w][1] * inv, o[2 * w + 1][0] * inv, o[2 * w + 1][1] * inv});
            if (li == 0)   // m, l are in log2 units: lse = (m + log2 l) * ln 2
                global_store_f32(p.lse_acc + ((int64_t)split * p.B + b) * p.H + h, l > 0.0f ? (m + fast_log2(l)) * kLn2 : -INFINITY);
        }
    }
}

}  // namespace lwm
