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

typedef float f32x2 __attribute__((ext_vector_type(2)));

// ---- primitives of this header (the shared vocabulary of wave_ops.h is pinned to the counter profile)
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
LWM_DEVICE f32x2 fma2(f32x2 a, f32x2 b, f32x2 c) { return f32x2{fmaf(a[0], b[0], c[0]), fmaf(a[1], b[1], c[1])}; }
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
// v_pk_fma_f32: the register pairs the packed conversion leaves are its operands as they are
LWM_DEVICE f32x2 fma2(f32x2 a, f32x2 b, f32x2 c) { return __builtin_elementwise_fma(a, b, c); }
#endif
// The loads written above this point are ISSUED above it: the optimiser may neither sink one below it (into the branch
// of its first use, behind a wait for everything outstanding) nor hoist later work between them.  No instruction.
LWM_DEVICE void issue_fence() {
    asm volatile("" ::: "memory");
    sched_fence();
}
LWM_DEVICE float global_load_f32(const float* p) { return *p; }
LWM_DEVICE uint8_t global_load_u8(const uint8_t* p) { return *p; }
LWM_DEVICE void global_store_f32(float* p, float v) { *p = v; }

// ------------------------------------------------------------------ quantising cache write
struct Kv8WriteParams {
    uint8_t* cache;            // (B, cache_rows, H, 128) e4m3 bytes
    float* scale;              // (B, cache_rows, H)
    const bf16_t* src;         // (B, *, H, 128) bf16
    int64_t cache_sb, scale_sb, src_sb;     // batch strides, elements
    const int32_t* row0_dev;   // the _at form: destination row = *row0_dev + dst_row0 + i
    int64_t dst_row0;          // destination row of source row src_row0 (the _at form: the offset added to *row0_dev)
    int64_t cache_rows;        // rows outside [0, cache_rows) are skipped
    int64_t src_row0, nrows;
    int32_t B, H;
};

// 16 lanes own one head of one row: lane i holds elements 8i..8i+7 (one 16-byte load), amax is reduced with four
// xor-shuffles inside the group, and each lane stores its 8 bytes.  Every lane of a wave runs every shuffle (the
// trip count is uniform over the workgroup; what a lane may not do is decided at the loads and stores).
LWM_DEVICE void kv8_quant_rows(const Kv8WriteParams& p, int64_t dst_row0) {
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
        // |x| as integers: bf16 magnitudes order like their bit patterns (and no denormal mode has a say)
        int am = 0;
        for (int c = 0; c < 4; ++c) {
            const int lo = (int)(raw[c] & 0x7fffu), hi = (int)((raw[c] >> 16) & 0x7fffu);
            am = lo > am ? lo : am;
            am = hi > am ? hi : am;
        }
        for (int msk = 1; msk < 16; msk <<= 1) {
            const int o = shfl_xor_i(am, msk);
            am = o > am ? o : am;
        }
        // amax = 1.m * 2^e: the smallest power of two s with amax / s <= 448 = 1.75 * 2^8 is 2^(e-8) when 1.m <= 1.75 and
        // 2^(e-7) otherwise.  Biased exponent of s, clamped to 2^-126 below (finite bf16 inputs stay under the upper
        // clamp of 2^127 by themselves: e <= 127 gives s <= 2^120).
        int se = 127;
        if (am != 0) {
            se = (am >> 7) - 8 + ((am & 0x7f) > 0x60 ? 1 : 0);
            se = se < 1 ? 1 : se;
        }
        const float s = __builtin_bit_cast(float, (uint32_t)se << 23);
        const float inv = __builtin_bit_cast(float, (uint32_t)(254 - se) << 23);
        float x[8];
        unpack_bf16x8(raw, x);
        u32x2 w;
        w[0] = pack_e4m3x4(x[0] * inv, x[1] * inv, x[2] * inv, x[3] * inv);
        w[1] = pack_e4m3x4(x[4] * inv, x[5] * inv, x[6] * inv, x[7] * inv);
        if (in && dr >= 0 && dr < p.cache_rows) {
            global_store_b64(p.cache + b * p.cache_sb + (dr * p.H + h) * kHeadDim + li * 8, w);
            if (li == 0) global_store_f32(p.scale + b * p.scale_sb + dr * p.H + h, s);
        }
    }
}

LWM_KERNEL(256) void kv8_quant_write_kernel(Kv8WriteParams p) { kv8_quant_rows(p, p.dst_row0); }
// The destination row from DEVICE memory, as kv_cache_write_at_kernel: nothing about a decode step depends on a host
// value, so the step can be captured in a hipGraph and replayed while the index advances on the device.
LWM_KERNEL(256) void kv8_quant_write_at_kernel(Kv8WriteParams p) { kv8_quant_rows(p, (int64_t)p.row0_dev[0] + p.dst_row0); }

// ------------------------------------------------------------------ decode attention over the 8-bit cache
struct Kv8DecodeParams {
    const bf16_t* q;           // (B, 1, H, 128) bf16
    const uint8_t* k;          // e4m3 bytes
    const uint8_t* v;
    const float* k_scale;
    const float* v_scale;
    int64_t q_sb, q_sh;
    int64_t k_sb, k_ss, k_sh;  // elements = bytes
    int64_t v_sb, v_ss, v_sh;
    int64_t ks_sb, ks_ss;      // scales: heads contiguous
    int64_t vs_sb, vs_ss;
    const uint8_t* dense_mask; // (B, Sk) u8 or null
    int64_t msk_sb;
    int32_t B, Sk, H, k_splits;
    float scale;
    float* out_acc;            // [k_splits, B, 1, H, 128] f32 normalised partials
    float* lse_acc;            // [k_splits, B, H, 1]
};

constexpr int kDec8Slots = kDecThreads / 8;                       // 64 head slots of 8 lanes
constexpr int kDec8LdsBytes = kDec8Slots * (kHeadDim + 2) * 4;    // the merge of the key lanes: o[128], m, l per slot

// The same contract as attn_decode_kernel -- one workgroup per (batch row, piece of the VISIBLE key range), holes
// handled per key, per-piece phase rotation, normalised partials merged by attn_combine_kernel, nothing visible =
// (0, -inf) -- over rows of half the size.  A head row is 128 B, so 8 lanes x 16 B own it (lane i holds d = 16i..16i+15
// of q, of the running output and of each K/V row) and the workgroup has 64 head slots.  Where H < 64 the slots beyond
// the first HS = H rounded up to a power of two take further KEYS: slot = kl * HS + head, the workgroup walks
// KP = 64 / HS keys per pass (two at H = 32: a wave load is still 1 KiB contiguous, one key's 8 heads), each key lane kl
// keeps its own online-softmax state over the keys = kl (mod KP) of the piece, and the KP states of a head are merged
// through LDS, in key-lane order, before the partial is written.  Keys are taken kDecUnroll passes at a time: 8 x 16-byte
// row loads in flight per lane as in the bf16 kernel, over twice the keys.  The two scales of a (key, head) are loaded
// WITH its rows -- their addresses depend on nothing the rows bring -- and enter as scalars:
// score = (q . k_q) * key_scale, p_v = p * value_scale.  A masked key contributes exactly nothing whatever its bytes
// and scales hold (e4m3 NaN patterns, NaN scales): its score is -inf by selection and its value row and scale are
// replaced by zeros before they are used.
LWM_KERNEL(kDecThreads) void attn_decode_kv8_kernel(Kv8DecodeParams p) {
    const int tid = thread_idx();
    const int slot = tid >> 3, li = tid & 7;
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
    while (HS < p.H && HS < kDec8Slots) HS <<= 1;
    const int KP = kDec8Slots / HS;                    // keys per pass
    const int kl = slot / HS, hs = slot % HS;
    const int span = KP * kDecUnroll;                  // keys per step of the workgroup

    for (int h0 = 0; h0 < p.H; h0 += HS) {
        const int h = h0 + hs;
        const bool h_ok = h < p.H;
        const int hc = h_ok ? h : p.H - 1;             // clamped: loads stay in bounds
        f32x2 qf[8], o[8];
        {
            const bf16_t* qp = p.q + (int64_t)b * p.q_sb + (int64_t)hc * p.q_sh + li * 16;
            float t0[8], t1[8];
            unpack_bf16x8(global_load_b128(qp), t0);
            unpack_bf16x8(global_load_b128(qp + 8), t1);
            for (int j = 0; j < 4; ++j) {              // scores directly in log2 units
                qf[j] = f32x2{t0[2 * j] * c, t0[2 * j + 1] * c};
                qf[4 + j] = f32x2{t1[2 * j] * c, t1[2 * j + 1] * c};
            }
            for (int j = 0; j < 8; ++j) o[j] = f32x2{0.0f, 0.0f};
        }
        float m = -INFINITY, l = 0.0f;
        const uint8_t* kb = p.k + (int64_t)b * p.k_sb + (int64_t)hc * p.k_sh + li * 16;
        const uint8_t* vb = p.v + (int64_t)b * p.v_sb + (int64_t)hc * p.v_sh + li * 16;
        const float* ksb = p.k_scale + (int64_t)b * p.ks_sb + hc;
        const float* vsb = p.v_scale + (int64_t)b * p.vs_sb + hc;
        // every piece starts at a different phase of its key range (see attn_decode.h)
        const int nq = (kz - ka + span - 1) / span;
        const int rot = nq > 0 ? (int)(((uint32_t)block_idx_x() * 2654435761u) >> 8) % nq : 0;
        for (int g = 0; g < nq; ++g) {
            const int gq = g + rot < nq ? g + rot : g + rot - nq;
            const int j0 = ka + gq * span + kl;
            u32x4 kr[kDecUnroll], vr[kDecUnroll];
            float ks[kDecUnroll], vs[kDecUnroll];
            uint8_t mb[kDecUnroll];
            bool vis[kDecUnroll];
            // Every load of the step is issued before anything waits: the mask byte is loaded unconditionally (a load
            // under `jj < kz && ...` is a branch with a wait for ALL outstanding loads behind it, which turns the
            // step's rows into kDecUnroll dependent round trips); without a mask the byte comes from the key row,
            // which is valid memory, and is ignored.
            for (int u = 0; u < kDecUnroll; ++u) {
                const int jj = j0 + u * KP;
                const int j = jj < kz ? jj : kz - 1;                 // clamped: loads stay in bounds
                const uint8_t* kp = kb + (int64_t)j * p.k_ss;
                kr[u] = global_load_b128(kp);
                vr[u] = global_load_b128(vb + (int64_t)j * p.v_ss);
                ks[u] = global_load_f32(ksb + (int64_t)j * p.ks_ss);
                vs[u] = global_load_f32(vsb + (int64_t)j * p.vs_ss);
                mb[u] = global_load_u8(mrow ? mrow + j : kp);
            }
            issue_fence();
            // a masked key enters as a row of zeros with zero scales and a score of -inf, by bit masks and one
            // constant select: nothing below depends on what its bytes and scales hold
            for (int u = 0; u < kDecUnroll; ++u) {
                vis[u] = (j0 + u * KP < kz) & (!mrow | (mb[u] != 0));
                const uint32_t keep = 0u - (uint32_t)vis[u];
                for (int w = 0; w < 4; ++w) {
                    kr[u][w] &= keep;
                    vr[u][w] &= keep;
                }
                ks[u] = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, ks[u]) & keep);
                vs[u] = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, vs[u]) & keep);
            }
            float s[kDecUnroll];
            float mx = -INFINITY;
            for (int u = 0; u < kDecUnroll; ++u) {
                f32x2 a2 = {0.0f, 0.0f};
                for (int w = 0; w < 4; ++w) {
                    a2 = fma2(qf[2 * w], cvt_e4m3x2_lo(kr[u][w]), a2);
                    a2 = fma2(qf[2 * w + 1], cvt_e4m3x2_hi(kr[u][w]), a2);
                }
                float a = a2[0] + a2[1];
                a += shfl_xor_f(a, 1);
                a += shfl_xor_f(a, 2);
                a += shfl_xor_f(a, 4);
                s[u] = a * ks[u] + (vis[u] ? 0.0f : -INFINITY);
                mx = fmaxf(mx, s[u]);
            }
            const float m_new = fmaxf(m, mx);
            const float m_safe = m_new == -INFINITY ? 0.0f : m_new;
            const float alpha = fast_exp2(m - m_safe);
            l *= alpha;
            for (int j = 0; j < 8; ++j) o[j] *= alpha;
            for (int u = 0; u < kDecUnroll; ++u) {
                const float pu = fast_exp2(s[u] - m_safe);     // 0 for a masked key
                l += pu;
                const float pv = pu * vs[u];
                const f32x2 pv2 = {pv, pv};
                for (int w = 0; w < 4; ++w) {
                    o[2 * w] = fma2(pv2, cvt_e4m3x2_lo(vr[u][w]), o[2 * w]);
                    o[2 * w + 1] = fma2(pv2, cvt_e4m3x2_hi(vr[u][w]), o[2 * w + 1]);
                }
            }
            m = m_new;
        }
        // merge the KP key lanes of each head: lanes kl > 0 leave (o, m, l), unnormalised, in LDS; lane 0 folds them
        // in, in key-lane order
        if (KP > 1) {
            const lds_t so = lds + (uint32_t)slot * (kHeadDim * 4) + (uint32_t)li * 64;
            const lds_t sm = lds + kDec8Slots * kHeadDim * 4 + (uint32_t)slot * 8;
            if (kl > 0) {
                for (int w = 0; w < 4; ++w)
                    lds_write_f32x4(so + 16 * w, f32x4{o[2 * w][0], o[2 * w][1], o[2 * w + 1][0], o[2 * w + 1][1]});
                if (li == 0) {
                    lds_write_f32(sm, m);
                    lds_write_f32(sm + 4, l);
                }
            }
            block_sync();
            if (kl == 0) {
                for (int t = 1; t < KP; ++t) {
                    const uint32_t other = (uint32_t)(t * HS) * (kHeadDim * 4);
                    const float m2 = lds_read_f32(sm + (uint32_t)(t * HS) * 8), l2 = lds_read_f32(sm + (uint32_t)(t * HS) * 8 + 4);
                    const float m_new = fmaxf(m, m2);
                    const float m_safe = m_new == -INFINITY ? 0.0f : m_new;
                    const float a1 = fast_exp2(m - m_safe), a2 = fast_exp2(m2 - m_safe);
                    l = l * a1 + l2 * a2;
                    for (int w = 0; w < 4; ++w) {
                        const f32x4 ov = lds_read_f32x4(so + other + 16 * w);
                        o[2 * w] = o[2 * w] * a1 + f32x2{ov[0], ov[1]} * a2;
                        o[2 * w + 1] = o[2 * w + 1] * a1 + f32x2{ov[2], ov[3]} * a2;
                    }
                    m = m_new;
                }
            }
            block_sync();                              // (the next pass over heads writes the same bytes)
        }
        if (h_ok && kl == 0) {
            const float inv = l > 0.0f ? 1.0f / l : 0.0f;
            float* op = p.out_acc + (((int64_t)split * p.B + b) * p.H + h) * kHeadDim + li * 16;
            for (int w = 0; w < 4; ++w)
                global_store_f32x4(op + 4 * w, f32x4{o[2 * w][0] * inv, o[2 * w][1] * inv, o[2 * w + 1][0] * inv, o[2 * w + 1][1] * inv});
            if (li == 0)   // m, l are in log2 units: lse = (m + log2 l) * ln 2
                global_store_f32(p.lse_acc + ((int64_t)split * p.B + b) * p.H + h, l > 0.0f ? (m + fast_log2(l)) * kLn2 : -INFINITY);
        }
    }
}

}  // namespace lwm
