// attn_decode_kvq.h -- what the quantised KV caches share: the quantising cache write and the cached-decode attention
// kernel, written once over a compile-time description of the format.  Requires wave_ops.h + attn_common.h +
// attn_decode.h (unpack_bf16x8, decode_visible_range, f32x2, fma2, issue_fence, the scalar loads and stores).  The
// formats -- their layout, codec and description struct, and the __global__ entry points -- are attn_decode_kv8.h,
// attn_decode_kv4.h and attn_decode_kv6.h.
//
// A format description F has only static members:
//   scale_t                         element type of the scale tensors
//   kHeadBytes                      bytes of one head of one cache row
//   write: kAmaxLanes               of the 16 lanes that own a head in the write (8 elements each), how many share a scale
//          kExpDrop, kMantTop       amax = 1.m * 2^e gets the scale 2^(e - kExpDrop), one more where the 7 bits of m > kMantTop
//          scale_of(se)             the biased exponent of the scale -> the stored scale_t
//          encode(y)                the lane's 8 scaled values -> their codes, one or two dwords
//          store(head, li, w, ok)   the lane's codes -> their bytes of the head row at `head`, where ok (every lane of the
//                                   wave calls it: a format may shuffle)
//   decode: kLanes                  lanes that own a head (128 / kLanes elements and kLaneDwords dwords of each row per lane)
//           kLaneDwords, codes_t    the lane's dwords of one row, and the vector of them
//           load_lane(ptr)          the lane's codes of one row (naturally aligned loads)
//           scale_index(h, li)      index of the lane's scale among the scales of one row
//           load_scale(ptr)         the scale's bits; zero bits stand for a masked key
//           scale_f32(bits)         (cleared) bits -> f32
//           cvt_lane(w, f)          the lane's codes -> its 128 / kLanes / 2 f32 pairs, element order
//           scale_lane(a, ks)       the lane's partial score before the reduction over the lanes of the head ...
//           scale_head(a, ks)       ... and the head's score after it: one of the two multiplies by ks
#pragma once

// a static member function of a format description (LWM_DEVICE is already `static` in the host emulation)
#ifdef LWM_EMU
#define LWM_FORMAT_FN LWM_DEVICE
#else
#define LWM_FORMAT_FN static LWM_DEVICE
#endif

namespace lwm {

// ------------------------------------------------------------------ quantising cache write
template <class F>
struct KvqWriteParams {
    uint8_t* cache;            // (B, cache_rows, H, kHeadBytes) codes
    typename F::scale_t* scale;  // (B, cache_rows, H [, scales per head])
    const bf16_t* src;         // (B, *, H, 128) bf16
    int64_t cache_sb, scale_sb, src_sb;     // batch strides, elements of their tensors
    const int32_t* row0_dev;   // the _at form: destination row = *row0_dev + dst_row0 + i
    int64_t dst_row0;          // destination row of source row src_row0 (the _at form: the offset added to *row0_dev)
    int64_t cache_rows;        // rows outside [0, cache_rows) are skipped
    int64_t src_row0, nrows;
    int32_t B, H;
};

// 16 lanes own one head of one row: lane i holds elements 8i..8i+7 (one 16-byte load).  The integer amax of the bf16 bit
// patterns is reduced with xor-shuffles over the kAmaxLanes lanes that share a scale; each lane stores its 8 codes and the
// first lane of a group the scale.  Every lane of a wave runs every shuffle (the trip count is uniform over the
// workgroup; what a lane may not do is decided at the loads and stores).
LWM_DEVICE void store_codes(uint8_t* p, uint32_t w) { global_store_b32(p, w); }
LWM_DEVICE void store_codes(uint8_t* p, u32x2 w) { global_store_b64(p, w); }
// F::store of a format whose lane's 8 codes are one naturally aligned unit: kHeadBytes / 16 bytes at li * that
template <class F, class W>
LWM_DEVICE void store_lane_codes(uint8_t* head, int li, W w, bool ok) {
    if (ok) store_codes(head + li * (F::kHeadBytes / 16), w);
}

template <class F>
LWM_DEVICE void kv_quant_rows(const KvqWriteParams<F>& p, int64_t dst_row0) {
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
        for (int msk = 1; msk < F::kAmaxLanes; msk <<= 1) {
            const int o = shfl_xor_i(am, msk);
            am = o > am ? o : am;
        }
        // biased exponent of the scale (the format's header has the rule), clamped to 2^-126 below; finite bf16 inputs
        // stay under the upper clamp by themselves
        int se = 127;
        if (am != 0) {
            se = (am >> 7) - F::kExpDrop + ((am & 0x7f) > F::kMantTop ? 1 : 0);
            se = se < 1 ? 1 : se;
        }
        const float inv = __builtin_bit_cast(float, (uint32_t)(254 - se) << 23);
        float x[8];
        unpack_bf16x8(raw, x);
        for (int j = 0; j < 8; ++j) x[j] *= inv;
        const auto w = F::encode(x);
        const typename F::scale_t s = F::scale_of(se);
        const bool ok = in && dr >= 0 && dr < p.cache_rows;
        F::store(p.cache + b * p.cache_sb + (dr * p.H + h) * F::kHeadBytes, li, w, ok);
        if (ok && (li & (F::kAmaxLanes - 1)) == 0)
            p.scale[b * p.scale_sb + (dr * p.H + h) * (16 / F::kAmaxLanes) + li / F::kAmaxLanes] = s;
    }
}

// ------------------------------------------------------------------ decode attention over a quantised cache
template <class F>
struct KvqDecodeParams {
    const bf16_t* q;           // (B, 1, H, 128) bf16
    const uint8_t* k;          // codes
    const uint8_t* v;
    const typename F::scale_t* k_scale;
    const typename F::scale_t* v_scale;
    int64_t q_sb, q_sh;
    int64_t k_sb, k_ss, k_sh;  // bytes
    int64_t v_sb, v_ss, v_sh;
    int64_t ks_sb, ks_ss;      // scales, in scale_t elements: the scales of a head and the heads of a row contiguous
    int64_t vs_sb, vs_ss;
    const uint8_t* dense_mask; // (B, Sk) u8 or null
    int64_t msk_sb;
    int32_t B, Sk, H, k_splits;
    float scale;
    float* out_acc;            // [k_splits, B, 1, H, 128] f32 normalised partials
    float* lse_acc;            // [k_splits, B, H, 1]
};

template <class F>
constexpr int kDecqSlots = kDecThreads / F::kLanes;                         // head slots of the workgroup
template <class F>
constexpr int kDecqLdsBytes = (kDecqSlots<F> / 2) * (kHeadDim + 2) * 4;     // the merge of the key lanes: half the slots leave o[128], m, l

// The same contract as attn_decode_kernel -- one workgroup per (batch row, piece of the VISIBLE key range), holes
// handled per key, per-piece phase rotation, normalised partials merged by attn_combine_kernel, nothing visible =
// (0, -inf) -- over smaller rows.  kLanes lanes x kLaneDwords dwords own a head row (lane i holds the 128 / kLanes elements
// from i * 128 / kLanes on of q, of the running output and of each K/V row) and the workgroup has 512 / kLanes head slots.
// Where H is smaller the slots beyond the first HS = H rounded up to a power of two take further KEYS:
// slot = kl * HS + head, the workgroup walks KP = slots / HS keys per pass (a wave load is still 1 KiB contiguous), each
// key lane kl keeps its own online-softmax state over the keys = kl (mod KP) of the piece.  The KP states of a head are
// merged through LDS by halving: the upper half of the key lanes leaves (o, m, l), the lower half folds it in, until
// key lane 0 holds the piece -- a fixed order.  Keys are taken kDecUnroll passes at a time: 8 row loads of a lane's
// width in flight per lane (16 bytes each as in the bf16 kernel, or 24 as three 8-byte loads).  The scales of a (key, head) are loaded WITH its rows -- their addresses depend
// on nothing the rows bring -- and p_v = p * value_scale.  A masked key contributes exactly nothing whatever its bytes
// and scales hold (NaN patterns, NaN scales): its score is -inf by selection and its rows and scale bits are cleared by
// bit masks before they are converted.
template <class F>
LWM_DEVICE void attn_decode_kvq(const KvqDecodeParams<F>& p) {
    constexpr int L = F::kLanes, S = kDecqSlots<F>;
    constexpr int E = kHeadDim / L;                    // elements of a head per lane,
    constexpr int NP = E / 2;                          // NP pairs of q, of o and of a converted row
    constexpr int W = F::kLaneDwords;
    typedef typename F::codes_t codes_t;
    const int tid = thread_idx();
    const int slot = (int)((uint32_t)tid / L), li = (int)((uint32_t)tid % L);
    const int nsplit = p.k_splits > 1 ? p.k_splits : 1;
    const int b = block_idx_x() / nsplit, split = block_idx_x() % nsplit;
    const float c = p.scale * kLog2e;
    const uint8_t* mrow = p.dense_mask ? p.dense_mask + (int64_t)b * p.msk_sb : nullptr;
    const lds_t lds = dyn_lds();

    int ka, kz;
    decode_visible_range(mrow, p.Sk, split, nsplit, lds, ka, kz);
    if (mrow) block_sync();                            // (the merge below reuses the scan's bytes)

    int HS = 1;
    while (HS < p.H && HS < S) HS <<= 1;
    const int KP = S / HS;                             // keys per pass
    const int kl = slot / HS, hs = slot % HS;
    const int span = KP * kDecUnroll;                  // keys per step of the workgroup

    for (int h0 = 0; h0 < p.H; h0 += HS) {
        const int h = h0 + hs;
        const bool h_ok = h < p.H;
        const int hc = h_ok ? h : p.H - 1;             // clamped: loads stay in bounds
        f32x2 qf[NP], o[NP];
        {
            const bf16_t* qp = p.q + (int64_t)b * p.q_sb + (int64_t)hc * p.q_sh + li * E;
            for (int w = 0; w < E / 8; ++w) {
                float t[8];
                unpack_bf16x8(global_load_b128(qp + 8 * w), t);
                for (int j = 0; j < 4; ++j) qf[4 * w + j] = f32x2{t[2 * j] * c, t[2 * j + 1] * c};   // scores in log2 units
            }
            for (int j = 0; j < NP; ++j) o[j] = f32x2{0.0f, 0.0f};
        }
        float m = -INFINITY, l = 0.0f;
        const uint8_t* kb = p.k + (int64_t)b * p.k_sb + (int64_t)hc * p.k_sh + li * (W * 4);
        const uint8_t* vb = p.v + (int64_t)b * p.v_sb + (int64_t)hc * p.v_sh + li * (W * 4);
        const typename F::scale_t* ksb = p.k_scale + (int64_t)b * p.ks_sb + F::scale_index(hc, li);
        const typename F::scale_t* vsb = p.v_scale + (int64_t)b * p.vs_sb + F::scale_index(hc, li);
        // every piece starts at a different phase of its key range (see attn_decode.h)
        const int nq = (kz - ka + span - 1) / span;
        const int rot = nq > 0 ? (int)(((uint32_t)block_idx_x() * 2654435761u) >> 8) % nq : 0;
        for (int g = 0; g < nq; ++g) {
            const int gq = g + rot < nq ? g + rot : g + rot - nq;
            const int j0 = ka + gq * span + kl;
            codes_t kr[kDecUnroll], vr[kDecUnroll];
            uint32_t ksw[kDecUnroll], vsw[kDecUnroll];
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
                kr[u] = F::load_lane(kp);
                vr[u] = F::load_lane(vb + (int64_t)j * p.v_ss);
                ksw[u] = F::load_scale(ksb + (int64_t)j * p.ks_ss);
                vsw[u] = F::load_scale(vsb + (int64_t)j * p.vs_ss);
                mb[u] = global_load_u8(mrow ? mrow + j : kp);
            }
            issue_fence();
            // a masked key enters as a row of zeros with zero scales and a score of -inf, by bit masks and one
            // constant select: nothing below depends on what its bytes and scales hold
            float ks[kDecUnroll], vs[kDecUnroll];
            for (int u = 0; u < kDecUnroll; ++u) {
                vis[u] = (j0 + u * KP < kz) & (!mrow | (mb[u] != 0));
                const uint32_t keep = 0u - (uint32_t)vis[u];
                for (int w = 0; w < W; ++w) {
                    kr[u][w] &= keep;
                    vr[u][w] &= keep;
                }
                ks[u] = F::scale_f32(ksw[u] & keep);
                vs[u] = F::scale_f32(vsw[u] & keep);
            }
            float s[kDecUnroll];
            float mx = -INFINITY;
            for (int u = 0; u < kDecUnroll; ++u) {
                f32x2 a2 = {0.0f, 0.0f};
                f32x2 kf[NP];
                F::cvt_lane(kr[u], kf);
                for (int j = 0; j < NP; ++j) a2 = fma2(qf[j], kf[j], a2);
                float a = F::scale_lane(a2[0] + a2[1], ks[u]);
#pragma unroll
                for (int msk = 1; msk < L; msk <<= 1) a += shfl_xor_f(a, msk);
                s[u] = F::scale_head(a, ks[u]) + (vis[u] ? 0.0f : -INFINITY);
                mx = fmaxf(mx, s[u]);
            }
            const float m_new = fmaxf(m, mx);
            const float m_safe = m_new == -INFINITY ? 0.0f : m_new;
            const float alpha = fast_exp2(m - m_safe);
            l *= alpha;
            for (int j = 0; j < NP; ++j) o[j] *= alpha;
            for (int u = 0; u < kDecUnroll; ++u) {
                const float pu = fast_exp2(s[u] - m_safe);     // 0 for a masked key
                l += pu;
                const float pv = pu * vs[u];
                const f32x2 pv2 = {pv, pv};
                f32x2 vf[NP];
                F::cvt_lane(vr[u], vf);
                for (int j = 0; j < NP; ++j) o[j] = fma2(pv2, vf[j], o[j]);
            }
            m = m_new;
        }
        // merge the KP key lanes of each head by halving: key lanes [half, 2 half) leave (o, m, l), unnormalised, in LDS;
        // key lanes [0, half) fold in the state of key lane kl + half
        for (int half = KP >> 1; half >= 1; half >>= 1) {
            const bool give = kl >= half && kl < 2 * half, take = kl < half;
            const uint32_t idx = (uint32_t)(give ? slot - half * HS : slot) & (S / 2 - 1);
            const lds_t so = lds + idx * (kHeadDim * 4) + (uint32_t)li * (E * 4);
            const lds_t sm = lds + (S / 2) * kHeadDim * 4 + idx * 8;
            if (give) {
                for (int w = 0; w < NP / 2; ++w)
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
                // o * a1 + other * a2, with the product that is rounded before the sum written out (left to contraction, it
                // changed with the register allocation): the other state's in the even pairs, the lane's own in the odd ones
                const f32x2 a1v = {a1, a1}, a2v = {a2, a2};
                for (int w = 0; w < NP / 2; ++w) {
                    const f32x4 ov = lds_read_f32x4(so + 16 * w);
                    o[2 * w] = mad2(o[2 * w], a1v, f32x2{ov[0], ov[1]} * a2v);
                    o[2 * w + 1] = mad2(f32x2{ov[2], ov[3]}, a2v, o[2 * w + 1] * a1v);
                }
                m = m_new;
            }
            block_sync();                              // (the next round, and the next pass over heads, write the same bytes)
        }
        if (h_ok && kl == 0) {
            const float inv = l > 0.0f ? 1.0f / l : 0.0f;
            float* op = p.out_acc + (((int64_t)split * p.B + b) * p.H + h) * kHeadDim + li * E;
            for (int w = 0; w < NP / 2; ++w)
                global_store_f32x4(op + 4 * w, f32x4{o[2 * w][0] * inv, o[2 * w][1] * inv, o[2 * w + 1][0] * inv, o[2 * w + 1][1] * inv});
            if (li == 0)   // m, l are in log2 units: lse = (m + log2 l) * ln 2
                global_store_f32(p.lse_acc + ((int64_t)split * p.B + b) * p.H + h, l > 0.0f ? (m + fast_log2(l)) * kLn2 : -INFINITY);
        }
    }
}

}  // namespace lwm
