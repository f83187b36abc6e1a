// attn_prefill_kv8.h -- attention of a BLOCK of queries over the 8-bit (e4m3) KV cache: chunked prefill, a follow-up
// turn, a block appended to a live cache.  Requires wave_ops.h + attn_common.h + attn_fwd.h + attn_decode.h
// (f32x2, issue_fence, global_load_u8, global_load_f32, global_load_b64) + attn_decode_kv8.h (the format,
// cvt_e4m3x2_lo/hi).
//
// The kernel is attn_fwd_body (attn_fwd.h) in its split-K partials form -- 512 threads, 256 queries per workgroup,
// 64-key LDS tiles, the same workgroup -> (q tile, head, batch, split) map, causal tile range and split walk, and
// fwd_tile<BUF> (fwd_phase_s / fwd_phase_softmax / fwd_phase_pv) called as it is -- with ONE part replaced: the
// staging.  K and V arrive as e4m3 bytes with one f32 scale per (row, head) and are dequantised between the global load
// and the LDS write; q * s is exactly representable in bf16 (attn_decode_kv8.h), so the LDS tiles are bit for bit the
// tiles attn_fwd_body stages from a bf16 copy of the cache, and everything after the staging is the arithmetic of that
// kernel.  No bf16 copy of a cache row ever exists in HBM.
//
// A key that is masked (key_valid == 0) or lies at or past Sk is staged as a row of zeros and its key-meta word is
// kSegInvalid: whatever its bytes and scales hold (e4m3 NaN patterns, NaN or Inf scales) reaches nothing -- they are
// cleared with bit masks before the conversion.
#pragma once

namespace lwm {

// The parameters of a block kernel over a quantised cache whose scales are scale_t (here float, one per (row, head);
// attn_prefill_kv6.h: e8m0 bytes, 4 per (row, head)).  One struct, so that api.inc fills it in one place.
template <class scale_t>
struct KvqPrefillParams {
    AttnParams a;              // q, out_acc, lse_acc, key_valid, B/H/Sq/Sk, q_start, scale, k_splits; causal = 1, final_out = carry_in = 0
    const uint8_t* k;          // codes (B,Sk,H,head bytes)
    const uint8_t* v;
    const scale_t* k_scale;    // (B,Sk,H [, scales per head])
    const scale_t* v_scale;
    int64_t k_sb, k_ss, k_sh;  // bytes
    int64_t v_sb, v_ss, v_sh;
    int64_t ks_sb, ks_ss;      // scale_t elements; the scales of a head and the heads of a row contiguous
    int64_t vs_sb, vs_ss;
    int64_t kv_sb;             // key_valid: bytes between batch rows
};
typedef KvqPrefillParams<float> Kv8PrefillParams;

// what one thread holds of the next tile between its loads and its LDS writes: 8 K bytes and 8 V bytes of each of its
// two rows (attn_fwd.h: 16 bytes of bf16 each), the rows' scales and validity bytes; threads < 64 also the key-meta byte
struct Fwd8Stage {
    u32x2 k[2];
    u32x2 v[2];
    float ks[2], vs[2];
    uint8_t ok[2];
    uint8_t kvalid;
};

// Every load of the tile is issued before anything waits (fwd_stage_load has the reasoning): the key-meta byte first,
// then rows, scales and validity bytes, all at addresses that depend on nothing a load brings.  Rows at or past Sk
// re-read the last row and are cleared at the write.  Without a key_valid tensor the validity byte is read from the
// key row (valid memory) and ignored: an unconditional load, no branch with a wait behind it.
LWM_DEVICE void fwd8_stage_load(const Kv8PrefillParams& p, const uint8_t* kb, const uint8_t* vb, const float* ksb,
                                const float* vsb, const uint8_t* kvb, int kt, int tid, Fwd8Stage& st) {
    const int Sk = p.a.Sk;
    if (tid < kFwdBK) {
        // (as fwd_stage_load.  hipcc waits for this byte at the join, in front of the loads below -- once per tile, wave 0
        // only.  Loading it in every thread, with no branch and no wait, measured 5 % SLOWER: profiles/r10_kv8_prefill.md)
        const int krow = kt * kFwdBK + tid;
        const int kr = krow < Sk ? krow : Sk - 1;
        st.kvalid = kvb ? global_load_u8(kvb + kr) : (uint8_t)1;
    }
    for (int i = 0; i < 2; ++i) {
        const int c = tid + kFwdThreads * i;
        const int row = c >> 4, slot = c & 15;
        const int krow = kt * kFwdBK + row;
        const int kr = krow < Sk ? krow : Sk - 1;
        const uint8_t* kp = kb + (int64_t)kr * p.k_ss + slot * 8;
        st.k[i] = global_load_b64(kp);
        st.v[i] = global_load_b64(vb + (int64_t)kr * p.v_ss + slot * 8);
        st.ks[i] = global_load_f32(ksb + (int64_t)kr * p.ks_ss);
        st.vs[i] = global_load_f32(vsb + (int64_t)kr * p.vs_ss);
        st.ok[i] = global_load_u8(kvb ? kvb + kr : kp);
    }
    issue_fence();
}

// 8 e4m3 bytes times one scale -> 8 bf16 (16 bytes), exactly.  The products are written on register pairs: the packed
// conversion leaves pairs and v_pk_mul_f32 takes them as they are (the library is built without SLP vectorisation, which
// would otherwise have to find them): 4 multiplies per 8 values instead of 8, beside a softmax that is VALU work too.
LWM_DEVICE u32x4 dequant_e4m3x8(u32x2 w, float s) {
    const f32x2 s2 = {s, s};
    const f32x2 a = cvt_e4m3x2_lo(w[0]) * s2, b = cvt_e4m3x2_hi(w[0]) * s2, c = cvt_e4m3x2_lo(w[1]) * s2, d = cvt_e4m3x2_hi(w[1]) * s2;
    return u32x4{pack_bf16x2(a[0], a[1]), pack_bf16x2(b[0], b[1]), pack_bf16x2(c[0], c[1]), pack_bf16x2(d[0], d[1])};
}

// the LDS image of fwd_stage_write: the same 16-byte slots under the same swizzle (cx.stage_w = tile_off(row, slot))
template <int BUF>
LWM_DEVICE void fwd8_stage_write(const FwdCtx& cx, const Fwd8Stage& st, int kt, int Sk, bool has_valid) {
    for (int i = 0; i < 2; ++i) {
        const int krow = kt * kFwdBK + ((cx.tid + kFwdThreads * i) >> 4);
        const bool vis = (krow < Sk) & (!has_valid | (st.ok[i] != 0));
        // a hidden row enters as zero bytes with zero scales, by bit masks: nothing below depends on what it holds
        const uint32_t keep = 0u - (uint32_t)vis;
        const u32x2 kw = {st.k[i][0] & keep, st.k[i][1] & keep}, vw = {st.v[i][0] & keep, st.v[i][1] & keep};
        const float ks = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, st.ks[i]) & keep);
        const float vs = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, st.vs[i]) & keep);
        lds_write_b128(cx.stage_w + BUF * kFwdTileBytes + i * 32 * kRowBytes, dequant_e4m3x8(kw, ks));
        lds_write_b128(cx.stage_w + (2 + BUF) * kFwdTileBytes + i * 32 * kRowBytes, dequant_e4m3x8(vw, vs));
    }
    if (cx.tid < kFwdBK) {
        const bool ok = (kt * kFwdBK + cx.tid < Sk) && st.kvalid != 0;
        lds_write_i32(cx.kseg_w + BUF * kFwdBK * 4, ok ? 0 : kSegInvalid);
    }
}

LWM_KERNEL(kFwdThreads) void attn_prefill_kv8_kernel(Kv8PrefillParams pp) {
    const AttnParams& p = pp.a;
    const lds_t lds = dyn_lds();
    const int tid = thread_idx();
    const int wave = tid >> 6, lane = tid & 63, l31 = lane & 31, hi = lane >> 5;

    // ---- block -> (q tile, head, batch, split): as attn_fwd_body
    const int nqt = (p.Sq + kFwdBQ - 1) / kFwdBQ;
    const int HB = p.H * p.B;
    const int nsplit = p.k_splits > 1 ? p.k_splits : 1;
    const int split = block_idx_x() / (nqt * HB);
    int lin = block_idx_x() - split * (nqt * HB), qt, hb;
    if ((HB & 7) == 0) {
        int xcd = lin & 7, i = lin >> 3;
        hb = xcd + 8 * (i / nqt);
        qt = nqt - 1 - (i % nqt);
    } else {
        hb = lin / nqt;
        qt = nqt - 1 - (lin % nqt);
    }
    const int b = hb / p.H, h = hb % p.H;

    const bf16_t* qb = p.q + (int64_t)b * p.q_sb + (int64_t)h * p.q_sh;
    const uint8_t* kb = pp.k + (int64_t)b * pp.k_sb + (int64_t)h * pp.k_sh;
    const uint8_t* vb = pp.v + (int64_t)b * pp.v_sb + (int64_t)h * pp.v_sh;
    const float* ksb = pp.k_scale + (int64_t)b * pp.ks_sb + h;
    const float* vsb = pp.v_scale + (int64_t)b * pp.vs_sb + h;
    const uint8_t* kvb = p.key_valid ? p.key_valid + (int64_t)b * pp.kv_sb : nullptr;

    // ---- this lane's query row
    const int q_row = qt * kFwdBQ + wave * 32 + l31;
    const bool q_ok = q_row < p.Sq;
    bf16x8 qf[8];
    for (int s = 0; s < 8; ++s) {
        if (q_ok) {
            u32x4 raw = global_load_b128(qb + (int64_t)q_row * p.q_ss + 16 * s + 8 * hi);
            qf[s] = __builtin_bit_cast(bf16x8, raw);
        } else {
            qf[s] = zero_bf16x8();
        }
    }

    FwdCtx cx;
    cx.tid = tid;
    cx.hi = hi;
    cx.ka = frag_rows_addr(lds, 0, l31, hi);
    cx.va = frag_tr_addr(lds + 2 * kFwdTileBytes, lane);
    cx.stage_w = lds + tile_off(tid >> 4, tid & 15);
    cx.kseg_w = lds + 4 * kFwdTileBytes + tid * 4;
    cx.kseg_r = lds + 4 * kFwdTileBytes + 16 * hi;
    cx.q_pos = p.q_start + q_row;
    cx.seg_q = 0;
    cx.has_kmeta = (p.key_valid != nullptr) || (p.Sk % kFwdBK != 0);
    cx.wq_min = p.q_start + qt * kFwdBQ + wave * 32;
    cx.wq_max = cx.wq_min + 31;
    cx.c = p.scale * kLog2e;
    cx.wave_idle = wave_uniform(qt * kFwdBQ + wave * 32 >= p.Sq ? 1 : 0) != 0;
    cx.mask_row = nullptr;

    // ---- kv tile range (causal: skip tiles wholly in the future of this q tile), then this split's piece of it
    const int nkt_all = (p.Sk + kFwdBK - 1) / kFwdBK;
    int nkt = nkt_all;
    const int q_last = (qt * kFwdBQ + kFwdBQ < p.Sq ? qt * kFwdBQ + kFwdBQ : p.Sq) - 1;
    {
        int64_t d = p.q_start + q_last;  // last visible key index (k_start = 0)
        if (d < 0) nkt = 0;
        else {
            int64_t t = d / kFwdBK + 1;
            nkt = t < nkt_all ? (int)t : nkt_all;
        }
    }
    int kt0 = 0;
    if (nsplit > 1) {
        const int per = (nkt_all + nsplit - 1) / nsplit;
        const int s0 = split * per, s1 = s0 + per;
        kt0 = kt0 > s0 ? kt0 : s0;
        nkt = nkt < s1 ? nkt : s1;
    }

    float m_run = -INFINITY;  // running max of raw scores (q.k, unscaled)
    float l_run = 0.0f;       // this half-wave's partial row sum
    f32x16 acc[4];
    for (int i = 0; i < 4; ++i) acc[i] = zero_f32x16();

    const bool has_valid = kvb != nullptr;
    if (kt0 < nkt) {
        Fwd8Stage stg;
        fwd8_stage_load(pp, kb, vb, ksb, vsb, kvb, kt0, tid, stg);
        fwd8_stage_write<0>(cx, stg, kt0, p.Sk, has_valid);
        block_sync();
        // two tiles per trip so the LDS buffer index is a compile-time constant
        for (int kt = kt0; kt < nkt; kt += 2) {
            const bool more1 = kt + 1 < nkt;
            if (more1) fwd8_stage_load(pp, kb, vb, ksb, vsb, kvb, kt + 1, tid, stg);
            fwd_tile<0>(p, cx, qf, kt, m_run, l_run, acc);
            if (more1) fwd8_stage_write<1>(cx, stg, kt + 1, p.Sk, has_valid);
            block_sync();
            if (!more1) break;
            const bool more2 = kt + 2 < nkt;
            if (more2) fwd8_stage_load(pp, kb, vb, ksb, vsb, kvb, kt + 2, tid, stg);
            fwd_tile<1>(p, cx, qf, kt + 1, m_run, l_run, acc);
            if (more2) fwd8_stage_write<0>(cx, stg, kt + 2, p.Sk, has_valid);
            block_sync();
        }
    }

    // ---- epilogue: normalised partials of this split (attn_fwd_body with final_out = 0, carry_in = 0)
    const float l_tot = l_run + xhalf(l_run);
    float inv = 0.0f, lse_b = -INFINITY;
    if (l_tot > 0.0f) {
        inv = 1.0f / l_tot;
        lse_b = m_run * p.scale + logf(l_tot);
    }
    if (q_ok) {
        const int64_t lse_idx = ((int64_t)b * p.H + h) * p.Sq + q_row + (int64_t)split * p.B * p.H * p.Sq;
        const int64_t arow = (((int64_t)b * p.Sq + q_row) * p.H + h) * kHeadDim +
                             (int64_t)split * p.B * p.Sq * p.H * kHeadDim;
        for (int db = 0; db < 4; ++db)
            for (int rq = 0; rq < 4; ++rq) {
                const int d0 = 32 * db + 8 * rq + 4 * hi;
                const float o0 = acc[db][4 * rq + 0] * inv, o1 = acc[db][4 * rq + 1] * inv;
                const float o2 = acc[db][4 * rq + 2] * inv, o3 = acc[db][4 * rq + 3] * inv;
                u32x4 pk = {__builtin_bit_cast(uint32_t, o0), __builtin_bit_cast(uint32_t, o1),
                            __builtin_bit_cast(uint32_t, o2), __builtin_bit_cast(uint32_t, o3)};
                global_store_b128(p.out_acc + arow + d0, pk);
            }
        if (hi == 0) p.lse_acc[lse_idx] = lse_b;
    }
}

}  // namespace lwm
