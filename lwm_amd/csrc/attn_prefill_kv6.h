// attn_prefill_kv6.h -- attention of a BLOCK of queries over the 6-bit (MXFP6 e2m3) KV cache: chunked prefill, a
// follow-up turn, a block appended to a live cache.  Requires wave_ops.h + attn_common.h + attn_fwd.h + attn_decode.h
// (global_load_u8, global_load_b64) + attn_decode_kv6.h (the format, cvt_e2m3x32_bf16, e8m0_to_f32) +
// attn_prefill_kv8.h (KvqPrefillParams).
//
// The kernel is attn_prefill_kv8.h with another staging: the same workgroup -> (q tile, head, batch, split) map, causal
// tile range, split walk, fwd_tile<BUF> and epilogue.  K and V arrive as 24-byte blocks of e2m3 codes with one e8m0
// byte each and are dequantised between the global load and the LDS write; q * s is exactly representable in bf16
// (attn_decode_kv6.h), so the LDS tiles are bit for bit the tiles attn_fwd_body stages from a bf16 copy of the cache.
// No bf16 copy of a cache row ever exists in HBM.
//
// Staging of a 64-key tile: 2 tensors x 64 rows x 4 blocks = 512 items, one per thread: tensor = tid >> 8,
// row = (tid & 255) >> 2, block = tid & 3.  An item is three 8-byte loads, one scale byte and the row's validity byte;
// one v_cvt_scalef32_pk32_bf16_fp6 turns it into 32 bf16, which go to the 16-byte slots 4 block .. 4 block + 3 of the
// row under fwd_stage_write's swizzle.  A key that is masked or lies at or past Sk is staged as a row of zeros and its
// key-meta word is kSegInvalid: its codes and scale byte are cleared with bit masks before the conversion.
#pragma once

namespace lwm {

// k, v: e2m3 blocks (B,Sk,H,96); k_scale, v_scale: e8m0 bytes (B,Sk,H,4)
typedef KvqPrefillParams<uint8_t> Kv6PrefillParams;

// what one thread holds of the next tile between its loads and its LDS writes
struct Fwd6Stage {
    u32x2 w[3];
    uint8_t sc, ok;
    uint8_t kvalid;            // threads < 64: the key-meta byte
};

// Every load of the tile is issued before anything waits (fwd8_stage_load has the reasoning).  `cb` / `sb`: this
// thread's tensor, at its head and block.
LWM_DEVICE void fwd6_stage_load(int Sk, const uint8_t* cb, int64_t c_ss, const uint8_t* sb, int64_t s_ss, const uint8_t* kvb,
                                int kt, int tid, Fwd6Stage& st) {
    if (tid < kFwdBK) {
        const int krow = kt * kFwdBK + tid;
        const int kr = krow < Sk ? krow : Sk - 1;
        st.kvalid = kvb ? global_load_u8(kvb + kr) : (uint8_t)1;
    }
    const int krow = kt * kFwdBK + ((tid & 255) >> 2);
    const int kr = krow < Sk ? krow : Sk - 1;
    const uint8_t* cp = cb + (int64_t)kr * c_ss;
    st.w[0] = global_load_b64(cp);
    st.w[1] = global_load_b64(cp + 8);
    st.w[2] = global_load_b64(cp + 16);
    st.sc = global_load_u8(sb + (int64_t)kr * s_ss);
    st.ok = global_load_u8(kvb ? kvb + kr : cp);
    issue_fence();
}

// `slot_w[j]`: the LDS address of slot 4 block + j of this thread's row in its tensor's tile 0
template <int BUF>
LWM_DEVICE void fwd6_stage_write(const FwdCtx& cx, const lds_t (&slot_w)[4], const Fwd6Stage& st, int kt, int Sk, bool has_valid) {
    const int krow = kt * kFwdBK + ((cx.tid & 255) >> 2);
    const bool vis = (krow < Sk) & (!has_valid | (st.ok != 0));
    // a hidden row enters as zero codes with a zero scale byte, by bit masks: nothing below depends on what it holds
    const uint32_t keep = 0u - (uint32_t)vis;
    const u32x6 w = {st.w[0][0] & keep, st.w[0][1] & keep, st.w[1][0] & keep, st.w[1][1] & keep, st.w[2][0] & keep, st.w[2][1] & keep};
    u32x4 o[4];
    cvt_e2m3x32_bf16(w, e8m0_to_f32((uint32_t)st.sc & keep), o);
    for (int j = 0; j < 4; ++j) lds_write_b128(slot_w[j] + BUF * kFwdTileBytes, o[j]);
    if (cx.tid < kFwdBK) {
        const bool ok = (kt * kFwdBK + cx.tid < Sk) && st.kvalid != 0;
        lds_write_i32(cx.kseg_w + BUF * kFwdBK * 4, ok ? 0 : kSegInvalid);
    }
}

LWM_KERNEL(kFwdThreads) void attn_prefill_kv6_kernel(Kv6PrefillParams pp) {
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
    const uint8_t* kvb = p.key_valid ? p.key_valid + (int64_t)b * pp.kv_sb : nullptr;
    // ---- this thread's staging item: waves 0-3 stage K, waves 4-7 V (a wave-uniform choice)
    const bool st_v = tid >= 256;
    const int st_row = (tid & 255) >> 2, st_blk = tid & 3;
    const uint8_t* cb = (st_v ? pp.v + (int64_t)b * pp.v_sb + (int64_t)h * pp.v_sh : pp.k + (int64_t)b * pp.k_sb + (int64_t)h * pp.k_sh) + st_blk * 24;
    const uint8_t* sb = (st_v ? pp.v_scale + (int64_t)b * pp.vs_sb : pp.k_scale + (int64_t)b * pp.ks_sb) + h * 4 + st_blk;
    const int64_t c_ss = st_v ? pp.v_ss : pp.k_ss, s_ss = st_v ? pp.vs_ss : pp.ks_ss;
    lds_t slot_w[4];
    for (int j = 0; j < 4; ++j) slot_w[j] = lds + (st_v ? 2 * kFwdTileBytes : 0) + tile_off(st_row, 4 * st_blk + j);

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
        Fwd6Stage stg;
        fwd6_stage_load(p.Sk, cb, c_ss, sb, s_ss, kvb, kt0, tid, stg);
        fwd6_stage_write<0>(cx, slot_w, stg, kt0, p.Sk, has_valid);
        block_sync();
        // two tiles per trip so the LDS buffer index is a compile-time constant
        for (int kt = kt0; kt < nkt; kt += 2) {
            const bool more1 = kt + 1 < nkt;
            if (more1) fwd6_stage_load(p.Sk, cb, c_ss, sb, s_ss, kvb, kt + 1, tid, stg);
            fwd_tile<0>(p, cx, qf, kt, m_run, l_run, acc);
            if (more1) fwd6_stage_write<1>(cx, slot_w, stg, kt + 1, p.Sk, has_valid);
            block_sync();
            if (!more1) break;
            const bool more2 = kt + 2 < nkt;
            if (more2) fwd6_stage_load(p.Sk, cb, c_ss, sb, s_ss, kvb, kt + 2, tid, stg);
            fwd_tile<1>(p, cx, qf, kt + 1, m_run, l_run, acc);
            if (more2) fwd6_stage_write<0>(cx, slot_w, stg, kt + 2, p.Sk, has_valid);
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
