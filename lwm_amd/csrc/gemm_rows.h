// gemm_rows.h -- y[r, :] = x[r, :] . W for 1..32 rows on the matrix pipe: the projections of a cached-decode step at
// batch sizes past the GEMV's four rows (gemv.h feeds x through v_readlane into `rows` FMAs per weight element: right
// for 1-4 rows, VALU-bound by 16).  Still weight streaming: W is read once, 2*K*N bytes (K*N as e4m3 bytes), for at
// most 32 tokens.  Requires wave_ops.h + attn_bwd64.h (the host form of the 16x16x32 MFMA) + gemv.h (GemvParams, the K
// partition, gemv_reduce_kernel) + gemv_w8.h (GemvW8Params) + gemv_w6.h (GemvW6Params, GemvW6Format::offset) + attn_decode_kv8.h (cvt_e4m3x2_lo/hi) + attn_decode.h
// (global_load_b64).
//
// Work split: the GEMV's along K -- a workgroup owns kGemvKT = 128 rows of K of one matrix and writes f32 partials
// [K/128][rows][N]; gemv_reduce_kernel (UNCHANGED: the residual add, ss_out and the bf16 / f32 stores are the GEMV's code)
// adds the K/128 partials of an output along its fixed tree.  No atomics: the same input gives the same bits.
//   * workgroup = 4 waves = 128 rows of K x 256 columns; wave w owns columns 64w..64w+63 over ALL 128 rows, so a partial
//     is finished inside one wave's accumulators: no sum across waves, no workgroup barrier (a wave whose columns lie
//     past N leaves at once);
//   * arithmetic: v_mfma_f32_16x16x32_bf16 with A = W^T (16 columns of W x 32 k), B = x^T (32 k x 16 batch rows), so a
//     lane ends up with four consecutive COLUMNS of one batch row: 16-byte stores into the partials.  Rows are padded to
//     16 or 32 inside the tile: rows >= `rows` are fed zeros (their addresses clamped to the last row) and never stored;
//   * W is N-contiguous and the instruction wants 8 consecutive k per lane: the wave's [128 k][64 n] tile goes through
//     its own 16 KiB of LDS (16 loads of 16 bytes per lane in flight, then 16 ds_write_b128) and is read back as
//     transposed fragments (2 x ds_read_b64_tr_b16 each).  LDS image: 128-byte rows; the 32-byte chunk c of row k sits at
//     chunk c ^ rows_swz(k), rows_swz(k) = bit 1 of k | bit 3 of k << 1.  A lane group of the transposed read (32 lanes)
//     takes rows {8g .. 8g+3} x 32 bytes for two g: with the parity of k choosing the half of the 256-byte bank row,
//     the swizzle sends the eight rows to eight different 32-byte bank groups -- conflict-free; a ds_write_b128 lane
//     group (16 lanes) writes two whole rows;
//   * the x fragment (batch row = lane % 16, 8 consecutive k) is one 16-byte global load per lane, no LDS;
//   * RMSNorm on load: gemv.h's gemv_norm expression and gemv_row_rstd tree over ss_in, per row, RESTATED here (as is
//     gemv_tile's lookup) -- the normalised x is bit for bit what lwm_gemv_fused_bf16 feeds its FMAs.  Calling the shared
//     functions gave the same bits and registers but cost the 32-row tile 1-3 % with the norm on (profiles/r16_proj_refactor.md);
//   * 8-bit packs (gemv_w8.h's format): the bytes become bf16 on their way into LDS (an e4m3 value is exact in bf16), the
//     group's power-of-two scale multiplies the finished partial once; everything between is the bf16 kernel's
//     instruction stream;
//   * 6-bit packs (gemv_w6.h's format): a lane takes four 24-byte slots (four rows of its eight columns each, one MX block
//     of the group per slot) and writes each as four rows of the rounded bf16 values e2m3(q) * s -- the tile image is bit for
//     bit the bf16 kernel's on the rounded weights, and everything after the LDS write is its instruction stream.  (A
//     ds_write_b128 lane group now writes half of eight rows, not two whole ones: bank conflicts cost time, not bits.)
// Row independence: output (r, n) is one dot product of the MFMA, fed by x[r] and column n alone; neither `rows`, nor the
// row's slot in the tile, nor its neighbours enter it.
// x must be 16-byte aligned with ldx % 8 == 0 (the GEMV reads x by the element and does not care).
#pragma once

namespace lwm {

constexpr int kRowsThreads = 256;
constexpr int kRowsMax = 32;
constexpr int kRowsWN = 64;                              // columns of W per wave
constexpr int kRowsNT = 4 * kRowsWN;                     // columns of W per workgroup
constexpr int kRowsWaveLds = kGemvKT * kRowsWN * 2;      // a wave's [128 k][64 n] bf16 tile
constexpr int kRowsLdsBytes = 4 * kRowsWaveLds;          // 64 KiB

#ifndef LWM_EMU
// (the host build has its own in attn_bwd64.h)  A: lane l holds A[row = l & 15][k = 8 (l >> 4) + j]; B: lane l holds
// B[k = 8 (l >> 4) + j][col = l & 15]; C/D: lane l, register j holds D[row = 4 (l >> 4) + j][col = l & 15]
LWM_DEVICE f32x4 mfma_16x16x32(bf16x8 a, bf16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
#endif

LWM_DEVICE int rows_swz(int k) { return ((k >> 1) & 1) | (((k >> 3) & 1) << 1); }
// byte offset of the bf16 at (row k, byte column cb) in a wave's tile image
LWM_DEVICE uint32_t rows_off(int k, int cb) { return (uint32_t)(k * (kRowsWN * 2) + ((((cb >> 5) ^ rows_swz(k)) << 5) | (cb & 31))); }

// 8 e4m3 bytes -> 8 bf16 (exact)
LWM_DEVICE u32x4 rows_e4m3x8_to_bf16(u32x2 w) {
    const f32x2 a = cvt_e4m3x2_lo(w[0]), b = cvt_e4m3x2_hi(w[0]), c = cvt_e4m3x2_lo(w[1]), d = cvt_e4m3x2_hi(w[1]);
    return u32x4{pack_bf16x2(a[0], a[1]), pack_bf16x2(b[0], b[1]), pack_bf16x2(c[0], c[1]), pack_bf16x2(d[0], d[1])};
}

// The weight format of the body: bf16 kernels (p.w), or the packs of gemv_w8.h / gemv_w6.h (q / scale hold the matrices)
enum RowsFormat { kRowsBf16, kRowsW8, kRowsW6 };

// One slot of a 6-bit pack (four rows of eight columns, gemv_w6.h) -> the four rows as the rounded bf16 values
// e2m3(q) * s, s = the eight column scales of the slot's MX block (e8m0 bytes): exact, so the tile image is the bf16
// kernel's on the rounded weights.
LWM_DEVICE void rows_e2m3x32_to_bf16(u32x6 w, u32x2 sb, u32x4 (&o)[4]) {
    f32x2 c[16], s[4];
    cvt_e2m3x32_f32(w, c);
    for (int h = 0; h < 4; ++h) {
        const uint32_t two = sb[h >> 1] >> (16 * (h & 1));
        s[h] = f32x2{e8m0_to_f32(two & 255u), e8m0_to_f32((two >> 8) & 255u)};
    }
    for (int j = 0; j < 4; ++j)
        for (int h = 0; h < 4; ++h) {
            const f32x2 v = c[4 * j + h] * s[h];
            o[j][h] = pack_bf16x2(v[0], v[1]);
        }
}

// RB = row blocks of 16 (1: rows <= 16, 2: rows <= 32); F: the weight format; S: its scale type (f32 per 128 rows of K
// for kRowsW8, e8m0 bytes per 32 rows for kRowsW6)
template <int RB, RowsFormat F, class S>
LWM_DEVICE void gemm_rows_body(const GemvParams& p, const uint8_t* const* q, const S* const* scale) {
    constexpr bool W8 = F == kRowsW8, W6 = F == kRowsW6;
    const int tid = thread_idx();
    const int wave = wave_uniform(tid >> 6), lane = tid & 63;
    int mi = 0;                                    // which matrix this workgroup belongs to (uniform)
    for (int i = 1; i < p.nmat; ++i) mi = block_idx_x() >= p.blk0[i] ? i : mi;
    const int N = p.N[mi];
    const int nbn = (N + kRowsNT - 1) / kRowsNT;
    const int bl = block_idx_x() - p.blk0[mi];
    const int ks = bl / nbn, nb = bl % nbn;
    const int n0 = nb * kRowsNT + wave * kRowsWN;
    if (n0 >= N) return;                           // (the whole wave; nothing below waits for another wave)
    const int k0 = ks * kGemvKT;
    const int left = (p.K - k0) >> 5;
    const int nsteps = left < 4 ? left : 4;        // 32-row steps of K that exist in this group (K % 32 == 0)
    const lds_t lds = dyn_lds() + (uint32_t)wave * kRowsWaveLds;

    // ---- W: 16 loads per lane in flight.  Load u: row 8u + (lane >> 3) of the group, columns 8 (lane & 7) .. + 7 of the
    // wave's 64.  Rows past K repeat the last row and columns past N the last eight (the loads stay inside the matrix):
    // such rows belong to steps that are skipped, such columns to outputs that are never stored.
    const int lr = lane >> 3, c8 = (lane & 7) * 8;
    int nc = n0 + c8;
    nc = nc < N ? nc : N - 8;
    u32x4 wv[16];
    u32x2 wq[16];
    u32x6 w6[4];
    u32x2 s6[4];
    if constexpr (W6) {
        // 6-bit packs: four slots per lane.  Slot u: k4 = 8u + (lane >> 3) of the group, n8 = lane & 7 of the wave's 64
        // columns -- rows 32u + 4 (lane >> 3) .. + 3, inside MX block u of the group, whose eight column scales ride along.
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = k0 + 32 * u + 4 * lr;
            const uint8_t* at = q[mi] + GemvW6Format::offset(k < p.K ? k : p.K - 4, nc, N);
            const u32x2 a = global_load_b64(at), b = global_load_b64(at + 8), c = global_load_b64(at + 16);
            w6[u] = u32x6{a[0], a[1], b[0], b[1], c[0], c[1]};
            s6[u] = global_load_b64(scale[mi] + (int64_t)((k < p.K ? k : p.K - 4) >> 5) * N + nc);
        }
    } else {
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int k = k0 + 8 * u + lr;
            const int64_t at = (int64_t)(k < p.K ? k : p.K - 1) * N + nc;
            if constexpr (W8) wq[u] = global_load_b64(q[mi] + at);
            else wv[u] = global_load_b128(p.w[mi] + at);
        }
    }

    // ---- x: fragment (rb, s) = batch row 16 rb + (lane & 15), k = k0 + 32 s + 8 (lane >> 4) .. + 7
    const int i15 = lane & 15, g = lane >> 4;
    float rstd[RB];
    for (int rb = 0; rb < RB; ++rb) rstd[rb] = 0.0f;
    if (p.gamma) {
        // rstd of every row from its partials: gemv_row_rstd's tree (all 64 lanes end with the same sum), one row at a time
        for (int r = 0; r < p.R; ++r) {
            float t = lane < p.ss_n ? p.ss_in[(int64_t)r * p.ss_n + lane] : 0.0f;
            for (int m = 1; m < 64; m <<= 1) t += shfl_xor_f(t, m);
            const float rs = 1.0f / sqrtf(t / (float)p.K + p.eps);
            if (i15 == (r & 15)) {                 // (no register array is indexed by a run-time value)
                if (RB == 1 || r < 16) rstd[0] = rs;
                else rstd[RB - 1] = rs;
            }
        }
    }
    bf16x8 xf[RB][4];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
        const int r = 16 * rb + i15;
        const bool r_ok = r < p.R;
        const bf16_t* xr = p.x + (int64_t)(r_ok ? r : p.R - 1) * p.ldx;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int k = k0 + 32 * s + 8 * g;
            const bool live = r_ok && s < nsteps;
            const int kc = k < p.K ? k : p.K - 8;
            u32x4 raw = global_load_b128(xr + kc);
            if (p.gamma) {
                const u32x4 gw = global_load_b128(p.gamma + kc);
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const float lo = (float)(bf16_t)((float)(bf16_t)(bf16_lo(raw[c]) * rstd[rb]) * bf16_lo(gw[c]));
                    const float hi = (float)(bf16_t)((float)(bf16_t)(bf16_hi(raw[c]) * rstd[rb]) * bf16_hi(gw[c]));
                    raw[c] = pack_bf16x2(lo, hi);
                }
            }
            if (!live) raw = u32x4{0, 0, 0, 0};
            xf[rb][s] = __builtin_bit_cast(bf16x8, raw);
        }
    }

    // ---- W into the wave's tile image
    if constexpr (W6) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            u32x4 o[4];
            rows_e2m3x32_to_bf16(w6[u], s6[u], o);
#pragma unroll
            for (int j = 0; j < 4; ++j) lds_write_b128(lds + rows_off(32 * u + 4 * lr + j, c8 * 2), o[j]);
        }
    } else {
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            if constexpr (W8) wv[u] = rows_e4m3x8_to_bf16(wq[u]);
            lds_write_b128(lds + rows_off(8 * u + lr, c8 * 2), wv[u]);
        }
    }
    wave_lds_fence();

    // ---- products.  Fragment (s, nbk) of W^T: lane (g, i15) gets W[32 s + 8 g + 0..7][16 nbk + i15] -- the first read
    // takes rows 8g .. 8g+3 (lanes 4j..4j+3 of the group point at four consecutive columns 4 (i15 & 3) .. of row j), the
    // second rows 8g+4 .. 8g+7.  (EXEC is all ones here: the branch on nsteps is uniform.)
    f32x4 acc[RB][4];
    for (int rb = 0; rb < RB; ++rb)
        for (int nbk = 0; nbk < 4; ++nbk) acc[rb][nbk] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        if (s < nsteps) {
#pragma unroll
            for (int nbk = 0; nbk < 4; ++nbk) {
                const int k = 32 * s + 8 * g + (i15 >> 2), cb = 32 * nbk + 8 * (i15 & 3);
                const bf16x4 lo = lds_read_tr16(lds + rows_off(k, cb)), up = lds_read_tr16(lds + rows_off(k + 4, cb));
                bf16x8 a;
                a[0] = lo[0]; a[1] = lo[1]; a[2] = lo[2]; a[3] = lo[3];
                a[4] = up[0]; a[5] = up[1]; a[6] = up[2]; a[7] = up[3];
#pragma unroll
                for (int rb = 0; rb < RB; ++rb) acc[rb][nbk] = mfma_16x16x32(a, xf[rb][s], acc[rb][nbk]);
            }
        }
    }

    // ---- partials: lane (g, i15) holds columns n0 + 16 nbk + 4 g + 0..3 of batch row 16 rb + i15
#pragma unroll
    for (int nbk = 0; nbk < 4; ++nbk) {
        const int n = n0 + 16 * nbk + 4 * g;
        if (n < N) {
            f32x4 sc = {1.0f, 1.0f, 1.0f, 1.0f};
            if constexpr (W8) sc = global_load_f32x4(scale[mi] + (int64_t)ks * N + n);     // the group's scale of the lane's columns
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) {
                const int r = 16 * rb + i15;
                if (r < p.R) {
                    float* dst = p.part + p.part_off[mi] + ((int64_t)ks * p.R + r) * N + n;
                    global_store_f32x4(dst, W8 ? acc[rb][nbk] * sc : acc[rb][nbk]);      // once per partial: s is a power of two
                }
            }
        }
    }
}

// dynamic LDS: kRowsLdsBytes
LWM_KERNEL(kRowsThreads) void gemm_rows_bf16_kernel(GemvParams p) {
    if (p.R <= 16) gemm_rows_body<1, kRowsBf16, float>(p, nullptr, nullptr);       // (uniform)
    else gemm_rows_body<2, kRowsBf16, float>(p, nullptr, nullptr);
}

LWM_KERNEL(kRowsThreads) void gemm_rows_w8_kernel(GemvW8Params pp) {
    if (pp.g.R <= 16) gemm_rows_body<1, kRowsW8>(pp.g, pp.q, pp.scale);
    else gemm_rows_body<2, kRowsW8>(pp.g, pp.q, pp.scale);
}

LWM_KERNEL(kRowsThreads) void gemm_rows_w6_kernel(GemvW6Params pp) {
    if (pp.g.R <= 16) gemm_rows_body<1, kRowsW6>(pp.g, pp.q, pp.scale);
    else gemm_rows_body<2, kRowsW6>(pp.g, pp.q, pp.scale);
}

}  // namespace lwm
