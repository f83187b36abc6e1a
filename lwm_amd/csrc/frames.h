// frames.h -- the frame preprocessor in front of the VQGAN tokeniser: uint8 RGB frames [T,H,W,3] ->
// f32 [T,size,size,3] in [-1,1], bit for bit what lwm/vision_chat.py:59-74 gets from Pillow (antialiased bicubic
// resize of the short side to `size`, centre crop, u/127.5 - 1).  Requires wave_ops.h.
//
// Pillow's 8-bit resample is integer arithmetic on 22-bit fixed-point coefficients: horizontal pass, uint8
// intermediate image, vertical pass.  The host builds the coefficient tables in f64 (lwm_amd/frames.py) and the
// 256-entry f32 table of the final scale; nothing here is floating-point arithmetic.  The contract of the tables is
// in include/lwm_hip.h (LwmFramesArgs); lwm_frames_preprocess_u8 validates them before either kernel is launched.
//
//   frames_hpass: the `size` cropped columns of the rows that the vertical pass reads -> inter [T,nrows,istride] u8.
//     One workgroup = one strip of kFrCols output columns x kFrRowsPerWg rows.  The strip's coefficients go to LDS
//     once; then, kFrRows rows at a time, the input span of the strip is staged in LDS with aligned dword loads (the
//     input is packed 3-byte pixels: no row starts aligned) and every thread picks its taps' bytes out of LDS dwords.
//   frames_vpass: inter -> out.  One thread = 4 consecutive bytes of an output row: one aligned dword of the
//     intermediate per tap feeds four accumulators.
// A pass that Pillow skips (output length == input length) copies its window.
// The accumulators are uint32 (sums modulo 2^32, then an arithmetic shift): exact for |acc| < 2^31, which Pillow's
// tables keep (255 * sum |k| + 2^21 < 2^31: tests/test_frames_ref.py), and defined for any table a caller passes.
#pragma once

namespace lwm {

constexpr int kFrThreads = 256;
constexpr int kFrCols = 64;        // output columns per workgroup = one wave
constexpr int kFrRows = 4;         // rows staged at a time = waves per workgroup
constexpr int kFrRowsPerWg = 16;   // rows per workgroup (the strip's coefficients are staged once for them)

struct FramesParams {
    const uint8_t* frames;
    float* out;
    uint8_t* inter;        // [T, nrows, istride]
    const int32_t* hb;     // device copies of the tables (null: pass skipped)
    const int32_t* hk;
    const int32_t* vb;
    const int32_t* vk;
    const float* scale;
    int64_t total;         // bytes of `frames`
    int32_t T, H, W, size, hks, vks, left, top;
    int32_t row0, nrows;   // input rows [row0, row0 + nrows) feed the vertical pass
    int32_t istride;       // bytes per intermediate row: size * 3 rounded up to 4
    int32_t span_dw;       // LDS dwords per staged row
    int32_t nstrips, nrblocks;
};

// LDS bytes of frames_hpass: bounds, coefficients (row stride odd: conflict-free across columns), staged rows
LWM_HD int frames_kstride(int hks) { return hks ? (hks | 1) : 0; }
LWM_HD size_t frames_hpass_lds(int hks, int span_dw) {
    return (size_t)kFrCols * 8 + (size_t)kFrCols * frames_kstride(hks) * 4 + (size_t)kFrRows * span_dw * 4;
}

// the three bytes at byte offset b of an LDS row, in bits 0-23
LWM_DEVICE uint32_t frames_px(lds_t row, int b) {
    const lds_t a = row + (lds_t)(b & ~3);
    const uint64_t lo = (uint32_t)lds_read_i32(a), hi = (uint32_t)lds_read_i32(a + 4);
    return (uint32_t)(((hi << 32) | lo) >> (8 * (b & 3)));
}

LWM_DEVICE uint32_t frames_clamp(uint32_t acc) {
    const int32_t v = (int32_t)acc >> 22;
    return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

LWM_KERNEL(256) void frames_hpass_kernel(FramesParams p) {
    const int tid = thread_idx();
    int bid = block_idx_x();
    const int strip = bid % p.nstrips;
    bid /= p.nstrips;
    const int rb = bid % p.nrblocks;
    const int t = bid / p.nrblocks;
    const int xs0 = strip * kFrCols;
    const int ncol = p.size - xs0 < kFrCols ? p.size - xs0 : kFrCols;
    const int kstride = frames_kstride(p.hks);
    const lds_t l_b = dyn_lds(), l_k = l_b + kFrCols * 8, l_rows = l_k + (lds_t)(kFrCols * kstride * 4);

    if (p.hks) {
        for (int i = tid; i < ncol * 2; i += kFrThreads) lds_write_i32(l_b + 4 * i, p.hb[xs0 * 2 + i]);
        for (int i = tid; i < ncol * p.hks; i += kFrThreads)
            lds_write_i32(l_k + 4 * ((i / p.hks) * kstride + i % p.hks), p.hk[(int64_t)xs0 * p.hks + i]);
    }
    block_sync();
    // input columns [lo, hi) of the strip (every thread: LDS broadcasts)
    int lo, hi;
    if (p.hks) {
        lo = 0x7fffffff;
        hi = 0;
        for (int i = 0; i < ncol; ++i) {
            const int first = lds_read_i32(l_b + 8 * i), taps = lds_read_i32(l_b + 8 * i + 4);
            lo = first < lo ? first : lo;
            hi = first + taps > hi ? first + taps : hi;
        }
    } else {
        lo = p.left + xs0;
        hi = lo + ncol;
    }
    const int nbytes = (hi - lo) * 3;
    const int col = tid & (kFrCols - 1), rsub = tid / kFrCols;
    int first = 0, taps = 0;
    if (p.hks && col < ncol) {
        first = lds_read_i32(l_b + 8 * col);
        taps = lds_read_i32(l_b + 8 * col + 4);
    }
    const int r_end = (rb + 1) * kFrRowsPerWg < p.nrows ? (rb + 1) * kFrRowsPerWg : p.nrows;
    for (int r0 = rb * kFrRowsPerWg; r0 < r_end; r0 += kFrRows) {
        for (int j = 0; j < kFrRows && r0 + j < r_end; ++j) {
            // bytes [goff, goff + nbytes) of `frames`, fetched as the aligned dwords that cover them
            const int64_t goff = (((int64_t)t * p.H + p.row0 + r0 + j) * p.W + lo) * 3;
            const int mis = (int)(((uintptr_t)p.frames + (uintptr_t)goff) & 3);
            const int nd = (mis + nbytes + 3) >> 2;
            for (int d = tid; d < nd; d += kFrThreads) {
                const int64_t off = goff - mis + 4 * (int64_t)d;
                uint32_t v = 0;
                if (off >= 0 && off + 4 <= p.total) {
                    v = *(const uint32_t*)(p.frames + off);
                } else {  // the first / last dword of the whole buffer: only the bytes inside it
                    for (int b = 0; b < 4; ++b)
                        if (off + b >= 0 && off + b < p.total) v |= (uint32_t)p.frames[off + b] << (8 * b);
                }
                lds_write_i32(l_rows + 4 * (lds_t)(j * p.span_dw + d), (int32_t)v);
            }
        }
        block_sync();
        const int r = r0 + rsub;
        if (r < r_end && col < ncol) {
            const int64_t goff = (((int64_t)t * p.H + p.row0 + r) * p.W + lo) * 3;
            const int mis = (int)(((uintptr_t)p.frames + (uintptr_t)goff) & 3);
            const lds_t row = l_rows + 4 * (lds_t)(rsub * p.span_dw);
            uint32_t u0, u1, u2;
            if (p.hks) {
                uint32_t a0 = 1u << 21, a1 = 1u << 21, a2 = 1u << 21;
                const lds_t kc = l_k + 4 * (lds_t)(col * kstride);
                int b = mis + (first - lo) * 3;
                for (int x = 0; x < taps; ++x, b += 3) {
                    const uint32_t k = (uint32_t)lds_read_i32(kc + 4 * x);
                    const uint32_t px = frames_px(row, b);
                    a0 += (px & 255u) * k;
                    a1 += ((px >> 8) & 255u) * k;
                    a2 += ((px >> 16) & 255u) * k;
                }
                u0 = frames_clamp(a0);
                u1 = frames_clamp(a1);
                u2 = frames_clamp(a2);
            } else {
                const uint32_t px = frames_px(row, mis + col * 3);
                u0 = px & 255u;
                u1 = (px >> 8) & 255u;
                u2 = (px >> 16) & 255u;
            }
            uint8_t* o = p.inter + ((int64_t)t * p.nrows + r) * p.istride + (xs0 + col) * 3;
            o[0] = (uint8_t)u0;
            o[1] = (uint8_t)u1;
            o[2] = (uint8_t)u2;
        }
        block_sync();
    }
}

LWM_KERNEL(256) void frames_vpass_kernel(FramesParams p) {
    const int quads = p.istride >> 2;
    const int per_frame = (p.size * quads + kFrThreads - 1) / kFrThreads;
    const int t = block_idx_x() / per_frame;
    const int i = (block_idx_x() % per_frame) * kFrThreads + thread_idx();
    if (i >= p.size * quads) return;
    const int yy = i / quads, q = i % quads;
    const uint8_t* src = p.inter + (int64_t)t * p.nrows * p.istride + q * 4;
    uint32_t u[4];
    if (p.vks) {
        const int first = p.vb[yy * 2] - p.row0, taps = p.vb[yy * 2 + 1];
        const int32_t* k = p.vk + (int64_t)yy * p.vks;
        uint32_t a[4] = {1u << 21, 1u << 21, 1u << 21, 1u << 21};
        for (int x = 0; x < taps; ++x) {
            const uint32_t v = *(const uint32_t*)(src + (int64_t)(first + x) * p.istride);
            const uint32_t kx = (uint32_t)k[x];
            for (int j = 0; j < 4; ++j) a[j] += ((v >> (8 * j)) & 255u) * kx;
        }
        for (int j = 0; j < 4; ++j) u[j] = frames_clamp(a[j]);
    } else {
        const uint32_t v = *(const uint32_t*)(src + (int64_t)(p.top - p.row0 + yy) * p.istride);
        for (int j = 0; j < 4; ++j) u[j] = (v >> (8 * j)) & 255u;
    }
    const int row_elems = p.size * 3;
    float* o = p.out + ((int64_t)t * p.size + yy) * row_elems + q * 4;
    if (q * 4 + 4 <= row_elems && ((uintptr_t)o & 15) == 0) {
        f32x4 f;
        for (int j = 0; j < 4; ++j) f[j] = p.scale[u[j]];
        global_store_f32x4(o, f);
    } else {
        for (int j = 0; j < 4 && q * 4 + j < row_elems; ++j) o[j] = p.scale[u[j]];
    }
}

}  // namespace lwm
