// dropout.h -- residual and embedding dropout of the training path (FlaxLLaMAAttention.resid_dropout, lwm/llama.py:423,
// :618; FlaxLLaMAMLP.dropout, :656-660; the embedding dropout, :998, :1017): y = res + dropout(x) in one pass over
// contiguous (B, S, C) tensors, bf16 or f32, and the backward dx = dropout'(g) as the same pass without `res`.
//
// The keep mask is a FUNCTION of (key0, key1, site, b, s_offset + s, c) -- a counter-based Philox4x32-10 draw, no state and
// no stored mask: the backward, a recompute of the forward and a chunk of rows [s0, s1) launched with s_offset = s0 all
// regenerate the bits the whole forward saw.  The rule, with its arithmetic, is stated in include/lwm_hip.h
// ("dropout"); tests/_dropout_ref.py restates it in numpy.
//
// One Philox call covers 8 consecutive channels -- one 16-byte bf16 vector, two 16-byte f32 vectors -- 16 bits each.
// A block takes tiles of 256 such vectors, grid-stride; the tile's first (b, s, c / 8) comes from one uniform division
// per tile, a lane's own from two compares (C >= 2048: a tile crosses at most one row end) or two 32-bit divisions.  No LDS, no atomics.  y may alias x or res: a lane reads its 8 elements
// of both before it writes them.
//
// Expects wave_ops.h (the product's or the host emulation's) to be included first.
#pragma once
#include "philox.h"

namespace lwm {

struct DropoutParams {
    const void* x;
    const void* res;         // null: y = dropout(x)
    void* y;
    int64_t nvec;            // B * S * C / 8
    uint32_t S, Cv;          // Cv = C / 8
    uint32_t s_offset, site, key0, key1;
    uint32_t thr16;          // drop iff the element's 16 bits < thr16
    float inv;               // 1 / (1 - thr16 / 65536), rounded to f32 on the host
};

// The two roundings of the contract, each an instruction of its own: never one fused multiply-add.
#ifdef LWM_EMU
LWM_DEVICE float dropout_mul(float a, float b) { return a * b; }      // (the emulation is built with -ffp-contract=off)
LWM_DEVICE float dropout_add(float a, float b) { return a + b; }
#else
LWM_DEVICE float dropout_mul(float a, float b) { return __fmul_rn(a, b); }
LWM_DEVICE float dropout_add(float a, float b) { return __fadd_rn(a, b); }
#endif

// element j (0..7) of the vector: keep ? x * inv : +0
LWM_DEVICE float dropout_elem(float x, const uint32_t r[4], int j, uint32_t thr16, float inv) {
    const uint32_t h = (j & 1) ? (r[j >> 1] >> 16) : (r[j >> 1] & 0xffffu);
    return h < thr16 ? 0.0f : dropout_mul(x, inv);
}

template <bool kF32, bool kRes>
LWM_KERNEL(256) void dropout_kernel(DropoutParams p) {
    const int64_t ntiles = (p.nvec + 255) >> 8;
    const int tid = thread_idx();
    for (int64_t t = block_idx_x(); t < ntiles; t += grid_dim_x()) {
        // the tile's first vector: uniform, one division per tile
        const int64_t v0 = t << 8;
        const int64_t row0 = v0 / p.Cv;
        const uint32_t cv0 = (uint32_t)(v0 - row0 * p.Cv);
        const int64_t b0 = row0 / p.S;
        const uint32_t s0 = (uint32_t)(row0 - b0 * p.S);
        const int64_t i = v0 + tid;
        if (i >= p.nvec) continue;
        // the loads first: their latency passes under the index arithmetic and the Philox rounds
        constexpr int kVecs = kF32 ? 2 : 1;                 // 16-byte vectors of 8 elements
        const char* xp = (const char*)p.x + i * (16 * kVecs);
        const char* rp = (const char*)p.res + i * (16 * kVecs);
        u32x4 xv[kVecs], rv[kVecs], o[kVecs];
#pragma unroll
        for (int k = 0; k < kVecs; ++k) {
            xv[k] = global_load_b128(xp + 16 * k);
            if (kRes) rv[k] = global_load_b128(rp + 16 * k);
        }
        // this lane's (b, s, c / 8): cv0 + tid < Cv + 256 and s0 + q < S + 256, both far inside 32 bits
        uint32_t cv = cv0 + (uint32_t)tid, s, qb;
        if (p.Cv >= 256u) {                                 // (uniform) a tile crosses at most one row end: compares
            const bool q = cv >= p.Cv;
            cv -= q ? p.Cv : 0u;
            s = s0 + (q ? 1u : 0u);
            qb = s >= p.S ? 1u : 0u;
            s -= qb ? p.S : 0u;
        } else {
            const uint32_t q = cv / p.Cv;
            cv -= q * p.Cv;
            s = s0 + q;
            qb = s / p.S;
            s -= qb * p.S;
        }
        uint32_t r[4] = {cv, p.s_offset + s, (uint32_t)b0 + qb, p.site};
        philox4x32_10(r, p.key0, p.key1);
        if (kF32) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const uint32_t xw = xv[j >> 2][j & 3], rw = kRes ? rv[j >> 2][j & 3] : 0u;      // (scalars: bit_cast takes no vector element)
                const float d = dropout_elem(__builtin_bit_cast(float, xw), r, j, p.thr16, p.inv);
                const float yf = kRes ? dropout_add(__builtin_bit_cast(float, rw), d) : d;
                o[j >> 2][j & 3] = __builtin_bit_cast(uint32_t, yf);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float d0 = dropout_elem(__builtin_bit_cast(float, xv[0][j] << 16), r, 2 * j, p.thr16, p.inv);
                float d1 = dropout_elem(__builtin_bit_cast(float, xv[0][j] & 0xffff0000u), r, 2 * j + 1, p.thr16, p.inv);
                if (kRes) {
                    d0 = dropout_add(__builtin_bit_cast(float, rv[0][j] << 16), d0);
                    d1 = dropout_add(__builtin_bit_cast(float, rv[0][j] & 0xffff0000u), d1);
                }
                o[0][j] = pack_bf16x2(d0, d1);      // the one rounding to bf16, to nearest even
            }
        }
        char* yp = (char*)p.y + i * (16 * kVecs);
#pragma unroll
        for (int k = 0; k < kVecs; ++k) global_store_b128(yp + 16 * k, o[k]);
    }
}

}  // namespace lwm
