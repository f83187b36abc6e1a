// vqgan_conv_bf16.h -- the opt-in second precision of the VQGAN convolutions: the geometry and epilogue of vqgan_conv.h
// (3x3 SAME, 1x1, Downsample, Upsample folded in, + bias + residual, clip) on the bf16 matrix instruction
// (v_mfma_f32_32x32x16_bf16, 16 times the rate of the exact-f32 one).  Requires wave_ops.h + vqgan_conv.h (ConvParams,
// kConvKC, IntTag, the ranged loads, global_load_f32_at / global_store_f32_at).
//
// Arithmetic contract (NOT the bit-exact one of vqgan_conv.h):
//   out = (sum over taps and input channels of bf16(x) * bf16(w), products exact, accumulated in f32) + bias [+ residual]
//   * activations stay f32 in memory, in and out; they are rounded to bf16 -- round to nearest even, pack_bf16x2 --
//     between the global load and the LDS write, the only place where the operand exists as bf16;
//   * the kernel arrives packed as bf16 (below), rounded once when the weights are loaded;
//   * the order of the sum is a fixed function of the launch geometry: taps in (kh, kw) order, 32 input channels per
//     step, two MFMAs per step on ONE f32 accumulator.  It depends neither on timing nor on where in the batch an image
//     lies, so the same launch gives the same bits and an image's bits do not depend on its neighbours;
//   * out-of-image taps contribute exact zeros whatever lies next to the tensor: they are never read.
// Normal numbers only: what the conversion and the matrix pipe do with subnormal or non-finite operands is outside the
// contract.
//
// The packed kernel, [tap][Cin / 8][Cout][8] bf16 (tap = kh * KW + kw): element (tap, ci, co) at
// ((tap * Cin / 8 + ci / 8) * Cout + co) * 8 + ci % 8.  The B operand of the MFMA is 8 consecutive input channels of one
// output channel per lane: one 16-byte load, 512 contiguous bytes per half-wave, straight from L1/L2 into registers
// (every workgroup walks the same pack); HWIO has the OUTPUT channel contiguous.  Cin % 32 == 0 and Cout % 32 == 0.
//
// Workgroup = 256 threads = WM x WN waves, wave tile (32 MB) pixels x (32 NB) channels.  K is walked in steps of 32 input
// channels of one tap.  A tile [BM pixels][32 cin] bf16 in LDS, two buffers, rows of 64 + 16 bytes: the ds_read_b128 of a
// fragment (16 pixels per lane group, one k-octet each) then covers all 16 slots of a bank row -- 20 p mod 64 is
// 4 (5 p mod 16), a bijection of p mod 16.  Staging: a thread loads 8 channels of a pixel (two ranged 16-byte loads: an
// out-of-image tap is an offset past the range and comes back as zeros), converts and writes 16 bytes.  The loads of
// step it + 2 are issued when step `it` begins and written when step it + 1 begins: a whole step of MFMAs hides them.
#pragma once

namespace lwm {

template <int WM, int WN, int MB, int NB>
struct Conv16Cfg {
    static constexpr int NT = 64 * WM * WN;
    static constexpr int BM = 32 * MB * WM;
    static constexpr int BN = 32 * NB * WN;
    static constexpr int A_ROW = kConvKC * 2 + 16;   // LDS stride of a staged pixel: its 32 channels + one unused 16-byte slot
    static constexpr int A_BYTES = BM * A_ROW;
    static constexpr int LDS_BYTES = 2 * A_BYTES;
    static constexpr int APX = NT / 4;               // pixels staged per pass (4 lanes x 32 B of f32 per pixel)
    static constexpr int AP = BM / APX;              // A staging passes
    static_assert(NT == 256 && BM % APX == 0 && AP >= 1, "A staging shape");
};

template <int WM, int WN, int MB, int NB>
LWM_DEVICE void conv16_body(const ConvParams& p) {
    using Cfg = Conv16Cfg<WM, WN, MB, NB>;
    constexpr int BM = Cfg::BM, BN = Cfg::BN, AP = Cfg::AP;
    const lds_t lds = dyn_lds();
    const int tid = thread_idx();
    const int wave = wave_uniform(tid >> 6), lane = tid & 63, l31 = lane & 31, hi = lane >> 5;
    const int wm = wave / WN, wn = wave % WN;
    const int ntn = (p.Cout + BN - 1) / BN;
    const int64_t m0 = (int64_t)(block_idx_x() / ntn) * BM;
    const int n0 = (block_idx_x() % ntn) * BN;
    const int nch = p.Cin / kConvKC;
    const int nit = p.KH * p.KW * nch;

    // ---- A staging roles (fixed for the whole launch): pixel ps * APX + tid / 4, channels 8 (tid % 4) .. + 7 of the step
    const int a_slot = tid & 3;
    int a_oy[AP], a_ox[AP];
    int64_t a_base[AP];  // element offset of (b, 0, 0, 0) in x; -1 = pixel past M
    for (int ps = 0; ps < AP; ++ps) {
        const int64_t m = m0 + ps * Cfg::APX + (tid >> 2);
        if (m < p.M) {
            const int64_t t = m / p.Wo;
            a_ox[ps] = (int)(m % p.Wo) * p.stride - p.pad;
            a_oy[ps] = (int)(t % p.Ho) * p.stride - p.pad;
            a_base[ps] = (t / p.Ho) * (int64_t)p.Hin * p.Win * p.Cin;
        } else {
            a_ox[ps] = 0;
            a_oy[ps] = 0;
            a_base[ps] = -1;
        }
    }
    const int Hv = p.Hin << p.up_shift, Wv = p.Win << p.up_shift;
    // Offsets are 32-bit and relative to the image of the tile's first pixel (a tile reaches a few images at most, and
    // the launch guarantees that span < 0xE0000000 bytes); kOob + any step's channel offset stays past the range.
    constexpr uint32_t kOob = 0xF0000000u;
    const int64_t img_el = (int64_t)p.Hin * p.Win * p.Cin;
    const int64_t el0 = m0 / ((int64_t)p.Ho * p.Wo) * img_el;
    const int64_t x_left = ((int64_t)p.B * img_el - el0) * 4;
    const ranged_t x_range = ranged_make(p.x + el0, (uint32_t)(x_left < 0xE0000000LL ? x_left : 0xE0000000LL));
    uint32_t a_tapb[AP];
    int ld_kh = 0, ld_kw = 0, ld_ch = 0;     // the (tap, step) the next stage_load fetches: a running counter
    auto stage_tap = [&]() {
#pragma unroll
        for (int ps = 0; ps < AP; ++ps) {
            const int vy = a_oy[ps] + ld_kh, vx = a_ox[ps] + ld_kw;
            const bool ok = a_base[ps] >= 0 && vy >= 0 && vy < Hv && vx >= 0 && vx < Wv;
            const int at = ((vy >> p.up_shift) * p.Win + (vx >> p.up_shift)) * p.Cin;
            a_tapb[ps] = ok ? (uint32_t)(a_base[ps] - el0 + at) * 4u + (uint32_t)a_slot * 32u : kOob;
        }
    };
    stage_tap();
    f32x4 sa[AP][2];
    // (unconditional: past the last step it fetches a tap that does not exist -- in range or zeros, written nowhere.
    //  A load behind a runtime branch makes hipcc wait for every load in flight at the join: vqgan_conv.h)
    auto stage_load = [&]() {
#pragma unroll
        for (int ps = 0; ps < AP; ++ps) {
            const uint32_t voff = a_tapb[ps] + (uint32_t)ld_ch * (kConvKC * 4u);
            sa[ps][0] = ranged_load_f32x4(x_range, voff);
            sa[ps][1] = ranged_load_f32x4(x_range, voff + 16u);
        }
        if (++ld_ch == nch) {
            ld_ch = 0;
            if (++ld_kw == p.KW) {
                ld_kw = 0;
                ++ld_kh;
            }
            stage_tap();
        }
    };
    const lds_t a_w = lds + (uint32_t)(tid >> 2) * Cfg::A_ROW + (uint32_t)a_slot * 16u;
    auto stage_write = [&](uint32_t bo) {      // f32 -> bf16, round to nearest even, HERE
#pragma unroll
        for (int ps = 0; ps < AP; ++ps) {
            const f32x4 lo = sa[ps][0], up = sa[ps][1];
            lds_write_b128(a_w + bo + (uint32_t)ps * Cfg::APX * Cfg::A_ROW,
                           u32x4{pack_bf16x2(lo[0], lo[1]), pack_bf16x2(lo[2], lo[3]), pack_bf16x2(up[0], up[1]), pack_bf16x2(up[2], up[3])});
        }
    };

    // ---- B operands: k-octet (4 it + 2 s + hi) of the pack, column n0 + (wn NB + j) 32 + l31.  A column block past Cout
    // (a ragged last tile; whole blocks: Cout % 32 == 0) reads the tile's first block instead and is never stored.
    const ranged_t w_range = ranged_make(p.w, (uint32_t)((int64_t)nit * kConvKC * p.Cout * 2));
    uint32_t b_voff[NB];
    for (int j = 0; j < NB; ++j) {
        const int cb = n0 + (wn * NB + j) * 32;
        b_voff[j] = (uint32_t)(hi * p.Cout + (cb < p.Cout ? cb : n0) + l31) * 16u;
    }
    const uint32_t b_step = (uint32_t)p.Cout * 32u;      // bytes of two k-octets: one MFMA's worth of every column
    bf16x8 bfr[2][2][NB];
    auto load_b = [&](int it, auto set_tag) {             // (past the last step: past the range, zeros)
        constexpr int SET = decltype(set_tag)::value;
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int j = 0; j < NB; ++j)
                bfr[SET][s][j] = __builtin_bit_cast(bf16x8, ranged_load_f32x4(w_range, b_voff[j] + (uint32_t)(2 * it + s) * b_step));
    };

    f32x16 acc[MB][NB];
    for (int i = 0; i < MB; ++i)
        for (int j = 0; j < NB; ++j) acc[i][j] = zero_f32x16();
    uint32_t a_r[MB];
    for (int i = 0; i < MB; ++i) a_r[i] = lds + (uint32_t)((wm * MB + i) * 32 + l31) * Cfg::A_ROW + (uint32_t)hi * 16u;

    stage_load();
    load_b(0, IntTag<0>{});
    stage_write(0);
    stage_load();
    block_sync_lds();
    // step `it` (SET = it % 2: its LDS buffer and B register set): step it + 1 goes to the other buffer -- nobody reads it
    // since the barrier that ended step it - 1 -- and the loads of step it + 2 and of the next B set go out, then the
    // MFMAs; the barrier at the end publishes buffer SET ^ 1 and retires the reads of buffer SET.
    auto step = [&](int it, auto set_tag) {
        constexpr int SET = decltype(set_tag)::value;
        if (it + 1 < nit) stage_write((uint32_t)(SET ^ 1) * Cfg::A_BYTES);
        stage_load();
        load_b(it + 1, IntTag<(SET ^ 1)>{});
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            bf16x8 af[MB];
#pragma unroll
            for (int i = 0; i < MB; ++i) af[i] = lds_read_b128(a_r[i] + (uint32_t)SET * Cfg::A_BYTES + (uint32_t)s * 32u);
#pragma unroll
            for (int i = 0; i < MB; ++i)
#pragma unroll
                for (int j = 0; j < NB; ++j) acc[i][j] = mfma_32x32x16(af[i], bfr[SET][s][j], acc[i][j]);
        }
        block_sync_lds();
    };
    int it = 0;
    for (; it + 1 < nit; it += 2) {
        step(it, IntTag<0>{});
        step(it + 1, IntTag<1>{});
    }
    if (it < nit) step(it, IntTag<0>{});

    // ---- epilogue, as vqgan_conv.h: + bias [+ residual] [clip], one float per (pixel, channel)
    const int64_t tile_base = m0 * p.Cout;
    float* const yb = p.y + tile_base;
    const float* const rb = p.res ? p.res + tile_base : p.y;
    const int64_t left = p.M - m0;                    // >= 1 rows of this tile exist
    const int rows = left < BM ? (int)left : BM;
    if (rows == BM && n0 + BN <= p.Cout) {
        // a whole tile: every residual read of the wave in flight together; an address is the lane's part in a VGPR plus
        // the (i, r) part, wave-uniform, in an SGPR
        const uint32_t voff = (uint32_t)(4 * hi * p.Cout + n0 + wn * NB * 32 + l31) * 4u;
        auto soff = [&](int i, int r) -> uint32_t {
            return (uint32_t)((wm * MB + i) * 32 + (r & 3) + 8 * (r >> 2)) * (uint32_t)p.Cout * 4u;
        };
        float rv[MB][NB][16];
        if (p.res) {
#pragma unroll
            for (int i = 0; i < MB; ++i)
#pragma unroll
                for (int j = 0; j < NB; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) rv[i][j][r] = global_load_f32_at(rb, voff + (uint32_t)j * 128u, soff(i, r));
        }
        float bv[NB];
#pragma unroll
        for (int j = 0; j < NB; ++j) bv[j] = p.bias ? p.bias[n0 + (wn * NB + j) * 32 + l31] : 0.0f;
#pragma unroll
        for (int i = 0; i < MB; ++i)
#pragma unroll
            for (int j = 0; j < NB; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    float v = acc[i][j][r];
                    if (p.bias) v = v + bv[j];
                    if (p.res) v = v + rv[i][j][r];
                    if (p.clip) v = v < -1.0f ? -1.0f : (v > 1.0f ? 1.0f : v);
                    global_store_f32_at(yb, voff + (uint32_t)j * 128u, soff(i, r), v);
                }
        return;
    }
    // a ragged tile (rows past M, column blocks past Cout): rows past M are clamped for the residual read and skipped for
    // the store
#pragma unroll
    for (int i = 0; i < MB; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const int co = n0 + (wn * NB + j) * 32 + l31;
            const bool col_ok = co < p.Cout;
            const int coc = col_ok ? co : p.Cout - 1;
            const float bv = p.bias ? p.bias[coc] : 0.0f;
            uint32_t off[16];
            float rv[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ml = (wm * MB + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                off[r] = (uint32_t)(ml < rows ? ml : rows - 1) * (uint32_t)p.Cout + (uint32_t)coc;
            }
            if (p.res) {
#pragma unroll
                for (int r = 0; r < 16; ++r) rv[r] = rb[off[r]];
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ml = (wm * MB + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                float v = acc[i][j][r];
                if (p.bias) v = v + bv;
                if (p.res) v = v + rv[r];
                if (p.clip) v = v < -1.0f ? -1.0f : (v > 1.0f ? 1.0f : v);
                if (col_ok && ml < rows) yb[off[r]] = v;
            }
        }
}

using Conv16T128x128 = Conv16Cfg<2, 2, 2, 2>;    // every wide layer: 8 MFMAs per wave and step
using Conv16T64x64 = Conv16Cfg<2, 2, 1, 1>;      // 64 output channels, or too few 128 x 128 tiles for the machine
using Conv16T128x32 = Conv16Cfg<4, 1, 1, 1>;     // 32 output channels
LWM_KERNEL_OCC(256, 2) void conv16_igemm_128x128(ConvParams p) { conv16_body<2, 2, 2, 2>(p); }
LWM_KERNEL(256) void conv16_igemm_64x64(ConvParams p) { conv16_body<2, 2, 1, 1>(p); }
LWM_KERNEL(256) void conv16_igemm_128x32(ConvParams p) { conv16_body<4, 1, 1, 1>(p); }

}  // namespace lwm
