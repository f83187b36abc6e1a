// attn_bwd64.h -- blockwise attention backward, ONE WAVE PER SIMD (the structure of attn_fwd64.h): the dK/dV kernel
// and (second half of the file) the dQ kernel of the two-kernel backward for one (q block, kv block) ring step on
// gfx950.  Requires wave_ops.h, attn_common.h, attn_fwd.h, attn_fwd64.h (f4_* instruction helpers) and attn_bwd.h (the
// delta kernel, the layout of the row statistics).
//
// Matrix instruction of both kernels: v_mfma_f32_16x16x32_bf16 (the forward uses 32x32x16).  At its power limit the chip
// holds a higher clock on this shape -- same FLOP, same cycles per FLOP, 7 - 18 % more FLOP/s on random operands
// (profiles/r09_dq16.md, profiles/r17_dkdv16.md) -- so a unit is the 32 x 32 one cut into 16 x 16 tiles at the same
// bytes and registers.  Operand maps (lane l: c = l & 15, g = l >> 4): A holds row c, k = 8g .. 8g+7; B holds column c,
// the same k; C / D hold column c, rows 4g .. 4g+3.
//
// dK/dV: replaces the dk / dv part of the custom-VJP backward of `ringattention` (call site lwm/llama.py:539-569;
// SURVEY.md Appendix A.1): p from the saved LSE, dv += p^T do, dp = do v^T, ds = p * (dp - rowsum(do * o)),
// dk += ds^T q * scale.  It is the mirror of the dQ kernel below (keys <-> queries, K | V <-> Q | dO).
//
// Workgroup = 4 waves = 128 keys; a wave owns 32 keys = two halves kh of 16 and the SIMD's whole register file: its K
// and V fragments (B operands, 32 + 32 registers) and the f32 dK^T / dV^T accumulators (64 + 64) live in the
// accumulator file -- 192 AGPRs -- so the only LDS traffic of the tile loop is the streamed operand, every address
// register-resident (no v_xor).  Q / dO arrive by LDS-DMA in steps of 64 queries through a ring of four 32-KiB slots:
// the pieces of step i+2 are issued in the first phase of step i and have landed, for every wave, at the barrier that
// ends step i -- a whole step before their first reader, which is what lets the last phase of step i+1 request the
// first fragments of step i+2 across the barrier.  The row statistics (attn_bwd.h: -lse * log2 e, -delta, padded)
// travel the same way, one dword per lane.
//
// A unit = 32 queries (two halves qh of 16) x the wave's 32 keys = two phases of 32 MFMAs, written as `asm volatile`
// statements in program order (attn_fwd64.h explains why), with the vector work placed in the gaps:
//
//   phase   matrix pipe (neighbours share an operand, never an accumulator)        vector pipe (same wave)
//   X(u)    S(u)[qh][kh] = Q(u) K^T and dP'(u) = dO(u) V^T - delta: 16 row          the vector work of unit u-1 continues:
//           fragments (ds_read_b128, 8 Q + 8 dO), each feeds the two kh: 32         dS = p dP', P and dS -> bf16
//   Y(u)    dV^T[db < 8][kh] += dO(u-1)^T(db) P(u-1)[kh], dK^T the same with Q^T    t = S(u) c - lse2, p(u) = exp2(t)
//           and dS: 16 transposed fragments (2 x ds_read_b64_tr_b16), each
//           feeds the two kh: 32
//
// D leaves column = key and rows = queries 4g .. 4g+3 of the half, so lse2 and -delta are per-ROW values, loaded by row
// group from the statistics slot: -delta enters as the C operand of the first MFMA of each dP chain, so the chain leaves
// dP' = dP - delta and dS is ONE multiply: 64 VALU per 64 MFMAs.  The B operand of Y is the packed P (dS) of the subtiles
// (qh = 0, kh) | (qh = 1, kh) as the MFMAs left them, which puts k-group g at queries {4g .. 4g+3, 16+4g .. 16+4g+3}: the
// transposed read takes its first four queries from rows 4g .., its second four from rows 16+4g ...  The products lag one
// unit; S needs one set of register tiles, dP' two (the multiply of unit u-1 runs beside the chains of unit u).
//
// LDS map: slot 0..3 = [Q tile 64 rows | dO tile 64 rows] (16 KiB each) | stats 0..3 = [nl2 64 | -delta 64 | seg_q 64]
// Tile image of both kernels: 256-byte rows, slot s of row r at physical slot s ^ q4_swz(r).  The swizzle of attn_common.h
// would leave both reads of this operand shape 2-way (the b128 lane groups take rows 0-3, 12-15 at one slot and rows 4-11
// at its neighbour; a half-wave of the transposed read takes 8 consecutive rows x 32 bytes); this one has
//   * q4_swz(r) ^ [4 <= r&15 < 12] a bijection of r & 15      -> the row reads are conflict-free,
//   * q4_swz(r) >> 1 a bijection of r & 7                     -> the transposed reads are conflict-free
// (q4_image_ok enumerates every lane group of every read of a unit at compile time).
#pragma once

namespace lwm {

constexpr int kD4BK = 128;      // keys per workgroup
constexpr int kD4BQ = 64;       // queries per step (two units of 32)
constexpr int kD4Threads = 256;
constexpr int kD4Slots = 4;
constexpr int kD4TileBytes = kD4BQ * kRowBytes;          // 16 KiB
constexpr int kD4SlotBytes = 2 * kD4TileBytes;           // Q | dO
constexpr int kD4OffStat = kD4Slots * kD4SlotBytes;      // 128 KiB
constexpr int kD4StatBytes = 3 * kD4BQ * 4;              // nl2 | delta | seg_q
constexpr int kD4LdsBytes = kD4OffStat + kD4Slots * kD4StatBytes;
// LDS fragments are requested kD4Ahead fragments before the MFMAs that consume them, through ONE register ring of
// eight that all phases share (fragment m of a unit lives in ring[m % 8]).
#ifndef LWM_D4_AHEAD
#define LWM_D4_AHEAD 6
#endif
constexpr int kD4Ahead = LWM_D4_AHEAD;
static_assert(kD4Ahead >= 1 && kD4Ahead <= 7, "prefetch distance in fragments");
// Fragments are requested and consumed in PAIRS: both requests go out in one gap, and the pair's YOUNGER fragment is
// consumed first -- the s_waitcnt hipcc puts in front of that MFMA covers the older one too.
static_assert((kD4Ahead % 2) == 0, "paired requests need an even distance");

// ---- the tile image (see the file header)
constexpr int q4_swz_of(int row) {
    const int r = row & 15;
    return (((r & 7) << 1) | (r >> 3)) ^ ((r >= 4 && r < 12) ? 1 : 0);
}
LWM_DEVICE int q4_swz(int row) { return q4_swz_of(row); }
LWM_DEVICE uint32_t q4_tile_off(int row, int slot) { return (uint32_t)(row * kRowBytes + ((slot ^ q4_swz(row)) << 4)); }
// Every lane group of every read of a unit hits one address per bank (MI355X: 64 banks of 4 bytes for both reads; a
// ds_read_b128 is served in four groups of 16 lanes -- {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32 --, a
// ds_read_b64_tr_b16 in the two halves of the wave).  Row fragment: lane (c, g) reads slot 4 s + g of row c; transposed
// fragment: lane t of group g reads 8 bytes at d 16 db + 4 (t & 3) of row 4 g + (t >> 2) (and of that row + 16).
constexpr bool q4_image_ok() {
    for (int s = 0; s < 4; ++s)
        for (int grp = 0; grp < 4; ++grp) {
            unsigned long long banks = 0;
            for (int l = 0; l < 64; ++l) {
                const int m = l & 31;
                const bool first = m < 4 || (m >= 12 && m < 16) || (m >= 20 && m < 28);
                if (2 * (l >> 5) + (first ? 0 : 1) != grp) continue;
                const int slot = (4 * s + (l >> 4)) ^ q4_swz_of(l & 15);
                const unsigned long long b = 0xFull << (4 * slot);
                if (banks & b) return false;
                banks |= b;
            }
            if (banks != ~0ull) return false;
        }
    for (int db = 0; db < 8; ++db)
        for (int up = 0; up < 2; ++up)
            for (int half = 0; half < 2; ++half) {
                unsigned long long banks = 0;
                for (int l = 32 * half; l < 32 * half + 32; ++l) {
                    const int g = l >> 4, t = l & 15, row = 16 * up + 4 * g + (t >> 2);
                    const int slot = (2 * db + ((t & 3) >> 1)) ^ q4_swz_of(row);
                    const unsigned long long b = 0x3ull << (4 * slot + 2 * (t & 1));
                    if (banks & b) return false;
                    banks |= b;
                }
                if (banks != ~0ull) return false;
            }
    return true;
}
static_assert(q4_image_ok(), "a read of the Q | dO (K | V) image is bank-conflicted");

// ---- the 16x16x32 statements of both kernels
#ifdef LWM_EMU
// host form of v_mfma_f32_16x16x32_bf16 from its operand maps (scripts/micro/mfma_timing.hip prints the device's;
// tests/test_gpu_dq16.py holds the device kernel to the oracle the emulated one meets)
LWM_DEVICE f32x4 mfma_16x16x32(bf16x8 a, bf16x8 b, f32x4 c) {
    emu::Wave& w = emu::g_blk->waves[emu::g_lane->tid >> 6];
    const int l = emu::g_lane->tid & 63;
    w.a[l] = a;
    w.b[l] = b;
    emu::wave_sync();
    f32x4 d;
    const int col = l & 15, g = l >> 4;
    for (int j = 0; j < 4; ++j) {
        const int row = 4 * g + j;
        float s = c[j];
        for (int k = 0; k < 32; ++k) s += (float)w.a[(k >> 3) * 16 + row][k & 7] * (float)w.b[(k >> 3) * 16 + col][k & 7];
        d[j] = s;
    }
    emu::wave_sync();
    return d;
}
LWM_DEVICE void q4_mfma_first(f32x4& d, bf16x8 a, bf16x8 b) { d = mfma_16x16x32(a, b, f32x4{0.0f, 0.0f, 0.0f, 0.0f}); }
LWM_DEVICE void q4_mfma(f32x4& d, bf16x8 a, bf16x8 b) { d = mfma_16x16x32(a, b, d); }
LWM_DEVICE void q4_mfma_c_first(f32x4& d, bf16x8 a, bf16x8 b, const f32x4& c) { d = mfma_16x16x32(a, b, c); }
LWM_DEVICE void q4_mfma_o(f32x4& d, bf16x8 a, bf16x8 b) { d = mfma_16x16x32(a, b, d); }
LWM_DEVICE void q4_mfma_o_first(f32x4& d, bf16x8 a, bf16x8 b) { d = mfma_16x16x32(a, b, f32x4{0.0f, 0.0f, 0.0f, 0.0f}); }
LWM_DEVICE void q4_opaque(f32x4 (&)[2]) {}
LWM_DEVICE void q4_settle_t(f32x4 (&)[4]) {}
LWM_DEVICE void q4_settle_acc(f32x4 (&)[16]) {}
#else
// the statements of attn_fwd64.h on the 16x16 shape: S chains (B from the accumulator file), the first MFMA of a dP
// chain (C = the -delta tuple, two wait states in front, see d4_mfma_p_first), the products into the accumulator file
LWM_DEVICE void q4_mfma_first(f32x4& d, bf16x8 a, bf16x8 b) {
    asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, 0" : "=&v"(d) : "v"(a), "a"(b));
}
LWM_DEVICE void q4_mfma(f32x4& d, bf16x8 a, bf16x8 b) {
    asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(d) : "v"(a), "a"(b));
}
LWM_DEVICE void q4_mfma_c_first(f32x4& d, bf16x8 a, bf16x8 b, const f32x4& c) {
    asm volatile("s_nop 1\n\tv_mfma_f32_16x16x32_bf16 %0, %1, %2, %3" : "=&v"(d) : "v"(a), "a"(b), "v"(c));
}
LWM_DEVICE void q4_mfma_o(f32x4& d, bf16x8 a, bf16x8 b) {
    asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(d) : "v"(a), "v"(b));
}
LWM_DEVICE void q4_mfma_o_first(f32x4& d, bf16x8 a, bf16x8 b) {
    asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, 0" : "=&a"(d) : "v"(a), "v"(b));
}
// registers that hold the same value: hipcc must not know (it would keep one and copy it into a tuple in front of
// every chain)
LWM_DEVICE void q4_opaque(f32x4 (&x)[2]) { asm volatile("" : "+v"(x[0]), "+v"(x[1])); }
LWM_DEVICE void q4_settle_t(f32x4 (&s)[4]) { asm volatile("s_nop 7\n\ts_nop 7" : "+v"(s[0]), "+v"(s[1]), "+v"(s[2]), "+v"(s[3])); }
LWM_DEVICE void q4_settle_acc(f32x4 (&a)[16]) {
    asm volatile("s_nop 7\n\ts_nop 7"
                 : "+a"(a[0]), "+a"(a[1]), "+a"(a[2]), "+a"(a[3]), "+a"(a[4]), "+a"(a[5]), "+a"(a[6]), "+a"(a[7]), "+a"(a[8]),
                   "+a"(a[9]), "+a"(a[10]), "+a"(a[11]), "+a"(a[12]), "+a"(a[13]), "+a"(a[14]), "+a"(a[15]));
}
#endif

// ====================================================================================================== dS hand-over
// The dK/dV kernel holds every dS it computes as packed bf16 B operands of its dK chain; the recompute dQ kernel spends
// two of its three GEMM units on producing the same numbers again.  With a workspace (LwmAttnArgs::ds_ws) the dK/dV
// kernel stores them and attn_bwd_dq_ds_kernel (end of the file) computes dQ = scale * dS K from them in ONE unit.
//
// Workspace = tiles of kDsTileBytes: tile (b, h, key block kbi, wave w, step st) = the dS of the 64 queries of step st
// against the 32 keys of wave w of key block kbi, in the order the dK/dV walk leaves them:
//   [unit = query half of the step: 2][key half kh: 2][lane (c, g) of the producer: 64][16 bytes]
// where the lane's 16 bytes are its dK-chain operand as it stands: key 16 kh + c, queries 4g .. 4g+3 | 16+4g .. 16+4g+3
// of the unit.  Only the steps a key block's walk visits have a tile (causal: steps from ds_first_step on -- the others
// lie wholly before the block's first key and every dS there is 0), rows of tiles are laid out [b, h][kbi][w][st - first],
// so that a wave's walk writes one run of memory (descending) and the four waves of a consumer workgroup read 16
// consecutive KiB per key step.  Eligible calls have one piece per operand, Sq % 64 == 0, Sk % 128 == 0 and no key meta,
// so everything below is a function of (causal, q_start, k_start, Sq, Sk) -- the same on the host (api.inc sizes the
// workspace with it) and in both kernels.
constexpr int kDsTileBytes = kD4BQ * 32 * 2;      // 4 KiB
// e: step st is visited by key block kbi iff st >= e + 2 kbi (the kernel's tiles_below on one piece: the steps wholly
// before key k_start + 128 kbi are the first floor((k_start - q_start + 128 kbi) / 64)); not causal: every step
constexpr int64_t ds_diag(int causal, int64_t q_start, int64_t k_start) {
    const int64_t lim = (int64_t)1 << 30, e = (k_start - q_start) >> 6;
    return !causal ? -lim : (e < -lim ? -lim : (e > lim ? lim : e));
}
constexpr int64_t ds_first_step(int64_t e, int64_t nst, int64_t kbi) {
    const int64_t s = e + 2 * kbi;
    return s < 0 ? 0 : (s > nst ? nst : s);
}
// tiles per wave in the key blocks before kbi: sum over j < kbi of nst - ds_first_step(e, nst, j), in closed form
constexpr int64_t ds_steps_before(int64_t e, int64_t nst, int64_t kbi) {
    const int64_t jl = e >= 0 ? 0 : (1 - e) >> 1;               // first key block with e + 2 j >= 0
    const int64_t jh0 = e >= nst ? 0 : (nst - e + 1) >> 1;      // first key block with e + 2 j >= nst
    const int64_t jh = jh0 > jl ? jh0 : jl;
    const int64_t a = kbi < jl ? kbi : jl, b = kbi < jh ? kbi : jh;
    return kbi * nst - ((b - a) * e + (b - a) * (a + b - 1) + (kbi - b) * nst);
}
constexpr bool ds_geom_ok() {
    const int64_t es[] = {-(1 << 30), -1000, -9, -8, -3, -2, -1, 0, 1, 2, 3, 7, 8, 9, 40, 1 << 30};
    const int64_t ns[] = {1, 2, 3, 4, 6, 8, 9, 32};
    for (int64_t e : es)
        for (int64_t nst : ns) {
            int64_t sum = 0;
            for (int64_t kbi = 0; kbi < 24; ++kbi) {
                if (ds_steps_before(e, nst, kbi) != sum) return false;
                sum += nst - ds_first_step(e, nst, kbi);
            }
        }
    return true;
}
static_assert(ds_geom_ok(), "closed form of the workspace row offsets disagrees with the sum it stands for");
// 32-key steps of the consumer's walk that hold a tile for query step s (they are the FIRST ones: ds_first_step ascends
// with the key block); 0 for a step past the operand
constexpr int64_t ds_wave_steps(int64_t e, int64_t nst, int64_t nkb, int64_t s) {
    if (s >= nst) return 0;
    const int64_t kend = s - e < 0 ? 0 : ((s - e) >> 1) + 1;
    return 4 * (kend < nkb ? kend : nkb);
}
// bytes of the workspace (0: nothing to hand over)
constexpr int64_t ds_ws_bytes(int64_t B, int64_t H, int64_t Sq, int64_t Sk, int causal, int64_t q_start, int64_t k_start) {
    return B * H * ds_steps_before(ds_diag(causal, q_start, k_start), Sq / kD4BQ, Sk / kD4BK) * 4 * kDsTileBytes;
}

// The producer's side: unit u's dS leave from the gaps W of the schedule table (phase X of unit u+1, or the drain), one
// lane-linear 16-byte store per key half = 1 KiB per instruction.  sw.p = the tile of the RUNNING step + kDsTileBytes, a
// scalar pointer that steps down with the walk, so that both cases fit the instruction's 13-bit offset: the first unit
// of the running step (stored from the step's second X phase) at BASE = -kDsTileBytes, the second unit of the step
// BEFORE (stored from the running step's first X phase, or from the drain) at BASE = kDsTileBytes / 2.
struct D4Ds {
    char* p;
    uint32_t v;         // 16 * lane
};
#ifdef LWM_EMU
LWM_DEVICE char* ds_uniform_ptr(char* p) { return p; }
template <int OFF>
LWM_DEVICE void d4_ds_store(const D4Ds& sw, bf16x8 x) { memcpy(sw.p + OFF + sw.v, &x, 16); }
#else
LWM_DEVICE char* ds_uniform_ptr(char* p) {
    const uint64_t a = (uint64_t)p;
    return (char*)(((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(a >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)a));
}
// (asm: hipcc does not count it, so it neither waits for it nor drains the LDS-DMA pieces around it.  Non-temporal: the
// tiles are read once, by another kernel, and 34 GB of them per layer at the bench shape would push the Q / dO tiles the
// key blocks of an XCD share out of its L2 -- measured: 17.2 ms with the hint, 18.4 ms without, 13.4 ms with no stores)
template <int OFF>
LWM_DEVICE void d4_ds_store(const D4Ds& sw, bf16x8 x) {
    static_assert(OFF >= -4096 && OFF <= 4095, "13-bit signed instruction offset");
    asm volatile("global_store_dwordx4 %0, %1, %2 offset:%3 nt" ::"v"(sw.v), "v"(x), "s"(sw.p), "n"(OFF) : "memory");
}
#endif

// ====================================================================================================== dK/dV
struct D4Ctx {
    uint32_t qa[4];             // Q row-fragment addresses (d step s of 32), rows 0..15 of the CURRENT step's Q tile
    uint32_t tlo[8];            // Q transposed-fragment addresses (d block of 16), rows 4g.. of the current step's Q tile
    uint32_t plo[8];            // the same in the PREVIOUS step's slot (the lagging products of a step's first unit)
    uint32_t stat;              // this step's statistics + 16 * g
    float c;                    // scale * log2(e)
};

#ifdef LWM_EMU
LWM_DEVICE float d4_mul(float a, float b) { return a * b; }
LWM_DEVICE void d4_dma_b32(uint32_t voff, const char* src, lds_t dst) { glds_load_b32(src + voff, dst); }
LWM_DEVICE void d4_settle_acc4(f32x16 (&)[4]) {}
#else
LWM_DEVICE float d4_mul(float a, float b) {
    float y;
    asm volatile("v_mul_f32 %0, %1, %2" : "=v"(y) : "v"(a), "v"(b));
    return y;
}
// one LDS-DMA dword per lane (64 floats of row statistics), M0 written bare as f4_dma1 does
LWM_DEVICE void d4_dma_b32(uint32_t voff, const char* src, lds_t dst) {
    const uint64_t a = (uint64_t)src;
    const uint64_t u = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(a >> 32)) << 32) |
                       (uint32_t)__builtin_amdgcn_readfirstlane((int)a);
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %0, %1" ::"v"(voff), "s"(u), "s"(dst) : "memory");
}
// (gemm_wgrad.h: 32x32 tuples)
LWM_DEVICE void d4_settle_acc4(f32x16 (&a)[4]) { asm volatile("s_nop 7\n\ts_nop 7" : "+a"(a[0]), "+a"(a[1]), "+a"(a[2]), "+a"(a[3])); }
#endif
// What hipcc does not know about an asm MFMA (cdna_hip_programming.md section 5.7 item 2): a register it has just
// written itself -- a copy that moves a tuple into place, a zero it materialises late -- needs two wait states before
// an MFMA reads it, and a register an MFMA writes is not ready when the MFMA has issued.  The statements below are used
// where that can happen:
//   * the first MFMA of a dP chain: its C operand, the -delta tuple, was filled by compiler-visible LDS loads, which
//     hipcc may route through copies: two wait states stand in front of the MFMA;
//   * the first product of the walk into each dK^T / dV^T tuple: C = 0 and an OUTPUT-only operand, so that no
//     compiler-made zero is read at all;
//   * where compiler-generated code reads the S tiles or the accumulators (the mask code, a control-flow merge, the
//     epilogue): wait states in a statement that names the tuples, so that every later use follows them.  The
//     accumulators take two statements (an asm statement has 30 operands at most): dK^T first -- the LAST four MFMAs
//     of a Y phase and of the drain write dK^T tuples, the last write of a dV^T tuple lies four MFMAs further back.
LWM_DEVICE void d4_mfma_p_first(f32x4& d, bf16x8 a, bf16x8 b, const f32x4& c) { q4_mfma_c_first(d, a, b, c); }
LWM_DEVICE void d4_mfma_o_first(f32x4& d, bf16x8 a, bf16x8 b) { q4_mfma_o_first(d, a, b); }
LWM_DEVICE void d4_settle_t(f32x4 (&s)[4]) { q4_settle_t(s); }
LWM_DEVICE void d4_settle_acc(f32x4 (&dk)[16], f32x4 (&dv)[16]) {
    q4_settle_acc(dk);
    q4_settle_acc(dv);
}

// per-lane byte offsets of the wave's four pieces of a 64-row tile (piece = 4 rows = 1 KiB; wave w moves pieces
// w, w+4, w+8, w+12: rows 4w + 16j + (l>>4)) relative to the step's first row, rows clamped to Sq-1 (rows past Sq
// get nl2 = -inf through the statistics).  Lane l writes physical slot l&15 of its row, so it fetches logical slot
// (l&15) ^ q4_swz(row) -- the XOR swizzle applied on the SOURCE column.
LWM_DEVICE void d4_stage_offsets(const AttnParams& p, int wave, int lane, int st, uint32_t (&vq)[4], uint32_t (&vdo)[4]) {
    const int slot = lane & 15;
    for (int j = 0; j < 4; ++j) {
        const int row = 4 * (wave + 4 * j) + (lane >> 4);
        int qrow = st * kD4BQ + row;
        qrow = qrow < p.Sq ? qrow : p.Sq - 1;
        const int rel = qrow - st * kD4BQ;
        const int col = (slot ^ q4_swz(row)) << 3;
        vq[j] = (uint32_t)(((int64_t)rel * p.q_ss + col) * 2);
        vdo[j] = (uint32_t)(((int64_t)rel * p.do_ss + col) * 2);
    }
}

// fragment f of a unit (32 per unit, each feeds the MFMAs of the two key halves; 32.. = the first fragments of the unit
// that follows).  A PAIR of fragments is one tensor: the MFMAs of a pair run (f+1, kh 0), (f+1, kh 1), (f, kh 1),
// (f, kh 0) -- neighbours share A, then B, then A -- and the next pair is the other tensor.
//   0..15   phase X: pair f>>1 = (d step s = f>>2, tensor (f>>1)&1: 0 = Q row fragment (S), 1 = dO (dP')); query half f&1
//   16..31  phase Y: j = f-16, pair j>>1 = (tensor (j>>1)&1: 0 = dO^T (dV), 1 = Q^T (dK)); d block 2 (j>>2) + (j&1) of the
//           PREVIOUS unit: queries 4g.. (first read) and 16+4g.. (second read)
// cx.qa points at the step's slot for HALF = 0 and for the X phase of HALF = 1; it has moved on to the next step's slot
// when the Y phase of HALF = 1 requests f >= 32.
template <int HALF>
LWM_DEVICE bf16x8 d4_frag(const D4Ctx& cx, int f) {
    if (f >= 32) {
        const int g = f - 32;
        return lds_read_b128(cx.qa[g >> 2] + ((g >> 1) & 1) * kD4TileBytes + (g & 1) * 16 * kRowBytes + (HALF == 0 ? 32 * kRowBytes : 0));
    }
    if (f < 16) return lds_read_b128(cx.qa[f >> 2] + ((f >> 1) & 1) * kD4TileBytes + (f & 1) * 16 * kRowBytes + HALF * 32 * kRowBytes);
    const int j = f - 16, db = 2 * (j >> 2) + (j & 1);
    // the previous unit: the second half of the previous step's tiles for HALF = 0, the first half of this step's
    const uint32_t a = (HALF == 0 ? cx.plo[db] : cx.tlo[db]) + (HALF == 0 ? 32 * kRowBytes : 0) + (((j >> 1) & 1) ? 0 : kD4TileBytes);
    bf16x4 lo = lds_read_tr16(a);
    bf16x4 up = lds_read_tr16(a + 16 * kRowBytes);
    bf16x8 o;
    o[0] = lo[0]; o[1] = lo[1]; o[2] = lo[2]; o[3] = lo[3];
    o[4] = up[0]; o[5] = up[1]; o[6] = up[2]; o[7] = up[3];
    return o;
}

// ---- where the vector work of a unit u goes.  Gaps are numbered over the two phases that host it: G = 0..31 = the
// gaps of Y(u) (gap = behind that MFMA), G = 32..63 = the gaps of X(u+1).  An MFMA holds the vector issue for 8 of its 16
// cycles, so a gap takes two plain VALU or one v_exp_f32 beside its LDS read.  Per element e (16 per lane: key half
// e >> 3, query half (e >> 2) & 1, row e & 3 of the group -- score tile e >> 2) / per pair i (8 per lane):
//   F(e)  t = S c - lse2          3 <= G (three MFMAs between the end of the S chains and their first reader), G <= 31
//                                 (X(u+1) overwrites S)
//   E(e)  p = exp2(t)             behind F(e)
//   M(e)  dS = p dP'              behind E(e)
//   P(i)  P words -> bf16         behind E(2i), E(2i+1); the products of Y(u) read the OLD words to their last MFMA:
//   D(i)  dS words -> bf16        G >= 32; D(i) behind M(2i), M(2i+1); everything done by G = 61
// The words of a key half are four consecutive packed registers, ready as the B operand of Y.
//   W(h)  dS of key half h -> HBM   (hand-over instantiation only, "dS hand-over" below) behind the half's last D; in
//                                 gap 63: behind the last LDS-DMA piece of a step's first phase, so that the stores are
//                                 the YOUNGEST vector-memory operations of a step and its counted wait leaves them in flight
struct D4Sched {
    int F[16], E[16], M[16], P[8], D[8], W[2];
};
constexpr bool d4_sched_ok(const D4Sched& c) {
    int load[64] = {};
    for (int e = 0; e < 16; ++e) {
        if (c.F[e] < 3 || c.F[e] > 31 || c.E[e] <= c.F[e] || c.M[e] <= c.E[e] || c.M[e] > 61) return false;
        load[c.F[e]] += 1;
        load[c.E[e]] += 2;
        load[c.M[e]] += 1;
    }
    for (int i = 0; i < 8; ++i) {
        if (c.P[i] < 32 || c.P[i] > 61 || c.P[i] <= c.E[2 * i] || c.P[i] <= c.E[2 * i + 1]) return false;
        if (c.D[i] < 32 || c.D[i] > 61 || c.D[i] <= c.M[2 * i] || c.D[i] <= c.M[2 * i + 1]) return false;
        load[c.P[i]] += 1;
        load[c.D[i]] += 1;
    }
    for (int h = 0; h < 2; ++h) {
        if (c.W[h] != 63) return false;
        for (int i = 4 * h; i < 4 * h + 4; ++i)
            if (c.W[h] <= c.D[i]) return false;
    }
    for (int g = 0; g < 64; ++g)
        if (load[g] > 2) return false;      // (in units of a plain VALU's issue; an exp counts two)
    return true;
}
// exponentials in Y (beside the transposed reads), multiplies and packs in X
constexpr D4Sched kD4Sched = {
    /* F */ {3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10},
    /* E */ {11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26},
    /* M */ {27, 27, 28, 28, 29, 29, 30, 30, 31, 31, 32, 32, 33, 33, 34, 34},
    /* P */ {35, 35, 36, 36, 37, 37, 38, 38},
    /* D */ {39, 39, 40, 40, 41, 41, 42, 42},
    /* W */ {63, 63}};
static_assert(d4_sched_ok(kD4Sched), "filler schedule violates a dependency or the issue budget of a gap");

// the LDS-DMA pieces one step issues (all wave-uniform but the offsets): Q and dO of the step two ahead
struct D4Dma {
    const char* q_src;
    const char* do_src;
    lds_t dst;          // the slot's Q tile + wave * 1024
};

// Live state of a wave across units.
struct D4Regs {
    f32x4 s[4];             // S tiles [2 kh + qh] (MFMA results, read-only for the vector pipe but for the masks)
    f32x4 dp[2][4];         // dP' tiles by unit parity
    f32x4 ndl[2];           // -delta of rows 4g.. of the unit's query halves: the C operand that starts each dP chain
    float nl[8];            // -lse * log2(e) of the same rows [4 qh + j]
    float t[16];            // exponents, then p
    float ds[16];           // dS = p * dP'
    bf16x8 pb[2], dsb[2];   // P / dS as B operands, by key half
    uint32_t pw[8], dw[8];  // their words as they are packed (a half is handed over when its fourth word is in)
    bf16x8 fr[8];           // the fragment ring
};

// the vector work scheduled in gap G for the unit of parity PAR
template <int G, int PAR>
LWM_DEVICE void d4_fillers(const D4Ctx& cx, D4Regs& rg) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        if (kD4Sched.F[e] == G) rg.t[e] = f4_fma(rg.s[e >> 2][e & 3], cx.c, rg.nl[4 * ((e >> 2) & 1) + (e & 3)]);
        if (kD4Sched.E[e] == G) rg.t[e] = f4_exp2(rg.t[e]);
        if (kD4Sched.M[e] == G) rg.ds[e] = d4_mul(rg.t[e], rg.dp[PAR][e >> 2][e & 3]);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        if (kD4Sched.P[i] == G) rg.pw[i] = f4_cvt_pk(rg.t[2 * i], rg.t[2 * i + 1]);
        if (kD4Sched.D[i] == G) rg.dw[i] = f4_cvt_pk(rg.ds[2 * i], rg.ds[2 * i + 1]);
    }
    // hand a half over behind its last word
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        int lp = 0, ld = 0;
        for (int i = 4 * h; i < 4 * h + 4; ++i) {
            lp = kD4Sched.P[i] > lp ? kD4Sched.P[i] : lp;
            ld = kD4Sched.D[i] > ld ? kD4Sched.D[i] : ld;
        }
        if (lp == G) rg.pb[h] = __builtin_bit_cast(bf16x8, u32x4{rg.pw[4 * h], rg.pw[4 * h + 1], rg.pw[4 * h + 2], rg.pw[4 * h + 3]});
        if (ld == G) rg.dsb[h] = __builtin_bit_cast(bf16x8, u32x4{rg.dw[4 * h], rg.dw[4 * h + 1], rg.dw[4 * h + 2], rg.dw[4 * h + 3]});
    }
}

// the hand-over stores scheduled in gap G (the unit's tile half begins at sw.p + BASE)
template <int G, int BASE>
LWM_DEVICE void d4_ds_stores(const D4Ds& sw, const D4Regs& rg) {
    if constexpr (kD4Sched.W[0] == G) d4_ds_store<BASE>(sw, rg.dsb[0]);
    if constexpr (kD4Sched.W[1] == G) d4_ds_store<BASE + 1024>(sw, rg.dsb[1]);
}

// Every MFMA index below is a template parameter (the phases are recursions, not loops): fragment, tile and filler
// selection must be constants, or the register arrays they index go to scratch.
//
// Phase X of unit u (parity HALF): 32 MFMAs, fragment (M>>1)^1 (a pair is requested every fourth gap, its YOUNGER
// fragment consumed first: one wait per four MFMAs), key half ((M>>1)^M)&1; fillers: gaps 32..63 of unit u-1.  A dependent
// MFMA finds its predecessor eight MFMAs back.  The first kD4Ahead fragments are ALREADY in the ring, rg.ndl holds the
// unit's -delta; the unit's -lse * log2 e is read here (needed from gap 3 of phase Y).
template <int HALF, bool HAS_PREV, bool DMA, bool DS, int M = 0>
LWM_DEVICE void d4_x(const D4Ctx& cx, D4Regs& rg, const bf16x8 (&kf)[8], const bf16x8 (&vf)[8], const uint32_t (&vq)[4],
                     const uint32_t (&vdo)[4], const D4Dma& dm, const D4Ds& sw) {
    if constexpr (M < 32) {
        if constexpr ((M & 3) == 0) {
            constexpr int f0 = (M >> 1) + kD4Ahead;
            rg.fr[f0 & 7] = d4_frag<HALF>(cx, f0);
            sched_fence();      // (the pair in this order: the wait for the younger fragment then covers both)
            rg.fr[(f0 + 1) & 7] = d4_frag<HALF>(cx, f0 + 1);
        }
        if constexpr (M == 10 || M == 18) {
            constexpr int qh = M == 18 ? 1 : 0;
            const f32x4 v = lds_read_f32x4(cx.stat + (HALF * 32 + 16 * qh) * 4);
            rg.nl[4 * qh + 0] = v[0]; rg.nl[4 * qh + 1] = v[1]; rg.nl[4 * qh + 2] = v[2]; rg.nl[4 * qh + 3] = v[3];
        }
        sched_fence();
        {
            constexpr int f = (M >> 1) ^ 1, qh = f & 1, kh = ((M >> 1) ^ M) & 1;
            constexpr int s = f >> 2, t = 2 * kh + qh;
            if constexpr (((f >> 1) & 1) == 0) {
                if constexpr (s == 0) q4_mfma_first(rg.s[t], rg.fr[f & 7], kf[4 * kh]);
                else q4_mfma(rg.s[t], rg.fr[f & 7], kf[4 * kh + s]);
            } else {
                if constexpr (s == 0) d4_mfma_p_first(rg.dp[HALF][t], rg.fr[f & 7], vf[4 * kh], rg.ndl[qh]);
                else q4_mfma(rg.dp[HALF][t], rg.fr[f & 7], vf[4 * kh + s]);
            }
        }
        if constexpr (DMA && (M & 3) == 3) {      // the wave's 4 Q and 4 dO pieces of the step two ahead, all in the step's first phase
            constexpr int i = M >> 2, j = i >> 1;
            if constexpr ((i & 1) == 0) f4_dma1(vq[j], dm.q_src, dm.dst + 4096 * j);
            else f4_dma1(vdo[j], dm.do_src, dm.dst + kD4TileBytes + 4096 * j);
        }
        if constexpr (HAS_PREV) d4_fillers<32 + M, HALF ^ 1>(cx, rg);
        if constexpr (HAS_PREV && DS) d4_ds_stores<32 + M, HALF == 1 ? -kDsTileBytes : kDsTileBytes / 2>(sw, rg);
        sched_fence();
        d4_x<HALF, HAS_PREV, DMA, DS, M + 1>(cx, rg, kf, vf, vq, vdo, dm, sw);
    }
}

// masks of a unit on its scores (lwm/llama.py:572-592): query row 16 qh + 4g + j of the unit sees the lane's key of half
// kh iff it is not before it (rel[kh] = key position - position of the unit's row 0 - 4g, clamped) and, with key meta,
// shares its segment (kseg = kSegInvalid for a padded / out-of-range key)
template <int HALF, bool HAS_META>
LWM_DEVICE void d4_mask(const D4Ctx& cx, f32x4 (&s)[4], const int (&rel)[2], const int32_t (&kseg)[2]) {
#pragma unroll
    for (int qh = 0; qh < 2; ++qh) {
        u32x4 sg = {0u, 0u, 0u, 0u};
        if (HAS_META) sg = lds_read_u32x4(cx.stat + 2 * kD4BQ * 4 + HALF * 32 * 4 + 16 * qh * 4);
#pragma unroll
        for (int kh = 0; kh < 2; ++kh)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool vis = (!HAS_META || (int32_t)sg[j] == kseg[kh]) && (16 * qh + j >= rel[kh]);
                s[2 * kh + qh][j] = vis ? s[2 * kh + qh][j] : -INFINITY;
            }
    }
}

// Phase Y of unit u: dV^T += dO(u-1)^T P(u-1) and dK^T += Q(u-1)^T dS(u-1), 32 MFMAs (fragment 16 + ((J>>1)^1), key half
// ((J>>1)^J)&1; every accumulator once)  ||  gaps 0..31 of unit u.  The last gaps request the first fragments of the unit
// that follows and its -delta (statn = the statistics slot of that unit + 16 g).
// INIT: these are the first products of the walk (C = 0: the tuples are defined here).
template <int HALF, bool HAS_PREV, bool NEXT, bool INIT, int J = 0>
LWM_DEVICE void d4_y(const D4Ctx& cx, D4Regs& rg, f32x4 (&dk)[16], f32x4 (&dv)[16], uint32_t statn) {
    if constexpr (J < 32) {
        if constexpr ((J & 3) == 0 && (16 + (J >> 1) + kD4Ahead < 32 || NEXT)) {
            constexpr int f0 = 16 + (J >> 1) + kD4Ahead;
            rg.fr[f0 & 7] = d4_frag<HALF>(cx, f0);
            sched_fence();      // (the pair in this order: the wait for the younger fragment then covers both)
            rg.fr[(f0 + 1) & 7] = d4_frag<HALF>(cx, f0 + 1);
        }
        if constexpr (NEXT && (J == 22 || J == 26)) {
            constexpr int qh = J == 26 ? 1 : 0;
            rg.ndl[qh] = lds_read_f32x4(statn + kD4BQ * 4 + ((HALF ^ 1) * 32 + 16 * qh) * 4);
        }
        sched_fence();
        if constexpr (HAS_PREV) {
            constexpr int jf = (J >> 1) ^ 1, kh = ((J >> 1) ^ J) & 1;
            constexpr int db = 2 * (jf >> 2) + (jf & 1);
            if constexpr (((jf >> 1) & 1) == 0) {
                if constexpr (INIT) d4_mfma_o_first(dv[2 * db + kh], rg.fr[(16 + jf) & 7], rg.pb[kh]);
                else q4_mfma_o(dv[2 * db + kh], rg.fr[(16 + jf) & 7], rg.pb[kh]);
            } else {
                if constexpr (INIT) d4_mfma_o_first(dk[2 * db + kh], rg.fr[(16 + jf) & 7], rg.dsb[kh]);
                else q4_mfma_o(dk[2 * db + kh], rg.fr[(16 + jf) & 7], rg.dsb[kh]);
            }
        }
        d4_fillers<J, HALF>(cx, rg);
        sched_fence();
        d4_y<HALF, HAS_PREV, NEXT, INIT, J + 1>(cx, rg, dk, dv, statn);
    }
}

// the pipeline's tail: the second half of the last unit's vector work, then its dV / dK products (no fillers left).
// PAR = the parity of the last unit (its dP' tiles); its tiles are addressed as the "previous unit" of a HALF = 0 unit.
template <int PAR, bool DS, int G = 32>
LWM_DEVICE void d4_drain_fill(const D4Ctx& cx, D4Regs& rg, const D4Ds& sw) {
    if constexpr (G < 64) {
        d4_fillers<G, PAR>(cx, rg);
        if constexpr (DS) d4_ds_stores<G, kDsTileBytes / 2>(sw, rg);      // (the pointer has moved on: as a step's first phase)
        d4_drain_fill<PAR, DS, G + 1>(cx, rg, sw);
    }
}
template <int H, int J = 0>
LWM_DEVICE void d4_drain_mfma(D4Regs& rg, f32x4 (&dk)[16], f32x4 (&dv)[16]) {
    if constexpr (J < 16) {
        constexpr int jf = 8 * H + (J >> 1), kh = ((J >> 1) ^ J) & 1;
        constexpr int db = 2 * (jf >> 2) + (jf & 1);
        if constexpr (((jf >> 1) & 1) == 0) q4_mfma_o(dv[2 * db + kh], rg.fr[jf & 7], rg.pb[kh]);
        else q4_mfma_o(dk[2 * db + kh], rg.fr[jf & 7], rg.dsb[kh]);
        d4_drain_mfma<H, J + 1>(rg, dk, dv);
    }
}
template <int PAR, bool DS>
LWM_DEVICE void d4_drain(const D4Ctx& cx, D4Regs& rg, f32x4 (&dk)[16], f32x4 (&dv)[16], const D4Ds& sw) {
    d4_drain_fill<PAR, DS>(cx, rg, sw);
#pragma unroll
    for (int j = 0; j < 8; ++j) rg.fr[j] = d4_frag<0>(cx, 16 + j);
    sched_fence();
    d4_drain_mfma<0>(rg, dk, dv);
    sched_fence();
#pragma unroll
    for (int j = 0; j < 8; ++j) rg.fr[j] = d4_frag<0>(cx, 24 + j);
    sched_fence();
    d4_drain_mfma<1>(rg, dk, dv);
    sched_fence();
}

// a wave's dK^T or dV^T tiles -> its epilogue staging tile (attn_common.h, "epilogue staging": the same image as
// epi_tile_write leaves, from the 16 x 16 accumulator layout): lane (c, g) holds, of tile [2 db + kh], the four columns
// 16 db + 4g + 0..3 of row 16 kh + c (the 8 contiguous lanes of a ds_write_b128 group: 8 rows x 4 distinct banks of 32)
LWM_DEVICE void d4_epi_tile_write(lds_t tb, const f32x4 (&acc)[16], float scale, int c, int g) {
#pragma unroll
    for (int db = 0; db < 8; ++db)
#pragma unroll
        for (int kh = 0; kh < 2; ++kh) {
            const f32x4 a = acc[2 * db + kh];
            lds_write_f32x4(tb + (uint32_t)((16 * kh + c) * kEpiRowBytes + (16 * db + 4 * g) * 4),
                            f32x4{a[0] * scale, a[1] * scale, a[2] * scale, a[3] * scale});
        }
}

// The epilogue of a key block: the wave's dK^T (scaled) and dV^T tiles, rows row0 .. row0 + 31 of (b, h), through the
// wave's LDS staging tile at tb (attn_common.h, "epilogue staging"; free of other readers and writers: the caller's
// barrier), merged with the ring carries, stored as whole rows -- bf16 results or f32 partials.  Everything the 32 store
// instructions share is read and computed ONCE (kernel arguments, the lane's first address of each buffer, the
// strides): left inside the row loop, hipcc re-read carry_in / final_out / Sk behind a wait per row and rebuilt the
// 64-bit address products -- 15 k cycles per key block (s_memtime), five times the data movement.
LWM_DEVICE void d4_store_tiles(const AttnParams& p, lds_t tb, const f32x4 (&dk)[16], const f32x4 (&dv)[16], int b, int h,
                               int row0, int lane) {
    const int l31 = lane & 31, hi = lane >> 5, col = l31 * 4;
    const int Sk = p.Sk;
    const bool carry = p.carry_in != 0, fin = p.final_out != 0;
    const int rows = Sk - (row0 + hi);                              // this lane stores rows row0 + hi + 2 i while 2 i < rows
    const int64_t acc0 = ((((int64_t)b * Sk + row0 + hi) * p.H + h) * kHeadDim + col) * 4;       // bytes
    const int64_t acc_step = (int64_t)2 * p.H * kHeadDim * 4;
#pragma unroll
    for (int which = 0; which < 2; ++which) {
        if (which) wave_lds_fence();        // (dK^T's rows have been read)
        d4_epi_tile_write(tb, which ? dv : dk, which ? 1.0f : p.scale, lane & 15, lane >> 4);
        wave_lds_fence();
        char* ap = (char*)(which ? p.dv_acc : p.dk_acc) + acc0;
        const int64_t o_ss = which ? p.dv_ss : p.dk_ss;
        char* op = (char*)((which ? p.dv : p.dk) + (int64_t)b * (which ? p.dv_sb : p.dk_sb) + (int64_t)(row0 + hi) * o_ss +
                           (int64_t)h * (which ? p.dv_sh : p.dk_sh) + col);
        const int64_t out_step = 2 * o_ss * 2;
        if (fin && !carry) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const f32x4 x = epi_tile_read(tb, i, lane);
                if (2 * i < rows) global_store_b64(op + i * out_step, u32x2{pack_bf16x2(x[0], x[1]), pack_bf16x2(x[2], x[3])});
            }
        } else if (!fin && !carry) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const f32x4 x = epi_tile_read(tb, i, lane);
                if (2 * i < rows) global_store_f32x4((float*)(ap + i * acc_step), x);
            }
        } else {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                f32x4 x = epi_tile_read(tb, i, lane);
                if (2 * i < rows) {
                    const f32x4 c = global_load_f32x4((const float*)(ap + i * acc_step));
                    x[0] += c[0]; x[1] += c[1]; x[2] += c[2]; x[3] += c[3];
                    if (fin) global_store_b64(op + i * out_step, u32x2{pack_bf16x2(x[0], x[1]), pack_bf16x2(x[2], x[3])});
                    else global_store_f32x4((float*)(ap + i * acc_step), x);
                }
            }
        }
    }
}

template <bool HAS_META, bool DS = false>
LWM_DEVICE void attn_bwd_dkdv4_body(const AttnParams& p) {
    static_assert(!(HAS_META && DS), "the hand-over has no key meta");
#ifdef LWM_PROF
    // (dump slots 11..13: entry -> last store issued, entry -> first step of the walk, entry -> first store of the epilogue)
    const unsigned long long d4_entry = __builtin_amdgcn_s_memtime();
    unsigned long long d4_head = 0, d4_epi = 0;
#endif
    const lds_t lds = dyn_lds();
    const int tid = thread_idx();
    const int wave = wave_uniform(tid >> 6), lane = tid & 63, l15 = lane & 15, g4 = lane >> 4;

    // ---- block -> (key block, head, batch): all key blocks of one (b,h) on one XCD, longest walks first
    const int nkb = (p.Sk + kD4BK - 1) / kD4BK;
    const int HB = p.H * p.B;
    int lin = block_idx_x(), kbi, hb;
    if ((HB & 7) == 0) {
        int xcd = lin & 7, i = lin >> 3;
        hb = xcd + 8 * (i / nkb);
        kbi = i % nkb;
    } else {
        hb = lin / nkb;
        kbi = lin % nkb;
    }
    const int b = hb / p.H, h = hb % p.H;
    const bf16_t* qb = p.q + (int64_t)b * p.q_sb + (int64_t)h * p.q_sh;
    const bf16_t* kb = p.k + (int64_t)b * p.k_sb + (int64_t)h * p.k_sh;
    const bf16_t* vb = p.v + (int64_t)b * p.v_sb + (int64_t)h * p.v_sh;
    const bf16_t* dob = p.dout + (int64_t)b * p.do_sb + (int64_t)h * p.do_sh;

    // ---- this lane's two keys (row 16 kh + c of the wave's 32): fragments straight into the accumulator file (a row
    // past Sk re-reads the last row: its results are never stored)
    int k_row[2], kr[2];
    bool k_ok[2];
#pragma unroll
    for (int kh = 0; kh < 2; ++kh) {
        k_row[kh] = kbi * kD4BK + wave * 32 + 16 * kh + l15;
        k_ok[kh] = k_row[kh] < p.Sk;
        kr[kh] = k_ok[kh] ? k_row[kh] : p.Sk - 1;
    }
    bf16x8 kf[8], vf[8];        // [4 kh + s]: d step s of 32
#pragma unroll
    for (int i = 0; i < 8; ++i) kf[i] = f4_load_agpr(kb + (int64_t)kr[i >> 2] * p.k_ss + 32 * (i & 3) + 8 * g4);
#pragma unroll
    for (int i = 0; i < 8; ++i) vf[i] = f4_load_agpr(vb + (int64_t)kr[i >> 2] * p.v_ss + 32 * (i & 3) + 8 * g4);
    const PosMap qm = q_map(p);
    const PosTab qt_ = load_postab(qm);                           // (register copies of the tables: prologue only)
    const int64_t k_base = pos_base(load_postab(k_map(p)), kbi * kD4BK);       // position of key row r of this workgroup = k_base + r
    int32_t kseg[2] = {0, 0};
    if (HAS_META) {
#pragma unroll
        for (int kh = 0; kh < 2; ++kh) {
            kseg[kh] = kSegInvalid;
            if (k_ok[kh]) {
                const bool valid = p.key_valid ? (p.key_valid[(int64_t)b * p.Sk + k_row[kh]] != 0) : true;
                if (valid) kseg[kh] = p.seg_k ? p.seg_k[(int64_t)b * p.Sk + k_row[kh]] : 0;
            }
        }
    }

    // ---- step range of the walk (steps of 64 queries; causal: skip steps wholly before this key block)
    int nst = (p.Sq + kD4BQ - 1) / kD4BQ;
    int st0 = 0;
    if (p.causal) st0 = tiles_below(qt_, kD4BQ, nst, k_base + (int64_t)kbi * kD4BK - 1);   // steps wholly before the block's key 0
    if (HAS_META && p.segb_q && p.segb_k && st0 < nst) {     // packed sequences: skip other documents' query steps
        const int nbq = (p.Sq + 31) >> 5, nbk = (p.Sk + 31) >> 5;
        int smin, smax, lo, hi2;
        seg_own_range(p.segb_k + (int64_t)b * nbk * 2, nbk, kbi * (kD4BK / 32), kD4BK / 32, smin, smax);
        seg_narrow<kD4Threads>(p.segb_q + (int64_t)b * nbq * 2, nbq, kD4BQ / 32, st0, nst, smin, smax, lds + kD4OffStat, tid, lo, hi2);
        st0 = lo;
        nst = hi2;
    }
    const int n = nst > st0 ? nst - st0 : 0;       // steps of the walk; walk index i -> step nst - 1 - i (descending:
                                                   // the key blocks resident on an XCD read the same tile at the same time)

    f32x4 dk[16], dv[16];      // [2 db + kh]: rows 16 db + 4g + 0..3 of dK^T / dV^T for key 16 kh + c; defined by the first
                               // products of the walk (d4_y<.., INIT>), or zero when there is no walk
    if (n == 0)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            dk[i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            dv[i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        }
    if (n == 0) {       // (no walk: the fragments are unused, their loads are not left in flight)
        f4_load_agpr_wait8(kf);
        f4_load_agpr_wait8(vf);
    }

    if (n > 0) {
        D4Ctx cx;
        cx.c = p.scale * kLog2e;
#pragma unroll
        for (int s = 0; s < 4; ++s) cx.qa[s] = lds + q4_tile_off(l15, 4 * s + g4);
#pragma unroll
        for (int db = 0; db < 8; ++db) {
            // lane t of a 16-lane group addresses query 4g + (t>>2), d 16 db + 4 (t&3): four queries x 16 d per group
            cx.tlo[db] = lds + q4_tile_off(4 * g4 + (l15 >> 2), 2 * db + ((l15 & 3) >> 1)) + (l15 & 1) * 8;
            cx.plo[db] = cx.tlo[db];
        }
        cx.stat = lds + kD4OffStat + 16 * g4;

        const int64_t q_step_bytes = (int64_t)kD4BQ * p.q_ss * 2, do_step_bytes = (int64_t)kD4BQ * p.do_ss * 2;
        uint32_t vq[4], vdo[4];
        d4_stage_offsets(p, wave, lane, 0, vq, vdo);      // full steps: nothing is clamped
        // The row statistics travel like the tiles: ONE LDS-DMA dword instruction moves the 64 floats of a step's nl2 row
        // (wave 0), of its nd row (wave 1) and -- with key meta -- of its query segment ids (wave 2), first thing in the
        // step, so that the counted wait at the bottom (all but the 8 tile pieces of the step) covers them.
        const int64_t Sqp = bwd_stat_pad(p.Sq);
        const char* stat_src = (const char*)(p.delta + bwd_stat_row((int64_t)b * p.H + h, Sqp) + (wave == 1 ? Sqp : 0));
        bool stat_on = wave < 2;
        if (HAS_META && wave == 2 && p.seg_q) {
            stat_src = (const char*)(p.seg_q + (int64_t)b * p.Sq);
            stat_on = true;
        }
        const lds_t stat_dst = lds + kD4OffStat + (uint32_t)(wave < 3 ? wave : 0) * kD4BQ * 4;
        const uint32_t vstat = (uint32_t)lane * 4;
        if (HAS_META && !p.seg_q)                          // no query segments: every slot's ids read as 0
            for (int sl = 0; sl < kD4Slots; ++sl)
                if (tid < kD4BQ) lds_write_i32(lds + kD4OffStat + sl * kD4StatBytes + 2 * kD4BQ * 4 + tid * 4, 0);
        // staging of walk index i from the slow path (prologue; the ragged top step has its own offsets, and its
        // segment ids stop at Sq: the statistics rows are padded, the caller's ids are not)
        auto stage_step = [&](int i) {
            const int st = nst - 1 - i;
            const lds_t dst = lds + (i & 3) * kD4SlotBytes + (uint32_t)wave * 1024;
            const char* qs = (const char*)qb + st * q_step_bytes;
            const char* ds = (const char*)dob + st * do_step_bytes;
            if (stat_on) {
                int row = st * kD4BQ + lane;
                if (HAS_META && wave == 2) row = row < p.Sq ? row : p.Sq - 1;
                glds_load_b32(stat_src + (int64_t)row * 4, stat_dst + (i & 3) * kD4StatBytes);
            }
            if (st * kD4BQ + kD4BQ > p.Sq) {
                uint32_t v2[4], d2[4];
                d4_stage_offsets(p, wave, lane, st, v2, d2);
                f4_dma<4>(v2, qs, dst);
                f4_dma<4>(d2, ds, dst + kD4TileBytes);
            } else {
                f4_dma<4>(vq, qs, dst);
                f4_dma<4>(vdo, ds, dst + kD4TileBytes);
            }
        };

        // ---- prologue: steps 0 and 1 in flight; the K / V fragments are waited for together with them (one memory
        // latency per workgroup, not two in a row: 2-3 us of the ~50 us a 32-step walk of a ring shard takes)
        stage_step(0);
        if (n > 1) stage_step(1);
        f4_load_agpr_wait8(kf);      // vmcnt(0): everything requested so far
        f4_load_agpr_wait8(vf);
        block_sync();

        // A unit needs the mask code when its first query lies before the wave's last key (or keys can be masked for
        // another reason than causality).  Units are named by the row of their first query inside the q block,
        // ub = 64 * step + 32 * half (steps descend, the halves of a step ascend); everything is clamped to 32 bits once.
        auto clamp32 = [](int64_t x) -> int { return x > (1 << 30) ? (1 << 30) : (x < -(1 << 30) ? -(1 << 30) : (int)x); };
        // positions relative to q_start; a unit's first query (row ub of the q block) sits at rel_pos(qm, ub)
        int k_rel[2];                                                                    // this lane's keys
#pragma unroll
        for (int kh = 0; kh < 2; ++kh) k_rel[kh] = clamp32(k_base + k_row[kh] - p.q_start) - 4 * g4;
        PosCursor qc = cursor_begin(qt_);
        auto q_rel_of = [&](int ub) -> int {             // (the walk descends: a compare while the unit is inside the piece)
            cursor_seek(qm, qc, ub);
            return clamp32(qc.base + ub - p.q_start);
        };
        // positions ascend with the row: the units that begin before the wave's last key -- the ones that need the mask
        // code -- are the first mask_end rows of the q block (one compare per unit in the walk)
        const int mask_end = p.causal ? 32 * tiles_reaching(qt_, 32, (p.Sq + 31) / 32, k_base + (int64_t)kbi * kD4BK + wave * 32 + 31 - 1) : 0;
        auto needs_causal = [&](int ub) -> bool { return ub < mask_end; };
        // the wave's 32 keys all valid and of one segment?  (then a step whose 64 queries carry it needs no segment test)
        const int32_t own_seg = wave_uniform(kseg[0]);
        const bool own_uniform = HAS_META && !wave_any(kseg[0] != own_seg || kseg[1] != own_seg || own_seg == kSegInvalid);
        auto rel_of = [&](int ub, int (&rel)[2]) {
            if (!p.causal) {
                rel[0] = rel[1] = -64;
                return;
            }
            const int qr = q_rel_of(ub);
#pragma unroll
            for (int kh = 0; kh < 2; ++kh) {
                const int64_t d = (int64_t)k_rel[kh] - qr;
                rel[kh] = d > 64 ? 64 : (d < -64 ? -64 : (int)d);
            }
        };

        D4Regs rg;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            rg.s[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            rg.dp[0][t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            rg.dp[1][t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            rg.t[r] = 0.0f;
            rg.ds[r] = 0.0f;
        }
#pragma unroll
        for (int r = 0; r < 8; ++r) rg.nl[r] = 0.0f;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            rg.pb[t] = zero_bf16x8();
            rg.dsb[t] = zero_bf16x8();
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) rg.fr[j] = zero_bf16x8();
        D4Dma dm = {};
        // hand-over: the tile of the walk's first step (the LAST step of the wave's row), see d4_ds_stores
        D4Ds sw = {};
        if (DS) {
            const int64_t e = ds_diag(p.causal, p.q_start, p.k_start);
            const int64_t tile = ((int64_t)hb * ds_steps_before(e, nst, nkb) + ds_steps_before(e, nst, kbi)) * 4 + (int64_t)wave * n + (n - 1);
            sw.p = ds_uniform_ptr(p.ds_ws + (tile + 1) * kDsTileBytes);
            sw.v = (uint32_t)lane * 16;
        }
        // the first unit's fragments and -delta (every later unit finds them requested by the unit before it)
#pragma unroll
        for (int j = 0; j < kD4Ahead; ++j) rg.fr[j] = d4_frag<0>(cx, j);
#pragma unroll
        for (int qh = 0; qh < 2; ++qh) rg.ndl[qh] = lds_read_f32x4(cx.stat + kD4BQ * 4 + 16 * qh * 4);

        // Step i of the walk.  Its tiles are in slot i & 3; the address registers in cx point there and move on to the slot
        // of step i+1 (wrapping) as the step ends: the row-fragment addresses behind the last X phase (the Y phase after
        // it already requests the next step's first fragments: that step's tiles became visible at the barrier before
        // this one), the others behind the barrier.  Top: the statistics piece and, inside the first X phase, the
        // LDS-DMA pieces of step i+2 -> slot (i+2) & 3 (last read by the lagging products at the head of step i-1).
        // Bottom: this wave's pieces have landed (they were issued >= 2000 cycles ago), one barrier.
#define LWM_D4_MASK(HALF_, HAS_PREV_, ub_)                                                                          \
    do {                                                                                                            \
        /* (the wait states sit in ONE statement on every path that needs them: with two, hipcc merges the tuples */ \
        /* of the two paths by copies placed right behind the last MFMA)                                         */ \
        if (!(HAS_PREV_)) d4_settle_t(rg.s);     /* no MFMA stands between the S chains and their first reader */    \
        if ((HAS_META && !uni_) || needs_causal(ub_)) {                                                             \
            if (HAS_PREV_) d4_settle_t(rg.s);                                                                       \
            int rel_[2];                                                                                            \
            rel_of(ub_, rel_);                                                                                      \
            if (HAS_META && !uni_) d4_mask<HALF_, HAS_META>(cx, rg.s, rel_, kseg);                                  \
            else d4_mask<HALF_, false>(cx, rg.s, rel_, kseg);                                                       \
        }                                                                                                           \
    } while (0)
        // (-DLWM_PROF builds, scripts/micro/attn_bench with LWM_PROF_DUMP=1: s_memtime laps of the pipelined steps of the
        // longest key block of head 0 -- 0 X(0), 1 mask, 2 Y(0), 3 X(1), 4 mask, 5 Y(1), 6 counted wait, 7 barrier,
        // 8 address registers; 9 steps, 10 total.  LWM_PROF = 1 stamps only 5..8: a stamp drains lgkmcnt, i.e. the
        // fragments requested across a phase boundary)
#ifdef LWM_PROF
        unsigned long long d4p[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, d4t = __builtin_amdgcn_s_memtime();
        const unsigned long long d4t0 = d4t;
        d4_head = d4t - d4_entry;
#define D4_LAP(slot)                                                  \
    do {                                                              \
        const unsigned long long now_ = __builtin_amdgcn_s_memtime(); \
        d4p[slot] += now_ - d4t;                                      \
        d4t = now_;                                                   \
    } while (0)
#if LWM_PROF > 1
#define D4_LAP2(slot) D4_LAP(slot)
#else
#define D4_LAP2(slot)
#endif
#else
#define D4_LAP(slot)
#define D4_LAP2(slot)
#endif
        // `ub` = first row of the running step, `src` pointers = the step two ahead (they walk down with the steps)
        int ub = (nst - 1) * kD4BQ;
        const char* q_src2 = (const char*)qb + (int64_t)(nst - 3) * q_step_bytes;
        const char* do_src2 = (const char*)dob + (int64_t)(nst - 3) * do_step_bytes;
        const char* st_src2 = stat_src + (int64_t)(nst - 3) * kD4BQ * 4;
#define LWM_D4_STEP(i, FIRST, PIPE)                                                                                 \
    do {                                                                                                            \
        if (PIPE) {                                                                                                 \
            if (stat_on) d4_dma_b32(vstat, st_src2, stat_dst + (((i) + 2) & 3) * kD4StatBytes);                     \
            dm.q_src = q_src2;                                                                                      \
            dm.do_src = do_src2;                                                                                    \
            dm.dst = lds + (((i) + 2) & 3) * kD4SlotBytes + (uint32_t)wave * 1024;                                  \
            q_src2 -= q_step_bytes;                                                                                 \
            do_src2 -= do_step_bytes;                                                                               \
            st_src2 -= kD4BQ * 4;                                                                                   \
        }                                                                                                           \
        const uint32_t d_ = (((i) & 3) == 3) ? (uint32_t)(-3 * kD4SlotBytes) : (uint32_t)kD4SlotBytes;             \
        const uint32_t e_ = (((i) & 3) == 3) ? (uint32_t)(-3 * kD4StatBytes) : (uint32_t)kD4StatBytes;             \
        const int32_t segw_ = HAS_META ? seg_step_word(cx.stat - 16 * g4 + 2 * kD4BQ * 4, lane) : 0;                \
        d4_x<0, !(FIRST), PIPE, DS>(cx, rg, kf, vf, vq, vdo, dm, sw);                                                       \
        const bool uni_ = HAS_META && seg_step_uniform(segw_, own_uniform, own_seg);                                \
        D4_LAP2(0);                                                                                                 \
        LWM_D4_MASK(0, !(FIRST), ub);                                                                               \
        D4_LAP2(1);                                                                                                 \
        d4_y<0, !(FIRST), true, false>(cx, rg, dk, dv, cx.stat);                                                    \
        D4_LAP2(2);                                                                                                 \
        d4_x<1, true, false, DS>(cx, rg, kf, vf, vq, vdo, dm, sw);                                                  \
        for (int s_ = 0; s_ < 4; ++s_) cx.qa[s_] += d_;                                                             \
        D4_LAP2(3);                                                                                                 \
        LWM_D4_MASK(1, true, ub + 32);                                                                              \
        D4_LAP2(4);                                                                                                 \
        d4_y<1, true, true, FIRST>(cx, rg, dk, dv, cx.stat + e_);                                                   \
        D4_LAP(5);                                                                                                  \
        ub -= kD4BQ;                                                                                                \
        /* wherever control flow merges behind a step (loop entry, loop exit, the short-walk branch) hipcc may */  \
        /* reconcile the accumulator tuples of the two paths by copies: they must find the last MFMAs retired  */  \
        if ((FIRST) || !(PIPE)) d4_settle_acc(dk, dv);                                                              \
        /* hand-over: the step's four dS stores are its youngest vector-memory operations (W = gap 63: behind   */  \
        /* the last LDS-DMA piece; the walk's first step has only two) and stay in flight; everything older --  */  \
        /* the pieces -- has retired                                                                            */  \
        if (DS) {                                                                                                   \
            if (FIRST) wait_vmem_le<2>();                                                                           \
            else wait_vmem_le<4>();                                                                                 \
            sw.p -= kDsTileBytes;                                                                                   \
        } else {                                                                                                    \
            glds_wait_all();                                                                                        \
        }                                                                                                           \
        D4_LAP(6);                                                                                                  \
        block_sync_lds();                                                                                           \
        D4_LAP(7);                                                                                                  \
        for (int db_ = 0; db_ < 8; ++db_) {                                                                         \
            cx.plo[db_] = cx.tlo[db_];                                                                              \
            cx.tlo[db_] += d_;                                                                                      \
        }                                                                                                           \
        cx.stat += e_;                                                                                              \
        D4_LAP(8);                                                                                                  \
    } while (0)

        int i = 0;
        if (n > 2) {
            LWM_D4_STEP(0, true, true);
#ifdef LWM_PROF
            for (int j = 0; j < 12; ++j) d4p[j] = 0;
            d4t = __builtin_amdgcn_s_memtime();
#endif
            for (i = 1; i + 2 < n; ++i) {
                LWM_D4_STEP(i, false, true);
#ifdef LWM_PROF
                d4p[9] += 1;
#endif
            }
#ifdef LWM_PROF
            if (!HAS_META && hb == 0 && kbi == 0 && lane == 0 && p.out_acc) {
                d4p[10] = __builtin_amdgcn_s_memtime() - d4t0;
                for (int j = 0; j < 11; ++j) ((unsigned long long*)p.out_acc)[wave * 16 + j] = d4p[j];
            }
#endif
            for (; i < n; ++i) LWM_D4_STEP(i, false, false);
        } else {
            LWM_D4_STEP(0, true, false);
            if (n > 1) LWM_D4_STEP(1, false, false);
        }
#undef LWM_D4_STEP
#undef D4_LAP
#undef D4_LAP2
#undef LWM_D4_MASK
        // the last unit's products: its tiles are the second half of the PREVIOUS slot now (the registers moved on)
        d4_drain<1, DS>(cx, rg, dk, dv, sw);
        d4_settle_acc(dk, dv);      // before the paths merge (hipcc reconciles the tuples by copies at the merge)
    }

    // ---- epilogue: scale, merge with the ring carries, store
    d4_settle_acc(dk, dv);
#ifdef LWM_PROF
    d4_epi = __builtin_amdgcn_s_memtime() - d4_entry;
#endif
    // The tiles leave as whole rows (attn_common.h, "epilogue staging"): the walk is over for every wave behind the
    // barrier, so the tile slots are free; a wave passes dK^T, then dV^T through its own 16 KiB of them.
    if (DS) glds_wait_all();      // (the last dS stores: nothing of the walk is in flight behind this point)
    block_sync_lds();
    d4_store_tiles(p, lds + (uint32_t)wave * kEpiTileBytes, dk, dv, b, h, kbi * kD4BK + wave * 32, lane);
#ifdef LWM_PROF
    if (!HAS_META && hb == 0 && kbi == 0 && lane == 0 && p.out_acc) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // (the stores have left)
        unsigned long long* o_ = (unsigned long long*)p.out_acc + wave * 16;
        o_[11] = __builtin_amdgcn_s_memtime() - d4_entry;
        o_[12] = d4_head;
        o_[13] = d4_epi;
    }
#endif
}


LWM_KERNEL(kD4Threads) void attn_bwd_dkdv4_kernel(AttnParams p) { attn_bwd_dkdv4_body<false>(p); }
LWM_KERNEL(kD4Threads) void attn_bwd_dkdv4_meta_kernel(AttnParams p) { attn_bwd_dkdv4_body<true>(p); }
LWM_KERNEL(kD4Threads) void attn_bwd_dkdv4_ds_kernel(AttnParams p) { attn_bwd_dkdv4_body<false, true>(p); }


// ====================================================================================================== dQ
// The dQ kernel of the two-kernel backward in the same structure.  Replaces the dq part of the custom VJP (see the
// file header): p from the saved LSE, dp = do v^T, ds = p * (dp - delta), dq += ds k * scale.  Same contract,
// operands, masks, carries and segment-block hints as the dK/dV kernel above.
//
// Matrix instruction, operand maps and tile image: the file header.
//
// Workgroup = 4 waves = 128 queries; a wave owns 32 query rows = two halves qh of 16: their Q and dO fragments (B
// operands, 32 + 32 registers) and the f32 dQ^T accumulator (64) live in the accumulator file.  Everything is computed
// transposed, as in the forward: a lane owns query column c of each half, so the row statistics are two scalars per
// lane and half, and -delta, the initial value of the dP chains, is ONE constant tuple per half for the whole launch
// (no per-unit statistics traffic at all).  K / V arrive by LDS-DMA in steps of 64 keys through the same ring of four
// 32-KiB slots [K tile | V tile]; a unit = 32 keys = two halves kh of 16:
//
//   phase   matrix pipe                                                     vector pipe (same wave)
//   X(u)    S^T(u)[kh][qh] = K(u) Q^T and dP'^T(u) = V(u) dO^T - delta:     the vector work of unit u-1 continues
//           16 row fragments (ds_read_b128), each feeds the two qh: 32
//   Y(u)    dQ^T[db < 8][qh] += K(u-1)^T(db) dS^T(u-1)[qh]: 8 transposed    t = S c - lse2, p = exp2(t), dS = p dP' -> bf16
//           fragments (2 x ds_read_b64_tr_b16), each feeds the two qh: 16
//
// The B operand of Y is the packed dS of the subtiles (kh = 0, qh) | (kh = 1, qh) as the MFMAs left them, which puts
// k-group g at keys {4g .. 4g+3, 16+4g .. 16+4g+3}: the transposed read takes its first four keys from rows 4g .., its
// second four from rows 16+4g ...  S and dP' have two sets of register tiles (by unit parity): the 56 VALU of a unit
// spread over the 48 gaps of Y(u) and X(u+1).  With key meta (segment ids, padded keys, a ragged last tile) the 64 meta
// words of a step are staged through LDS by the threads themselves, as the forward does.
//
// LDS map: slot 0..3 = [K tile 64 rows | V tile 64 rows] (16 KiB each) | key meta 0..3 (64 words each)
constexpr int kQ4BQ = 128;      // queries per workgroup
constexpr int kQ4BK = 64;       // keys per step (two units of 32)
constexpr int kQ4OffMeta = kD4Slots * kD4SlotBytes;
constexpr int kQ4LdsBytes = kQ4OffMeta + kD4Slots * kQ4BK * 4;


// G = 0..15 = the gaps of Y(u), G = 16..47 = the gaps of X(u+1) (gap = behind that MFMA).  An MFMA holds the vector
// issue for 8 of its 16 cycles, so a gap takes two plain VALU or one v_exp_f32 beside its LDS read.  F >= 3 (three
// MFMAs between the end of the S chains and their first reader); E behind F, M behind E, D behind its two M; the
// products of Y(u) read the OLD dS words to their last MFMA: D >= 16; everything done by G = 45.
struct Q4Sched {
    int F[16], E[16], M[16], D[8];
};
constexpr bool q4_sched_ok(const Q4Sched& c) {
    int load[48] = {};
    for (int e = 0; e < 16; ++e) {
        if (c.F[e] < 3 || c.E[e] <= c.F[e] || c.M[e] <= c.E[e] || c.M[e] > 45) return false;
        load[c.F[e]] += 1;
        load[c.E[e]] += 2;
        load[c.M[e]] += 1;
    }
    for (int i = 0; i < 8; ++i) {
        if (c.D[i] < 16 || c.D[i] > 45 || c.D[i] <= c.M[2 * i] || c.D[i] <= c.M[2 * i + 1]) return false;
        load[c.D[i]] += 1;
    }
    for (int g = 0; g < 48; ++g)
        if (load[g] > 2) return false;      // (in units of a plain VALU's issue; an exp counts two)
    return true;
}
constexpr Q4Sched kQ4Sched = {
    /* F */ {3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 13, 14, 14, 15, 15},
    /* E */ {16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31},
    /* M */ {32, 32, 33, 33, 34, 34, 35, 35, 36, 36, 37, 37, 38, 38, 39, 39},
    /* D */ {40, 40, 41, 41, 42, 42, 43, 43}};
static_assert(q4_sched_ok(kQ4Sched), "filler schedule violates a dependency or the issue budget of a gap");

struct Q4Ctx {
    uint32_t ka[4];             // K row-fragment addresses (d step s of 32), rows 0..15 of the CURRENT step's K tile
    uint32_t tlo[8];            // K transposed-fragment addresses (d block of 16), rows 4g.. of the current step's K tile
    uint32_t plo[8];            // the same in the PREVIOUS step's slot
    uint32_t meta;              // this step's key meta + 16 * g
    float c, nl[2];             // scale * log2(e); -lse * log2(e) of this lane's two queries (-inf: p = 0)
};

// element e of the vector work = (qh = e >> 3, kh = (e >> 2) & 1, j = e & 3): score tile e >> 2 = 2 qh + kh, register j;
// the dS words of a query half are then four consecutive packed registers, ready as the B operand of Y
struct Q4Regs {
    f32x4 s[2][4], dp[2][4];    // S^T / dP'^T tiles by unit parity (MFMA results, read-only for the vector pipe)
    f32x4 ndl[2];               // -delta of this lane's queries in every element: the C operand that starts each dP chain
    float t[16], ds[16];
    bf16x8 dsb[2];
    uint32_t dw[8];
    bf16x8 fr[8];
};


// fragment f of a unit (24 per unit, each feeds the MFMAs of the two query halves; 24.. = the first fragments of the
// unit that follows):
//   0..15   phase X: pair f>>1 = (d step s = f>>2, key half kh = (f>>1)&1); even = K row fragment (S^T), odd = V (dP'^T)
//   16..23  phase Y: K^T of the PREVIOUS unit, d block f-16: keys 4g.. (first read) and 16+4g.. (second read)
template <int HALF>
LWM_DEVICE bf16x8 q4_frag(const Q4Ctx& cx, int f) {
    if (f >= 24) {
        const int g = f - 24;
        return lds_read_b128(cx.ka[g >> 2] + (g & 1) * kD4TileBytes + ((g >> 1) & 1) * 16 * kRowBytes + (HALF == 0 ? 32 * kRowBytes : 0));
    }
    if (f < 16) return lds_read_b128(cx.ka[f >> 2] + (f & 1) * kD4TileBytes + ((f >> 1) & 1) * 16 * kRowBytes + HALF * 32 * kRowBytes);
    const int db = f - 16;
    const uint32_t a = (HALF == 0 ? cx.plo[db] : cx.tlo[db]) + (HALF == 0 ? 32 * kRowBytes : 0);
    bf16x4 lo = lds_read_tr16(a);
    bf16x4 up = lds_read_tr16(a + 16 * kRowBytes);
    bf16x8 o;
    o[0] = lo[0]; o[1] = lo[1]; o[2] = lo[2]; o[3] = lo[3];
    o[4] = up[0]; o[5] = up[1]; o[6] = up[2]; o[7] = up[3];
    return o;
}

// the vector work scheduled in gap G for the unit of parity PAR
template <int G, int PAR>
LWM_DEVICE void q4_fillers(const Q4Ctx& cx, Q4Regs& rg) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        if (kQ4Sched.F[e] == G) rg.t[e] = f4_fma(rg.s[PAR][e >> 2][e & 3], cx.c, cx.nl[e >> 3]);
        if (kQ4Sched.E[e] == G) rg.t[e] = f4_exp2(rg.t[e]);
        if (kQ4Sched.M[e] == G) rg.ds[e] = d4_mul(rg.t[e], rg.dp[PAR][e >> 2][e & 3]);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i)
        if (kQ4Sched.D[i] == G) rg.dw[i] = f4_cvt_pk(rg.ds[2 * i], rg.ds[2 * i + 1]);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        int ld = 0;
        for (int i = 4 * h; i < 4 * h + 4; ++i) ld = kQ4Sched.D[i] > ld ? kQ4Sched.D[i] : ld;
        if (ld == G) rg.dsb[h] = __builtin_bit_cast(bf16x8, u32x4{rg.dw[4 * h], rg.dw[4 * h + 1], rg.dw[4 * h + 2], rg.dw[4 * h + 3]});
    }
}
// Every MFMA index below is a template parameter (the phases are recursions, not loops): fragment, tile and filler
// selection must be constants, or the register arrays they index go to scratch.
//
// Phase X of unit u (parity HALF): 32 MFMAs, fragment m>>1 (pairs K | V requested together every fourth gap, the pair's
// YOUNGER fragment consumed first: one wait per four MFMAs), query half m&1; fillers: gaps 16..47 of unit u-1.
template <int HALF, bool HAS_PREV, bool DMA, int M = 0>
LWM_DEVICE void q4_x(const Q4Ctx& cx, Q4Regs& rg, const bf16x8 (&qf)[8], const bf16x8 (&dof)[8], const uint32_t (&vk)[4],
                     const uint32_t (&vv)[4], const D4Dma& dm) {
    if constexpr (M < 32) {
        if constexpr ((M & 3) == 0) {
            constexpr int f0 = (M >> 1) + kD4Ahead;
            rg.fr[f0 & 7] = q4_frag<HALF>(cx, f0);
            sched_fence();      // (the pair in this order: the wait for the younger fragment then covers both)
            rg.fr[(f0 + 1) & 7] = q4_frag<HALF>(cx, f0 + 1);
        }
        sched_fence();
        {
            constexpr int f = (M >> 1) ^ 1, qh = M & 1;      // even = K (S^T), odd = V (dP'^T)
            constexpr int s = f >> 2, t = 2 * qh + ((f >> 1) & 1);
            if constexpr ((f & 1) == 0) {
                if constexpr (s == 0) q4_mfma_first(rg.s[HALF][t], rg.fr[f & 7], qf[4 * qh]);
                else q4_mfma(rg.s[HALF][t], rg.fr[f & 7], qf[4 * qh + s]);
            } else {
                if constexpr (s == 0) q4_mfma_c_first(rg.dp[HALF][t], rg.fr[f & 7], dof[4 * qh], rg.ndl[qh]);
                else q4_mfma(rg.dp[HALF][t], rg.fr[f & 7], dof[4 * qh + s]);
            }
        }
        if constexpr (DMA && (M & 3) == 3) {
            constexpr int i = M >> 2, j = i >> 1;
            if constexpr ((i & 1) == 0) f4_dma1(vk[j], dm.q_src, dm.dst + 4096 * j);
            else f4_dma1(vv[j], dm.do_src, dm.dst + kD4TileBytes + 4096 * j);
        }
        if constexpr (HAS_PREV) q4_fillers<16 + M, HALF ^ 1>(cx, rg);
        sched_fence();
        q4_x<HALF, HAS_PREV, DMA, M + 1>(cx, rg, qf, dof, vk, vv, dm);
    }
}

// masks of a unit on its transposed scores (lwm/llama.py:572-592): key row 16 kh + 4g + j of the unit is visible to the
// lane's query of half qh iff it is not after it (rel[qh] = query position - position of the unit's key 0 - 4g, clamped)
// and, with key meta, carries the query's segment (kSegInvalid: a padded / out-of-range key)
template <int HALF, bool HAS_META>
LWM_DEVICE void q4_mask(const Q4Ctx& cx, f32x4 (&s)[4], const int (&rel)[2], const int32_t (&seg_q)[2]) {
#pragma unroll
    for (int kh = 0; kh < 2; ++kh) {
        u32x4 sg = {0u, 0u, 0u, 0u};
        if (HAS_META) sg = lds_read_u32x4(cx.meta + HALF * 32 * 4 + 16 * kh * 4);
#pragma unroll
        for (int qh = 0; qh < 2; ++qh)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool vis = (!HAS_META || (int32_t)sg[j] == seg_q[qh]) && (16 * kh + j <= rel[qh]);
                s[2 * qh + kh][j] = vis ? s[2 * qh + kh][j] : -INFINITY;
            }
    }
}

// Phase Y of unit u: dQ^T += K(u-1)^T dS^T(u-1), 16 MFMAs (d block j>>1, query half j&1)  ||  gaps 0..15 of unit u.
// INIT: the first products of the walk.
template <int HALF, bool HAS_PREV, bool INIT, int J = 0>
LWM_DEVICE void q4_y(const Q4Ctx& cx, Q4Regs& rg, f32x4 (&dq)[16]) {
    if constexpr (J < 16) {
        if constexpr ((J & 3) == 0) {
            constexpr int f0 = 16 + (J >> 1) + kD4Ahead;
            rg.fr[f0 & 7] = q4_frag<HALF>(cx, f0);
            sched_fence();      // (the pair in this order: the wait for the younger fragment then covers both)
            rg.fr[(f0 + 1) & 7] = q4_frag<HALF>(cx, f0 + 1);
        }
        sched_fence();
        if constexpr (HAS_PREV) {
            constexpr int db = (J >> 1) ^ 1, qh = J & 1;      // (pairs: the younger fragment first)
            if constexpr (INIT) q4_mfma_o_first(dq[2 * db + qh], rg.fr[(16 + db) & 7], rg.dsb[qh]);
            else q4_mfma_o(dq[2 * db + qh], rg.fr[(16 + db) & 7], rg.dsb[qh]);
        }
        q4_fillers<J, HALF>(cx, rg);
        sched_fence();
        q4_y<HALF, HAS_PREV, INIT, J + 1>(cx, rg, dq);
    }
}

template <int PAR, int G = 16>
LWM_DEVICE void q4_drain_fill(const Q4Ctx& cx, Q4Regs& rg) {
    if constexpr (G < 48) {
        q4_fillers<G, PAR>(cx, rg);
        q4_drain_fill<PAR, G + 1>(cx, rg);
    }
}
template <int J = 0>
LWM_DEVICE void q4_drain_mfma(Q4Regs& rg, f32x4 (&dq)[16]) {
    if constexpr (J < 16) {
        q4_mfma_o(dq[J], rg.fr[J >> 1], rg.dsb[J & 1]);
        q4_drain_mfma<J + 1>(rg, dq);
    }
}
template <int PAR>
LWM_DEVICE void q4_drain(const Q4Ctx& cx, Q4Regs& rg, f32x4 (&dq)[16]) {
    q4_drain_fill<PAR>(cx, rg);
#pragma unroll
    for (int j = 0; j < 8; ++j) rg.fr[j] = q4_frag<0>(cx, 16 + j);
    sched_fence();
    q4_drain_mfma(rg, dq);
}

// per-lane byte offsets of the wave's four pieces of a 64-row K / V tile, rows clamped to Sk-1 (rows past Sk are masked
// through the key meta); lane l writes physical slot l&15 of its row, so it fetches logical slot (l&15) ^ q4_swz(row)
LWM_DEVICE void q4_stage_offsets(const AttnParams& p, int wave, int lane, int st, uint32_t (&vk)[4], uint32_t (&vv)[4]) {
    const int slot = lane & 15;
    for (int j = 0; j < 4; ++j) {
        const int row = 4 * (wave + 4 * j) + (lane >> 4);
        int krow = st * kQ4BK + row;
        krow = krow < p.Sk ? krow : p.Sk - 1;
        const int rel = krow - st * kQ4BK;
        const int col = (slot ^ q4_swz(row)) << 3;
        vk[j] = (uint32_t)(((int64_t)rel * p.k_ss + col) * 2);
        vv[j] = (uint32_t)(((int64_t)rel * p.v_ss + col) * 2);
    }
}

// the stores of query half QH: row q_row of (b, h), 4 consecutive d per d block (what the stores share is read once and
// the three cases are three loops: left inside one loop, hipcc re-read carry_in / final_out behind a wait per store --
// see d4_store_tiles)
template <int QH>
LWM_DEVICE void q4_store(const AttnParams& p, const f32x4 (&dq)[16], int b, int h, int q_row, int g4) {
    const bool carry = p.carry_in != 0, fin = p.final_out != 0;
    const float sc = p.scale;
    bf16_t* const op = p.dq + (int64_t)b * p.dq_sb + (int64_t)q_row * p.dq_ss + (int64_t)h * p.dq_sh + 4 * g4;
    float* const ap = p.dq_acc + (int64_t)b * p.dqa_sb + (int64_t)q_row * p.dqa_ss + (int64_t)h * p.dqa_sh + 4 * g4;
    if (fin && !carry) {
#pragma unroll
        for (int db = 0; db < 8; ++db) {
            const f32x4 a = dq[2 * db + QH];
            global_store_b64(op + 16 * db, u32x2{pack_bf16x2(a[0] * sc, a[1] * sc), pack_bf16x2(a[2] * sc, a[3] * sc)});
        }
    } else {
#pragma unroll
        for (int db = 0; db < 8; ++db) {
            const f32x4 a = dq[2 * db + QH];
            float o0 = a[0] * sc, o1 = a[1] * sc, o2 = a[2] * sc, o3 = a[3] * sc;
            if (carry) {
                const f32x4 c = global_load_f32x4(ap + 16 * db);
                o0 += c[0]; o1 += c[1]; o2 += c[2]; o3 += c[3];
            }
            if (fin) global_store_b64(op + 16 * db, u32x2{pack_bf16x2(o0, o1), pack_bf16x2(o2, o3)});
            else global_store_f32x4(ap + 16 * db, f32x4{o0, o1, o2, o3});
        }
    }
}

template <bool HAS_META>
LWM_DEVICE void attn_bwd_dq4_body(const AttnParams& p) {
    const lds_t lds = dyn_lds();
    const int tid = thread_idx();
    const int wave = wave_uniform(tid >> 6), lane = tid & 63, l15 = lane & 15, g4 = lane >> 4;

    // ---- block -> (q block, head, batch): all q blocks of one (b,h) on one XCD, longest walks (the last blocks) first
    const int nqb = (p.Sq + kQ4BQ - 1) / kQ4BQ;
    const int HB = p.H * p.B;
    int lin = block_idx_x(), qbi, hb;
    if ((HB & 7) == 0) {
        int xcd = lin & 7, i = lin >> 3;
        hb = xcd + 8 * (i / nqb);
        qbi = nqb - 1 - (i % nqb);
    } else {
        hb = lin / nqb;
        qbi = nqb - 1 - (lin % nqb);
    }
    const int b = hb / p.H, h = hb % p.H;
    const bf16_t* qb = p.q + (int64_t)b * p.q_sb + (int64_t)h * p.q_sh;
    const bf16_t* kb = p.k + (int64_t)b * p.k_sb + (int64_t)h * p.k_sh;
    const bf16_t* vb = p.v + (int64_t)b * p.v_sb + (int64_t)h * p.v_sh;
    const bf16_t* dob = p.dout + (int64_t)b * p.do_sb + (int64_t)h * p.do_sh;

    // ---- this lane's two queries (row 16 qh + c of the wave's 32): fragments straight into the accumulator file (a row
    // past Sq re-reads the last row: its results are never stored), their statistics
    int q_row[2], qr[2];
    bool q_ok[2];
#pragma unroll
    for (int qh = 0; qh < 2; ++qh) {
        q_row[qh] = qbi * kQ4BQ + wave * 32 + 16 * qh + l15;
        q_ok[qh] = q_row[qh] < p.Sq;
        qr[qh] = q_ok[qh] ? q_row[qh] : p.Sq - 1;
    }
    bf16x8 qf[8], dof[8];       // [4 qh + s]: d step s of 32
#pragma unroll
    for (int i = 0; i < 8; ++i) qf[i] = f4_load_agpr(qb + (int64_t)qr[i >> 2] * p.q_ss + 32 * (i & 3) + 8 * g4);
#pragma unroll
    for (int i = 0; i < 8; ++i) dof[i] = f4_load_agpr(dob + (int64_t)qr[i >> 2] * p.do_ss + 32 * (i & 3) + 8 * g4);
    Q4Ctx cx;
    Q4Regs rg;
    {
        const int64_t Sqp = bwd_stat_pad(p.Sq), srow = bwd_stat_row((int64_t)b * p.H + h, Sqp);
#pragma unroll
        for (int qh = 0; qh < 2; ++qh) {
            cx.nl[qh] = q_ok[qh] ? p.delta[srow + qr[qh]] : -INFINITY;
            const float nd = p.delta[srow + Sqp + qr[qh]];
#pragma unroll
            for (int r = 0; r < 4; ++r) rg.ndl[qh][r] = nd;
        }
        q4_opaque(rg.ndl);
    }
    cx.c = p.scale * kLog2e;
    int32_t seg_q[2];
#pragma unroll
    for (int qh = 0; qh < 2; ++qh) seg_q[qh] = (HAS_META && q_ok[qh] && p.seg_q) ? p.seg_q[(int64_t)b * p.Sq + q_row[qh]] : 0;
    const PosMap km = k_map(p);
    const PosTab kt_ = load_postab(km);                           // (register copies of the tables: prologue only)
    const int64_t q_base = pos_base(load_postab(q_map(p)), qbi * kQ4BQ);       // position of query row r of this workgroup = q_base + r

    // ---- key step range of the walk (steps of 64 keys; causal: up to the diagonal of the workgroup's last query)
    const int nst_all = (p.Sk + kQ4BK - 1) / kQ4BK;
    int nst = nst_all, st0 = 0;
    const int q_last = (qbi * kQ4BQ + kQ4BQ < p.Sq ? qbi * kQ4BQ + kQ4BQ : p.Sq) - 1;
    if (p.causal) nst = tiles_reaching(kt_, kQ4BK, nst_all, q_base + q_last);      // up to the step of the last visible key
    if (HAS_META && p.segb_q && p.segb_k && nst > 0) {     // packed sequences: skip other documents' key steps
        const int nbq = (p.Sq + 31) >> 5, nbk = (p.Sk + 31) >> 5;
        int smin, smax, lo, hi2;
        seg_own_range(p.segb_q + (int64_t)b * nbq * 2, nbq, qbi * (kQ4BQ / 32), kQ4BQ / 32, smin, smax);
        seg_narrow<kD4Threads>(p.segb_k + (int64_t)b * nbk * 2, nbk, kQ4BK / 32, 0, nst, smin, smax, lds + kQ4OffMeta, tid, lo, hi2);
        st0 = lo;
        nst = hi2;
    }
    const int n = nst > st0 ? nst - st0 : 0;       // walk index i -> key step st0 + i (ascending)

    f32x4 dq[16];               // [2 db + qh]: dQ^T rows 16 db + 4g + 0..3 of query 16 qh + c
    if (n == 0)
#pragma unroll
        for (int i = 0; i < 16; ++i) dq[i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    if (n == 0) {
        f4_load_agpr_wait8(qf);
        f4_load_agpr_wait8(dof);
    }

    if (n > 0) {
#pragma unroll
        for (int s = 0; s < 4; ++s) cx.ka[s] = lds + q4_tile_off(l15, 4 * s + g4);
#pragma unroll
        for (int db = 0; db < 8; ++db) {
            // lane t of a 16-lane group addresses key 4g + (t>>2), d 16 db + 4 (t&3): four keys x 16 d per group
            cx.tlo[db] = lds + q4_tile_off(4 * g4 + (l15 >> 2), 2 * db + ((l15 & 3) >> 1)) + (l15 & 1) * 8;
            cx.plo[db] = cx.tlo[db];
        }
        cx.meta = lds + kQ4OffMeta + 16 * g4;
        const int64_t k_step_bytes = (int64_t)kQ4BK * p.k_ss * 2, v_step_bytes = (int64_t)kQ4BK * p.v_ss * 2;
        uint32_t vk[4], vv[4];
        q4_stage_offsets(p, wave, lane, 0, vk, vv);       // full steps: nothing is clamped
        // key meta of walk index i -> meta slot i & 3: segment id, or kSegInvalid for padded / out-of-range keys
        auto meta_stage = [&](int i) {
            if (HAS_META && tid < kQ4BK) {
                const int krow = (st0 + i) * kQ4BK + tid;
                const int kr = krow < p.Sk ? krow : p.Sk - 1;
                const uint8_t kvalid = p.key_valid ? p.key_valid[(int64_t)b * p.Sk + kr] : (uint8_t)1;
                const int32_t kseg = p.seg_k ? p.seg_k[(int64_t)b * p.Sk + kr] : 0;
                lds_write_i32(lds + kQ4OffMeta + (i & 3) * kQ4BK * 4 + tid * 4, (krow < p.Sk && kvalid != 0) ? kseg : kSegInvalid);
            }
        };
        auto stage_step = [&](int i) {
            const int st = st0 + i;
            const lds_t dst = lds + (i & 3) * kD4SlotBytes + (uint32_t)wave * 1024;
            const char* ks = (const char*)kb + st * k_step_bytes;
            const char* vs = (const char*)vb + st * v_step_bytes;
            if (st * kQ4BK + kQ4BK > p.Sk) {
                uint32_t v2[4], d2[4];
                q4_stage_offsets(p, wave, lane, st, v2, d2);
                f4_dma<4>(v2, ks, dst);
                f4_dma<4>(d2, vs, dst + kD4TileBytes);
            } else {
                f4_dma<4>(vk, ks, dst);
                f4_dma<4>(vv, vs, dst + kD4TileBytes);
            }
            meta_stage(i);
        };
        // the ragged last step of the K/V block may only be staged from this slow path: the pipelined steps stop before it
        const bool ragged = (p.Sk % kQ4BK) != 0;
        const int n_pipe_end = (ragged && nst == nst_all) ? n - 1 : n;      // walk indices >= this are never issued in-loop

        // ---- prologue: steps 0 and 1 in flight, waited for together with the Q / dO fragments
        stage_step(0);
        if (n > 1) stage_step(1);
        f4_load_agpr_wait8(qf);      // vmcnt(0): everything requested so far
        f4_load_agpr_wait8(dof);
        block_sync();

        auto clamp32 = [](int64_t x) -> int { return x > (1 << 30) ? (1 << 30) : (x < -(1 << 30) ? -(1 << 30) : (int)x); };
        // positions relative to k_start; a unit's first key (row ub of the K/V block) sits at rel_pos(km, ub)
        int q_rel[2];                                                                    // this lane's queries
#pragma unroll
        for (int qh = 0; qh < 2; ++qh) q_rel[qh] = clamp32(q_base + q_row[qh] - p.k_start) - 4 * g4;
        PosCursor kc = cursor_begin(kt_);
        auto k_rel_of = [&](int ub) -> int {             // (the walk ascends)
            cursor_seek(km, kc, ub);
            return clamp32(kc.base + ub - p.k_start);
        };
        // a unit needs the mask code when its last key lies after the wave's first query: positions ascend with the row,
        // so those are the units from row mask_from of the K/V block on (one compare per unit in the walk)
        const int mask_from = p.causal ? 32 * tiles_below(kt_, 32, (p.Sk + 31) / 32, q_base + (int64_t)qbi * kQ4BQ + wave * 32) : 0x7fffffff;
        auto needs_causal = [&](int ub) -> bool { return ub >= mask_from; };
        // the wave's 32 queries of one segment?  (then a step whose 64 keys carry it needs no segment test; rows past Sq
        // are never stored and do not count)
        const int32_t own_seg = wave_uniform(seg_q[0]);
        const bool own_uniform = HAS_META && !wave_any((q_ok[0] && seg_q[0] != own_seg) || (q_ok[1] && seg_q[1] != own_seg));
        auto rel_of = [&](int ub, int (&rel)[2]) {
            if (!p.causal) {
                rel[0] = rel[1] = 64;
                return;
            }
            const int kr = k_rel_of(ub);
#pragma unroll
            for (int qh = 0; qh < 2; ++qh) {
                const int64_t d = (int64_t)q_rel[qh] - kr;
                rel[qh] = d > 64 ? 64 : (d < -64 ? -64 : (int)d);
            }
        };

#pragma unroll
        for (int par = 0; par < 2; ++par)
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                rg.s[par][t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                rg.dp[par][t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            rg.t[r] = 0.0f;
            rg.ds[r] = 0.0f;
        }
#pragma unroll
        for (int t = 0; t < 2; ++t) rg.dsb[t] = zero_bf16x8();
#pragma unroll
        for (int j = 0; j < 8; ++j) rg.fr[j] = zero_bf16x8();
        D4Dma dm = {};
#pragma unroll
        for (int j = 0; j < kD4Ahead; ++j) rg.fr[j] = q4_frag<0>(cx, j);

#define LWM_Q4_MASK(HALF_, HAS_PREV_, ub_)                                                                          \
    do {                                                                                                            \
        if (!(HAS_PREV_)) q4_settle_t(rg.s[HALF_]);     /* no MFMA stands between the S chains and their first reader */ \
        if ((HAS_META && !uni_) || needs_causal(ub_)) {                                                             \
            if (HAS_PREV_) q4_settle_t(rg.s[HALF_]);                                                                \
            int rel_[2];                                                                                            \
            rel_of(ub_, rel_);                                                                                      \
            if (HAS_META && !uni_) q4_mask<HALF_, HAS_META>(cx, rg.s[HALF_], rel_, seg_q);                          \
            else q4_mask<HALF_, false>(cx, rg.s[HALF_], rel_, seg_q);                                               \
        }                                                                                                           \
    } while (0)
        int ub = st0 * kQ4BK;
        const char* k_src2 = (const char*)kb + (int64_t)(st0 + 2) * k_step_bytes;
        const char* v_src2 = (const char*)vb + (int64_t)(st0 + 2) * v_step_bytes;
#define LWM_Q4_STEP(i, FIRST, PIPE)                                                                                 \
    do {                                                                                                            \
        if (PIPE) {                                                                                                 \
            dm.q_src = k_src2;                                                                                      \
            dm.do_src = v_src2;                                                                                     \
            dm.dst = lds + (((i) + 2) & 3) * kD4SlotBytes + (uint32_t)wave * 1024;                                  \
            k_src2 += k_step_bytes;                                                                                 \
            v_src2 += v_step_bytes;                                                                                 \
            meta_stage((i) + 2);                                                                                    \
        }                                                                                                           \
        const uint32_t d_ = (((i) & 3) == 3) ? (uint32_t)(-3 * kD4SlotBytes) : (uint32_t)kD4SlotBytes;             \
        const uint32_t e_ = (((i) & 3) == 3) ? (uint32_t)(-3 * kQ4BK * 4) : (uint32_t)(kQ4BK * 4);                 \
        const int32_t segw_ = HAS_META ? seg_step_word(cx.meta - 16 * g4, lane) : 0;                               \
        q4_x<0, !(FIRST), PIPE>(cx, rg, qf, dof, vk, vv, dm);                                                       \
        const bool uni_ = HAS_META && seg_step_uniform(segw_, own_uniform, own_seg);                                \
        LWM_Q4_MASK(0, !(FIRST), ub);                                                                               \
        q4_y<0, !(FIRST), false>(cx, rg, dq);                                                                       \
        q4_x<1, true, false>(cx, rg, qf, dof, vk, vv, dm);                                                          \
        for (int s_ = 0; s_ < 4; ++s_) cx.ka[s_] += d_;                                                             \
        LWM_Q4_MASK(1, true, ub + 32);                                                                              \
        q4_y<1, true, FIRST>(cx, rg, dq);                                                                           \
        ub += kQ4BK;                                                                                                \
        if ((FIRST) || !(PIPE)) q4_settle_acc(dq);                                                                  \
        glds_wait_all();                                                                                            \
        block_sync_lds();                                                                                           \
        for (int db_ = 0; db_ < 8; ++db_) {                                                                         \
            cx.plo[db_] = cx.tlo[db_];                                                                              \
            cx.tlo[db_] += d_;                                                                                      \
        }                                                                                                           \
        cx.meta += e_;                                                                                              \
    } while (0)

        int i = 0;
        if (n_pipe_end > 2) {
            LWM_Q4_STEP(0, true, true);
            for (i = 1; i + 2 < n_pipe_end; ++i) LWM_Q4_STEP(i, false, true);
            // the ragged last step (if any) was not issued by the loop: stage it now, two steps ahead of its use
            if (n_pipe_end < n) {
                stage_step(n - 1);
                glds_wait_all();
                block_sync_lds();
            }
            for (; i < n; ++i) LWM_Q4_STEP(i, false, false);
        } else {
            if (n > 2) {                 // (n == 3 with a ragged last step: nothing was pipelined)
                stage_step(2);
                glds_wait_all();
                block_sync_lds();
            }
            LWM_Q4_STEP(0, true, false);
            for (i = 1; i < n; ++i) LWM_Q4_STEP(i, false, false);
        }
#undef LWM_Q4_STEP
#undef LWM_Q4_MASK
        // the last unit's product: its K tile is the second half of the PREVIOUS slot now (the registers moved on)
        q4_drain<1>(cx, rg, dq);
        q4_settle_acc(dq);      // before the paths merge
    }

    // ---- epilogue: scale, merge with the ring carry, store (a query row per lane and half: 16 stores of 4 consecutive d)
    q4_settle_acc(dq);
    if (q_ok[0]) q4_store<0>(p, dq, b, h, q_row[0], g4);
    if (q_ok[1]) q4_store<1>(p, dq, b, h, q_row[1], g4);
}

LWM_KERNEL(kD4Threads) void attn_bwd_dq4_kernel(AttnParams p) { attn_bwd_dq4_body<false>(p); }
LWM_KERNEL(kD4Threads) void attn_bwd_dq4_meta_kernel(AttnParams p) { attn_bwd_dq4_body<true>(p); }

// ====================================================================================================== dQ from dS
// The consumer of the dS hand-over (above): dQ = scale * dS K, ONE GEMM unit, no softmax, no masks -- a tile the dK/dV
// walk did not visit holds only zeros and is simply not part of the sum, a masked element inside a visited tile was
// stored as 0.  The kernel streams 2 bytes per 128 FLOP and is bound by HBM.
//
// Workgroup = 4 waves = 256 queries; a wave owns 64 query rows = one step st of the producer, i.e. ONE tile per key
// step, private to the wave.  A key step = the 32 keys of one producer wave (key block kbi = step >> 2, wave step & 3),
// ascending: the sum runs in key order, fixed, no atomics.  Computed transposed like the dQ kernel above:
// dQ^T[db < 8][column tile] += K^T(db) dS^T, A = the transposed K fragments of the recompute kernel's Y phase, B = dS^T
// read with the same instruction from the staged tile, 8 + 4 fragments for 32 MFMAs, the accumulators (32 tiles of
// 16 x 16) in the accumulator file: 128 AGPRs.
//
// K (8 KiB per step, two 1-KiB pieces per wave, the q4 tile image) and the wave's tile (4 pieces) arrive by LDS-DMA
// through a ring of kS4Slots slots, kS4Ahead steps ahead, behind counted waits; one barrier per step.
//
// The staged tile keeps the producer's 16-byte pieces whole and permutes them (on the SOURCE address of the DMA): the
// piece of producer lane (c, g') stands at position 16 g' + (c ^ 8 (g' & 1)) of its 1-KiB unit-and-key-half.  The lane
// t = 4 r + m of 16-lane group g of a transposed read points at key 4g + r and takes its four queries from the query
// half m & 1 of producer group g' = 2 T + (m >> 1): a half-wave then reads 16 whole pieces at 16 distinct positions
// mod 16 = every bank once (s4_image_ok).  Column t of the B operand -- and of the accumulator tiles [.., T] of the
// unit -- is therefore query 16 ((t >> 2) & 1) + 4 (2 T + (t >> 3)) + (t & 3) of the unit, which is all the epilogue
// needs to know; k-group g holds keys {4g .. 4g+3, 16+4g .. 16+4g+3} as in the other two kernels.
constexpr int kS4BQ = 256;      // queries per workgroup
constexpr int kS4BK = 32;       // keys per step
constexpr int kS4Slots = 3;                // 72 KiB of LDS, 208 registers: TWO workgroups per CU -- one waits at its
                                           // barrier while the other's pieces arrive (measured: 5.7 ms against 6.2 ms with
                                           // four slots, three steps ahead and one workgroup per CU)
constexpr int kS4Ahead = kS4Slots - 1;     // steps in flight
constexpr int kS4KBytes = kS4BK * kRowBytes;                     // 8 KiB
constexpr int kS4SlotBytes = kS4KBytes + 4 * kDsTileBytes;       // K tile | the four waves' dS tiles
constexpr int kS4LdsBytes = kS4Slots * kS4SlotBytes;
static_assert(kS4Ahead == 2 || kS4Ahead == 3, "the counted waits below leave one or two steps in flight");

constexpr int s4_piece_pos(int c, int g) { return 16 * g + (c ^ ((g & 1) << 3)); }
// byte offset, inside a 1-KiB unit-and-key-half, of the 8 bytes lane (t, g) of a transposed read of column tile T points at
constexpr int s4_read_off(int t, int g, int T) { return 16 * s4_piece_pos(4 * g + (t >> 2), 2 * T + ((t & 3) >> 1)) + 8 * (t & 1); }
constexpr bool s4_image_ok() {
    for (int T = 0; T < 2; ++T)
        for (int half = 0; half < 2; ++half) {
            unsigned long long banks = 0;
            for (int l = 32 * half; l < 32 * half + 32; ++l) {
                const int a = s4_read_off(l & 15, l >> 4, T);
                const unsigned long long b = 0x3ull << ((a >> 2) & 63);
                if (banks & b) return false;
                banks |= b;
            }
            if (banks != ~0ull) return false;
        }
    // the permutation is an involution on the 64 pieces (the DMA applies it to the source, the reads to the image)
    for (int l = 0; l < 64; ++l)
        if (s4_piece_pos(s4_piece_pos(l & 15, l >> 4) & 15, s4_piece_pos(l & 15, l >> 4) >> 4) != l) return false;
    return true;
}
static_assert(s4_image_ok(), "a transposed read of the staged dS tile is bank-conflicted");

// at most N vector-memory operations outstanding, N one of the sums a step's piece counts (0, 2 or 6) can make
LWM_DEVICE void s4_wait_keep(int cnt) {
    if (cnt >= 12) wait_vmem_le<12>();
    else if (cnt >= 8) wait_vmem_le<8>();
    else if (cnt >= 6) wait_vmem_le<6>();
    else if (cnt >= 4) wait_vmem_le<4>();
    else if (cnt >= 2) wait_vmem_le<2>();
    else wait_vmem_le<0>();
}

// glds_load_b128 with the non-temporal hint (the tiles are read once; K is what the workgroups of an XCD share)
#ifdef LWM_EMU
LWM_DEVICE void s4_dma(const void* g, lds_t wave_base) { glds_load_b128(g, wave_base); }
#else
LWM_DEVICE void s4_dma(const void* g, lds_t wave_base) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off nt\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(g), "s"(wave_base) : "memory");
}
#endif
// a transposed fragment: the k-group's first four keys from `a`, its second four from `b`
LWM_DEVICE bf16x8 s4_frag(lds_t a, lds_t b) {
    const bf16x4 lo = lds_read_tr16(a), up = lds_read_tr16(b);
    bf16x8 o;
    o[0] = lo[0]; o[1] = lo[1]; o[2] = lo[2]; o[3] = lo[3];
    o[4] = up[0]; o[5] = up[1]; o[6] = up[2]; o[7] = up[3];
    return o;
}

LWM_DEVICE void attn_bwd_dq_ds_body(const AttnParams& p) {
    const lds_t lds = dyn_lds();
    const int tid = thread_idx();
    const int wave = wave_uniform(tid >> 6), lane = tid & 63, l15 = lane & 15, g4 = lane >> 4;

    // ---- block -> (q block, head, batch): the map of the dQ kernel
    const int nqb = (p.Sq + kS4BQ - 1) / kS4BQ;
    const int HB = p.H * p.B;
    int lin = block_idx_x(), qbi, hb;
    if ((HB & 7) == 0) {
        int xcd = lin & 7, i = lin >> 3;
        hb = xcd + 8 * (i / nqb);
        qbi = nqb - 1 - (i % nqb);
    } else {
        hb = lin / nqb;
        qbi = nqb - 1 - (lin % nqb);
    }
    const int b = hb / p.H, h = hb % p.H;
    const char* kb = (const char*)(p.k + (int64_t)b * p.k_sb + (int64_t)h * p.k_sh);

    // ---- the walk: this wave's tiles are the first n_w key steps, the workgroup walks those of its last query step
    const int nst = p.Sq / kD4BQ, nkb = p.Sk / kD4BK;
    const int64_t e = ds_diag(p.causal, p.q_start, p.k_start);
    const int s_w = 4 * qbi + wave, s_last = 4 * qbi + 3 < nst ? 4 * qbi + 3 : nst - 1;
    const int n_w = (int)ds_wave_steps(e, nst, nkb, s_w), n = (int)ds_wave_steps(e, nst, nkb, s_last);

    f32x4 dq[2][16];            // [unit hq][2 db + T]: dQ^T rows 16 db + 4g + 0..3 of the query of column c (file header)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        dq[0][i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        dq[1][i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    }
    q4_settle_acc(dq[0]);       // (compiler-written zeros: wait states before an MFMA reads them)
    q4_settle_acc(dq[1]);

    if (n > 0) {
        // per-lane addresses: the K tile's transposed fragments (as the dQ kernel's Y phase), the dS tile's
        uint32_t ka[8], da[2];
#pragma unroll
        for (int db = 0; db < 8; ++db) ka[db] = lds + q4_tile_off(4 * g4 + (l15 >> 2), 2 * db + ((l15 & 3) >> 1)) + (l15 & 1) * 8;
#pragma unroll
        for (int T = 0; T < 2; ++T) da[T] = lds + kS4KBytes + (uint32_t)wave * kDsTileBytes + (uint32_t)s4_read_off(l15, g4, T);
        // DMA sources: the wave's two K pieces (rows 4 (wave + 4j) + (l >> 4), the swizzle on the source column) and the
        // permuted piece of the tile
        uint32_t vk[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int row = 4 * (wave + 4 * j) + g4;
            vk[j] = (uint32_t)(((int64_t)row * p.k_ss + ((l15 ^ q4_swz(row)) << 3)) * 2);
        }
        const uint32_t vds = (uint32_t)s4_piece_pos(l15, g4) * 16;
        const int64_t k_step_bytes = (int64_t)kS4BK * p.k_ss * 2;
        // the cursor of the DMA: the row of tiles of key step `nxt` (it begins at the key block's first visited step)
        const char* row_p = p.ds_ws + (int64_t)hb * ds_steps_before(e, nst, nkb) * 4 * kDsTileBytes;
        int first = (int)ds_first_step(e, nst, 0);
        const char* k_src = kb;
        int nxt = 0;
        uint32_t so_nxt = 0;        // byte offset of the slot of step nxt
        auto issue = [&]() {        // the pieces of key step nxt -> its slot
            const lds_t dst = lds + so_nxt;
            glds_load_b128(k_src + vk[0], dst + (uint32_t)wave * 1024);
            glds_load_b128(k_src + vk[1], dst + (uint32_t)(wave + 4) * 1024);
            if (nxt < n_w) {
                const char* t = row_p + (int64_t)(s_w - first) * kDsTileBytes + vds;
#pragma unroll
                for (int c = 0; c < 4; ++c) s4_dma(t + 1024 * c, dst + kS4KBytes + (uint32_t)wave * kDsTileBytes + 1024 * c);
            }
            row_p += (int64_t)(nst - first) * kDsTileBytes;
            if ((nxt & 3) == 3) first = (int)ds_first_step(e, nst, (nxt >> 2) + 1);
            k_src += k_step_bytes;
            so_nxt = so_nxt + kS4SlotBytes == (uint32_t)kS4LdsBytes ? 0u : so_nxt + (uint32_t)kS4SlotBytes;
            ++nxt;
        };
        auto pieces = [&](int j) -> int { return j < n ? (j < n_w ? 6 : 2) : 0; };

        for (int j = 0; j < kS4Ahead && j < n; ++j) issue();
        s4_wait_keep(pieces(1) + (kS4Ahead == 3 ? pieces(2) : 0));
        block_sync_lds();

        // step i: the pieces of step i + kS4Ahead go out (their slot was read last in step i - 1), the products of step i,
        // then step i + 1 must have landed for every wave: the younger steps stay in flight across the barrier
        uint32_t so = 0;             // byte offset of the slot of step i
        for (int i = 0; i < n; ++i) {
            if (i + kS4Ahead < n) issue();
            if (i < n_w) {
                bf16x8 bf[2][2], af[8];
#pragma unroll
                for (int hq = 0; hq < 2; ++hq)
#pragma unroll
                    for (int T = 0; T < 2; ++T) bf[hq][T] = s4_frag(da[T] + so + 2048 * hq, da[T] + so + 2048 * hq + 1024);
#pragma unroll
                for (int db = 0; db < 8; ++db) af[db] = s4_frag(ka[db] + so, ka[db] + so + 16 * kRowBytes);
#pragma unroll
                for (int db = 0; db < 8; ++db)
#pragma unroll
                    for (int j = 0; j < 4; ++j) q4_mfma_o(dq[j >> 1][2 * db + (j & 1)], af[db], bf[j >> 1][j & 1]);
            }
            s4_wait_keep(pieces(i + 2) + (kS4Ahead == 3 ? pieces(i + 3) : 0));
            block_sync_lds();
            so = so + kS4SlotBytes == (uint32_t)kS4LdsBytes ? 0u : so + (uint32_t)kS4SlotBytes;
        }
        q4_settle_acc(dq[0]);       // before the paths merge, and before compiler-generated code reads the tuples
        q4_settle_acc(dq[1]);
    }

    // ---- epilogue: the row-wise stores of the dQ kernel; column c of tile [.., T] of unit hq is this query
    q4_settle_acc(dq[0]);
    q4_settle_acc(dq[1]);
    if (s_w < nst) {
        const int row0 = s_w * kD4BQ + 16 * ((l15 >> 2) & 1) + 4 * (l15 >> 3) + (l15 & 3);
        q4_store<0>(p, dq[0], b, h, row0, g4);
        q4_store<1>(p, dq[0], b, h, row0 + 8, g4);
        q4_store<0>(p, dq[1], b, h, row0 + 32, g4);
        q4_store<1>(p, dq[1], b, h, row0 + 40, g4);
    }
}

LWM_KERNEL(kD4Threads) void attn_bwd_dq_ds_kernel(AttnParams p) { attn_bwd_dq_ds_body(p); }

}  // namespace lwm
