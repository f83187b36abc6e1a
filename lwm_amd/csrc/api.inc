// api.inc -- the C ABI of include/lwm_hip.h: argument validation, grid sizing,
// kernel launches.  Included by lwm_hip.hip (product, HIP launch glue) and by
// tests/emu/lwm_emu.cpp (host emulation of the same kernels; test-only).
// Expects: wave_ops.h, launch.h, attn_common.h, attn_fwd.h, attn_fwd64.h, attn_bwd.h, attn_bwd64.h,
// misc_kernels.h and "lwm_hip.h" already included.
#include "sample.h"
#include "optim.h"
#include "dropout.h"
#include "attn_decode_kvq.h"
#include "attn_decode_kv8.h"
#include "attn_decode_kv4.h"
#include "attn_prefill_kv8.h"
#include "attn_decode_kv6.h"
#include "attn_prefill_kv6.h"
#include "gemv_w8.h"
#include "gemv_w4.h"
#include "gemv_w6.h"
#include "gemm_rows.h"

namespace lwm {

static bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

static int check_t4(const char* name, const LwmTensor4& t, bool required) {
    if (!t.ptr) return required ? fail(LWM_EINVAL, "%s: null pointer", name) : 0;
    if (!aligned16(t.ptr)) return fail(LWM_EINVAL, "%s: pointer not 16-byte aligned", name);
    if ((t.stride_b % 8) || (t.stride_s % 8) || (t.stride_h % 8))
        return fail(LWM_EINVAL, "%s: strides must be multiples of 8 elements", name);
    return 0;
}

// piecewise position maps: cuts strictly inside the operand on multiples of 256 rows, positions ascending, no overlap
static int check_pieces(const char* side, int32_t n, const int32_t* row, const int64_t* pos, int64_t start, int32_t S) {
    if (n <= 1) return 0;
    if (n > LWM_MAX_PIECES) return fail(LWM_EINVAL, "%s: %ld pieces (at most %ld)", side, (long)n, (long)LWM_MAX_PIECES);
    if (row[0] != 0 || pos[0] != start) return fail(LWM_EINVAL, "%s: piece 0 must be (row 0, position *_start)", side);
    for (int i = 1; i < n; ++i)
        if (row[i] <= row[i - 1] || row[i] >= S || (row[i] & 255) || pos[i] < pos[i - 1] + (row[i] - row[i - 1]))
            return fail(LWM_EINVAL, "%s: piece %ld: rows must be multiples of 256, ascending, inside (0, S); positions ascending, no overlap", side, (long)i);
    return 0;
}

static int check_common(const LwmAttnArgs* a) {
    if (!a) return fail(LWM_EINVAL, "%s", "args is null");
    if (a->D != kHeadDim) return fail(LWM_EUNSUPPORTED, "%s: head_dim %ld (only 128)", "attn", a->D);
    if (a->B < 0 || a->H <= 0 || a->Sq < 0 || a->Sk < 0)
        return fail(LWM_EINVAL, "%s", "negative dimension");
    if ((a->segment_ids_q == nullptr) != (a->segment_ids_k == nullptr))
        return fail(LWM_EINVAL, "%s", "segment_ids_q and segment_ids_k must be given together");
    if (!(a->scale > 0.0f)) return fail(LWM_EINVAL, "%s", "scale must be > 0");
    int rp;
    if ((rp = check_pieces("q", a->q_pieces, a->q_piece_row, a->q_piece_pos, a->q_start, a->Sq))) return rp;
    if ((rp = check_pieces("k", a->k_pieces, a->k_piece_row, a->k_piece_pos, a->k_start, a->Sk))) return rp;
    int r;
    if ((r = check_t4("q", a->q, true))) return r;
    if ((r = check_t4("k", a->k, true))) return r;
    if ((r = check_t4("v", a->v, true))) return r;
    return 0;
}

static AttnParams to_params(const LwmAttnArgs* a) {
    AttnParams p;
    memset(&p, 0, sizeof(p));
    p.q = (const bf16_t*)a->q.ptr; p.k = (const bf16_t*)a->k.ptr; p.v = (const bf16_t*)a->v.ptr;
    p.out = (bf16_t*)a->out.ptr;
    p.lse = a->lse; p.out_acc = a->out_acc; p.lse_acc = a->lse_acc;
    p.dout = (const bf16_t*)a->dout.ptr;
    p.delta = a->delta;
    p.dq = (bf16_t*)a->dq.ptr; p.dk = (bf16_t*)a->dk.ptr; p.dv = (bf16_t*)a->dv.ptr;
    p.dq_acc = a->dq_acc; p.dk_acc = a->dk_acc; p.dv_acc = a->dv_acc;
    p.seg_q = a->segment_ids_q; p.seg_k = a->segment_ids_k; p.key_valid = a->key_valid;
    p.q_sb = a->q.stride_b; p.q_ss = a->q.stride_s; p.q_sh = a->q.stride_h;
    p.k_sb = a->k.stride_b; p.k_ss = a->k.stride_s; p.k_sh = a->k.stride_h;
    p.v_sb = a->v.stride_b; p.v_ss = a->v.stride_s; p.v_sh = a->v.stride_h;
    p.o_sb = a->out.stride_b; p.o_ss = a->out.stride_s; p.o_sh = a->out.stride_h;
    p.do_sb = a->dout.stride_b; p.do_ss = a->dout.stride_s; p.do_sh = a->dout.stride_h;
    p.dq_sb = a->dq.stride_b; p.dq_ss = a->dq.stride_s; p.dq_sh = a->dq.stride_h;
    p.dk_sb = a->dk.stride_b; p.dk_ss = a->dk.stride_s; p.dk_sh = a->dk.stride_h;
    p.dv_sb = a->dv.stride_b; p.dv_ss = a->dv.stride_s; p.dv_sh = a->dv.stride_h;
    p.B = a->B; p.H = a->H; p.Sq = a->Sq; p.Sk = a->Sk;
    p.q_start = a->q_start; p.k_start = a->k_start;
    p.q_np = a->q_pieces > 1 ? a->q_pieces : 1;
    p.k_np = a->k_pieces > 1 ? a->k_pieces : 1;
    for (int i = 0; i < kMaxPieces; ++i) {       // unused entries: a row no tile reaches
        const bool qi = i < p.q_np, ki = i < p.k_np;
        p.q_row[i] = i == 0 ? 0 : (qi ? a->q_piece_row[i] : 0x7fffffff);
        p.k_row[i] = i == 0 ? 0 : (ki ? a->k_piece_row[i] : 0x7fffffff);
        p.q_pos[i] = i == 0 ? a->q_start : (qi ? a->q_piece_pos[i] : 0);
        p.k_pos[i] = i == 0 ? a->k_start : (ki ? a->k_piece_pos[i] : 0);
    }
    p.scale = a->scale;
    p.causal = a->causal ? 1 : 0;
    p.carry_in = a->carry_in ? 1 : 0;
    p.final_out = a->final_out ? 1 : 0;
    p.dense_mask = a->dense_mask;
    p.msk_sb = a->mask_stride_b; p.msk_sq = a->mask_stride_q;
    p.k_splits = a->k_splits > 1 ? a->k_splits : 1;
    p.segb_q = a->seg_blocks_q; p.segb_k = a->seg_blocks_k;
    if (a->dq_acc_head_major) {       // [B,H,Sq,D]: a 32-query tile of one head is 16 KiB contiguous
        p.dqa_ss = kHeadDim; p.dqa_sh = (int64_t)a->Sq * kHeadDim; p.dqa_sb = (int64_t)a->H * a->Sq * kHeadDim;
    } else {                          // [B,Sq,H,D]
        p.dqa_sh = kHeadDim; p.dqa_ss = (int64_t)a->H * kHeadDim; p.dqa_sb = (int64_t)a->Sq * a->H * kHeadDim;
    }
    return p;
}

// The entries of the quantised caches (attn_decode_kv8.h, attn_decode_kv4.h, attn_decode_kv6.h) share their checks.  What differs per
// entry is passed in: the names, the kernel, the code that its shape and alignment refusals return, and the alignment
// rule.  `at`: the destination row comes from device memory (row0_dev) and dst_row0 is the offset added to it.
template <class P>
static int kvq_cache_write(const char* name, const char* kname, void (*kernel)(P), bool at, int ecode,
                           int cache_align, int scale_stride_align, const char* align_rule, void* cache, const void* src,
                           int32_t B, int64_t cache_stride_b, int64_t src_stride_b, const int32_t* row0_dev, int64_t dst_row0,
                           int64_t cache_rows, int64_t src_row0, int64_t nrows, int32_t row_elems, void* scale,
                           int64_t scale_stride_b, int32_t H, void* stream) {
    if (!cache || !src || !scale) return fail(LWM_EINVAL, "%s: null pointer", name);
    if (B < 0 || nrows < 0 || H <= 0 || src_row0 < 0 || cache_stride_b < 0 || scale_stride_b < 0 || src_stride_b < 0)
        return fail(LWM_EINVAL, "%s: bad dimension", name);
    if (row_elems != H * kHeadDim)
        return fail(ecode, "%s: row_elems = %ld, H * 128 = %ld (head_dim is 128)", name, (long)row_elems, (long)H * kHeadDim);
    if (!aligned16(src) || (src_stride_b & 7) || (((uintptr_t)cache | (uintptr_t)cache_stride_b) & (cache_align - 1)) ||
        (((uintptr_t)scale) & 3) || (scale_stride_b & (scale_stride_align - 1)))
    {
        char msg[160];
        snprintf(msg, sizeof(msg), "%s: misaligned (%s)", name, align_rule);
        return fail(ecode, "%s", msg);
    }
    if (at && !row0_dev) return fail(LWM_EINVAL, "%s: null pointer", name);
    if (at ? cache_rows < 0 : dst_row0 < 0) return fail(LWM_EINVAL, "%s: bad dimension", name);
    if (B == 0 || nrows == 0) return LWM_OK;
    P p;
    p.cache = (uint8_t*)cache; p.scale = (decltype(p.scale))scale; p.src = (const bf16_t*)src;
    p.cache_sb = cache_stride_b; p.scale_sb = scale_stride_b; p.src_sb = src_stride_b;
    p.row0_dev = row0_dev; p.dst_row0 = dst_row0;
    p.cache_rows = at ? cache_rows : dst_row0 + nrows;          // host index: the caller has checked the range against its cache
    p.src_row0 = src_row0; p.nrows = nrows; p.B = B; p.H = H;
    const int64_t blocks = ((int64_t)B * nrows * H * 16 + 255) / 256;
    return launch(kname, kernel, (long)(blocks > 16384 ? 16384 : blocks), 256, 0, stream, p);
}

// What the decode and the block entries check of the cache, the outputs and k_splits, in this order.  ecode: what an
// alignment refusal returns.  head_bytes > 0: the strides are checked too (non-negative, a head no smaller than that).
// scales_f32: the scale pointers are checked for 4-byte alignment with lse_acc.  row_align: 16, or 8 where a lane's part
// of a row is loaded in 8-byte words.
template <class Args>
static int kvq_check_cache(const char* name, int ecode, int head_bytes, bool scales_f32, int row_align, const Args* a) {
    if (!a->k || !a->v || !a->k_scale || !a->v_scale || !a->out_acc || !a->lse_acc)
        return fail(LWM_EINVAL, "%s: null pointer (k, v, k_scale, v_scale, out_acc, lse_acc)", name);
    if (!aligned16(a->out_acc) || (((uintptr_t)a->k | (uintptr_t)a->v | (uintptr_t)a->k_stride_b | (uintptr_t)a->k_stride_s |
                                    (uintptr_t)a->k_stride_h | (uintptr_t)a->v_stride_b | (uintptr_t)a->v_stride_s |
                                    (uintptr_t)a->v_stride_h) & (uintptr_t)(row_align - 1)))
        return fail(ecode, row_align == 16 ? "%s: cache rows and out_acc must be 16-byte aligned (pointers and strides)"
                                           : "%s: cache rows must be 8-byte and out_acc 16-byte aligned (pointers and strides)", name);
    if (head_bytes > 0 &&
        (a->k_stride_s < 0 || a->v_stride_s < 0 || a->k_stride_h < head_bytes || a->v_stride_h < head_bytes || a->k_scale_stride_s < 0 ||
         a->v_scale_stride_s < 0 || a->k_scale_stride_b < 0 || a->v_scale_stride_b < 0 || a->k_stride_b < 0 || a->v_stride_b < 0))
        return fail(LWM_EINVAL, "%s: bad strides (non-negative; a head is %ld bytes)", name, (long)head_bytes);
    if (((scales_f32 ? (uintptr_t)a->k_scale | (uintptr_t)a->v_scale : 0) | (uintptr_t)a->lse_acc) & 3)
        return fail(ecode, scales_f32 ? "%s: scales and lse_acc must be 4-byte aligned" : "%s: lse_acc must be 4-byte aligned", name);
    if (a->k_splits < 0 || a->k_splits > 4096) return fail(LWM_EINVAL, "%s: k_splits out of range", name);
    return 0;
}

// ecode: what the shape and alignment refusals of the entry return.  head_bytes (> 0: the strides are checked too),
// scales_f32 and row_align (16, or 8 for rows loaded in 8-byte words): passed on to kvq_check_cache above.
template <class F, class P, class Args>
static int kvq_attn_decode(const char* name, void (*kernel)(P), int ecode, int head_bytes, bool scales_f32, int row_align,
                           const Args* a, void* stream) {
    if (!a) return fail(LWM_EINVAL, "%s: args is null", name);
    int r;
    if ((r = check_t4("q", a->q, true))) return r;
    if (a->D != kHeadDim) return fail(ecode, "%s: head_dim %ld (only 128)", name, a->D);
    if (a->B < 0 || a->Sk < 0 || a->H <= 0) return fail(LWM_EINVAL, "%s: bad dimension", name);
    if (!(a->scale > 0.0f)) return fail(LWM_EINVAL, "%s: scale must be > 0", name);
    if ((r = kvq_check_cache(name, ecode, head_bytes, scales_f32, row_align, a))) return r;
    if (a->B == 0) return LWM_OK;
    P p;
    p.q = (const bf16_t*)a->q.ptr; p.q_sb = a->q.stride_b; p.q_sh = a->q.stride_h;
    p.k = (const uint8_t*)a->k; p.v = (const uint8_t*)a->v;
    p.k_scale = (const typename F::scale_t*)a->k_scale; p.v_scale = (const typename F::scale_t*)a->v_scale;
    p.k_sb = a->k_stride_b; p.k_ss = a->k_stride_s; p.k_sh = a->k_stride_h;
    p.v_sb = a->v_stride_b; p.v_ss = a->v_stride_s; p.v_sh = a->v_stride_h;
    p.ks_sb = a->k_scale_stride_b; p.ks_ss = a->k_scale_stride_s;
    p.vs_sb = a->v_scale_stride_b; p.vs_ss = a->v_scale_stride_s;
    p.dense_mask = a->dense_mask; p.msk_sb = a->mask_stride_b;
    p.B = a->B; p.Sk = a->Sk; p.H = a->H; p.k_splits = a->k_splits > 1 ? a->k_splits : 1;
    p.scale = a->scale; p.out_acc = a->out_acc; p.lse_acc = a->lse_acc;
    return launch(name, kernel, (long)p.B * p.k_splits, kDecThreads, kDecqLdsBytes<F>, stream, p);
}

// The block kernels over the quantised caches (attn_prefill_kv8.h, attn_prefill_kv6.h; P = KvqPrefillParams<scale type>):
// both entries refuse a head_dim and an alignment with LWM_EUNSUPPORTED (the kv6 DECODE entry returns LWM_EINVAL).
template <class P, class Args>
static int kvq_attn_prefill(const char* name, void (*kernel)(P), int head_bytes, bool scales_f32, int row_align, const Args* a,
                            void* stream) {
    if (!a) return fail(LWM_EINVAL, "%s: args is null", name);
    int r;
    if ((r = check_t4("q", a->q, true))) return r;
    if (a->D != kHeadDim) return fail(LWM_EUNSUPPORTED, "%s: head_dim %ld (only 128)", name, a->D);
    if (a->B < 0 || a->Sq < 1 || a->Sk < 1 || a->H <= 0 || a->q_start < 0)
        return fail(LWM_EINVAL, "%s: bad dimension (B >= 0, Sq >= 1, Sk >= 1, H >= 1, q_start >= 0)", name);
    if (!(a->scale > 0.0f)) return fail(LWM_EINVAL, "%s: scale must be > 0", name);
    if ((r = kvq_check_cache(name, LWM_EUNSUPPORTED, head_bytes, scales_f32, row_align, a))) return r;
    if (a->B == 0) return LWM_OK;
    P p;
    memset(&p, 0, sizeof(p));
    p.a.q = (const bf16_t*)a->q.ptr; p.a.q_sb = a->q.stride_b; p.a.q_ss = a->q.stride_s; p.a.q_sh = a->q.stride_h;
    p.a.out_acc = a->out_acc; p.a.lse_acc = a->lse_acc; p.a.key_valid = a->key_valid;
    p.a.B = a->B; p.a.H = a->H; p.a.Sq = a->Sq; p.a.Sk = a->Sk;
    p.a.q_start = a->q_start; p.a.k_start = 0; p.a.q_np = 1; p.a.k_np = 1;
    p.a.scale = a->scale; p.a.causal = 1; p.a.carry_in = 0; p.a.final_out = 0;
    p.a.k_splits = a->k_splits > 1 ? a->k_splits : 1;
    p.k = (const uint8_t*)a->k; p.v = (const uint8_t*)a->v;
    p.k_scale = (decltype(p.k_scale))a->k_scale; p.v_scale = (decltype(p.v_scale))a->v_scale;
    p.k_sb = a->k_stride_b; p.k_ss = a->k_stride_s; p.k_sh = a->k_stride_h;
    p.v_sb = a->v_stride_b; p.v_ss = a->v_stride_s; p.v_sh = a->v_stride_h;
    p.ks_sb = a->k_scale_stride_b; p.ks_ss = a->k_scale_stride_s;
    p.vs_sb = a->v_scale_stride_b; p.vs_ss = a->v_scale_stride_s;
    p.kv_sb = a->key_valid_stride_b;
    const long nqt = (p.a.Sq + kFwdBQ - 1) / kFwdBQ;
    return launch(name, kernel, nqt * p.a.H * p.a.B * p.a.k_splits, kFwdThreads, kFwdLdsBytes, stream, p);
}

}  // namespace lwm

extern "C" {

int lwm_attn_fwd(const LwmAttnArgs* a, void* stream) {
    using namespace lwm;
    int r;
    if ((r = check_common(a))) return r;
    if (a->final_out) {
        if ((r = check_t4("out", a->out, true))) return r;
        if (!a->lse) return fail(LWM_EINVAL, "%s", "fwd: final_out needs lse");
    } else if (!a->out_acc || !a->lse_acc) {
        return fail(LWM_EINVAL, "%s", "fwd: final_out=0 needs out_acc and lse_acc");
    }
    if (a->carry_in && (!a->out_acc || !a->lse_acc))
        return fail(LWM_EINVAL, "%s", "fwd: carry_in needs out_acc and lse_acc");
    if (a->out_acc && !aligned16(a->out_acc)) return fail(LWM_EINVAL, "%s", "out_acc misaligned");
    if (a->B == 0 || a->Sq == 0) return LWM_OK;
    AttnParams p = to_params(a);
    long nqt = (p.Sq + kFwdBQ - 1) / kFwdBQ;
    if (p.k_splits > 1 && (a->final_out || a->carry_in))
        return fail(LWM_EINVAL, "%s", "fwd: k_splits > 1 needs final_out = 0 and carry_in = 0");
    if (p.k_splits > 4096) return fail(LWM_EINVAL, "%s", "fwd: k_splits too large");
    if ((a->q_pieces > 1 || a->k_pieces > 1) && (p.dense_mask || p.k_splits > 1 || (p.Sq == 1 && !a->final_out && !a->carry_in)))
        return fail(LWM_EUNSUPPORTED, "%s", "fwd: piecewise position maps are for the training kernel (no dense_mask, no k_splits, no decode)");
    // decode: one query per batch row, no other mask source -> streaming GEMV kernel
    if (p.Sq == 1 && !a->final_out && !a->carry_in && !p.causal && !p.seg_q && !p.key_valid)
        return launch("attn_decode", attn_decode_kernel, (long)p.B * p.k_splits, kDecThreads, 64, stream, p);
    if (p.dense_mask || p.k_splits > 1)
        return launch("attn_fwd_infer", attn_fwd_infer_kernel, nqt * p.H * p.B * p.k_splits, kFwdThreads,
                      kFwdLdsBytes, stream, p);
    // training path: one wave per SIMD, 64 query rows per wave (attn_fwd64.h); the variant with key meta only
    // when a key can be masked for another reason than causality
    const bool meta = p.seg_k || p.key_valid || (p.Sk % kF4BK) != 0;
    if (meta)
        return launch("attn_fwd64_meta", attn_fwd64_meta_kernel, nqt * p.H * p.B, kF4Threads, kF4LdsBytes, stream, p);
    return launch("attn_fwd64", attn_fwd64_kernel, nqt * p.H * p.B, kF4Threads, kF4LdsBytes, stream, p);
}

int lwm_attn_segment_blocks(const int32_t* segment_ids, const uint8_t* valid, int32_t* blocks,
                            int32_t B, int32_t S, void* stream) {
    using namespace lwm;
    if (!segment_ids || !blocks) return fail(LWM_EINVAL, "%s", "segment_blocks: null pointer");
    if (B < 0 || S < 0) return fail(LWM_EINVAL, "%s", "segment_blocks: bad dimension");
    if (B == 0 || S == 0) return LWM_OK;
    const long n = (long)B * ((S + 31) / 32);
    return launch("seg_blocks", seg_blocks_kernel, (n + 255) / 256, 256, 0, stream, segment_ids, valid, blocks,
                  (int)B, (int)S);
}

int lwm_attn_combine(const float* o_parts, const float* lse_parts, int32_t P, LwmTensor4 out,
                     float* out_f32, float* lse, int32_t B, int32_t Sq, int32_t H, int32_t D,
                     void* stream) {
    using namespace lwm;
    if (!o_parts || !lse_parts) return fail(LWM_EINVAL, "%s", "combine: null partials");
    if (P <= 0 || B < 0 || Sq < 0 || H <= 0 || D <= 0 || (D & 3)) return fail(LWM_EINVAL, "%s", "combine: bad dimension");
    if (D != kHeadDim) return fail(LWM_EUNSUPPORTED, "%s: head_dim %ld (only 128)", "combine", D);
    if (!out.ptr && !out_f32) return fail(LWM_EINVAL, "%s", "combine: no output");
    int r;
    if (out.ptr && (r = check_t4("out", out, true))) return r;
    if (!aligned16(o_parts) || (out_f32 && !aligned16(out_f32))) return fail(LWM_EINVAL, "%s", "combine: misaligned");
    if (B == 0 || Sq == 0) return LWM_OK;
    CombineParams p;
    p.o_parts = o_parts; p.lse_parts = lse_parts; p.out = (bf16_t*)out.ptr;
    p.o_sb = out.stride_b; p.o_ss = out.stride_s; p.o_sh = out.stride_h;
    p.out_f32 = out_f32; p.lse = lse; p.P = P; p.B = B; p.Sq = Sq; p.H = H; p.D = D;
    long blocks = (long)((int64_t)B * Sq * H);
    if (blocks > 65536) blocks = 65536;
    return launch("attn_combine", attn_combine_kernel, blocks, kCombineThreads, kCombineSubs * 32 * 32, stream, p);
}

int lwm_kv_cache_write(void* cache, const void* src, int32_t B, int64_t cache_stride_b,
                       int64_t src_stride_b, int64_t dst_row0, int64_t src_row0, int64_t nrows,
                       int32_t row_elems, void* stream) {
    using namespace lwm;
    if (!cache || !src) return fail(LWM_EINVAL, "%s", "kv_cache_write: null pointer");
    if (B < 0 || nrows < 0 || row_elems <= 0 || (row_elems & 7) || dst_row0 < 0 || src_row0 < 0 ||
        (cache_stride_b & 7) || (src_stride_b & 7))
        return fail(LWM_EINVAL, "%s", "kv_cache_write: bad dimension (rows are multiples of 8 bf16)");
    if (!aligned16(cache) || !aligned16(src)) return fail(LWM_EINVAL, "%s", "kv_cache_write: misaligned");
    if (B == 0 || nrows == 0) return LWM_OK;
    long blocks = (long)(((int64_t)B * nrows * (row_elems / 8) + 255) / 256);
    if (blocks > 16384) blocks = 16384;
    return launch("kv_cache_write", kv_cache_write_kernel, blocks, 256, 0, stream, (bf16_t*)cache,
                  (const bf16_t*)src, (int)B, cache_stride_b, src_stride_b, dst_row0, src_row0, nrows,
                  (int)row_elems);
}

int lwm_kv_cache_write_at(void* cache, const void* src, int32_t B, int64_t cache_stride_b,
                          int64_t src_stride_b, const int32_t* dst_row0_dev, int64_t row_offset,
                          int64_t cache_rows, int64_t src_row0, int64_t nrows, int32_t row_elems,
                          void* stream) {
    using namespace lwm;
    if (!cache || !src || !dst_row0_dev) return fail(LWM_EINVAL, "%s", "kv_cache_write_at: null pointer");
    if (B < 0 || nrows < 0 || row_elems <= 0 || (row_elems & 7) || cache_rows < 0 || src_row0 < 0 ||
        (cache_stride_b & 7) || (src_stride_b & 7))
        return fail(LWM_EINVAL, "%s", "kv_cache_write_at: bad dimension (rows are multiples of 8 bf16)");
    if (!aligned16(cache) || !aligned16(src)) return fail(LWM_EINVAL, "%s", "kv_cache_write_at: misaligned");
    if (B == 0 || nrows == 0) return LWM_OK;
    long blocks = (long)(((int64_t)B * nrows * (row_elems / 8) + 255) / 256);
    if (blocks > 16384) blocks = 16384;
    return launch("kv_cache_write_at", kv_cache_write_at_kernel, blocks, 256, 0, stream, (bf16_t*)cache,
                  (const bf16_t*)src, (int)B, cache_stride_b, src_stride_b, dst_row0_dev, row_offset,
                  cache_rows, src_row0, nrows, (int)row_elems);
}

static const char kKv8WriteAlign[] = "cache and src rows 16-byte aligned, scale 4-byte";
static const char kKv4WriteAlign[] = "src rows 16-byte aligned, cache and scale rows 4-byte";
static const char kKv6WriteAlign[] = "src rows 16-byte aligned, cache rows 8-byte, scale rows 4-byte";

int lwm_kv8_cache_write(void* cache, const void* src, int32_t B, int64_t cache_stride_b,
                        int64_t src_stride_b, int64_t dst_row0, int64_t src_row0, int64_t nrows,
                        int32_t row_elems, float* scale, int64_t scale_stride_b, int32_t H, void* stream) {
    return lwm::kvq_cache_write("kv8_cache_write", "kv8_quant_write", lwm::kv8_quant_write_kernel, false, LWM_EUNSUPPORTED, 16,
                                           1, kKv8WriteAlign, cache, src, B, cache_stride_b, src_stride_b, nullptr, dst_row0, 0,
                                           src_row0, nrows, row_elems, scale, scale_stride_b, H, stream);
}

int lwm_kv8_cache_write_at(void* cache, const void* src, int32_t B, int64_t cache_stride_b,
                           int64_t src_stride_b, const int32_t* dst_row0_dev, int64_t row_offset,
                           int64_t cache_rows, int64_t src_row0, int64_t nrows, int32_t row_elems,
                           float* scale, int64_t scale_stride_b, int32_t H, void* stream) {
    return lwm::kvq_cache_write("kv8_cache_write_at", "kv8_quant_write_at", lwm::kv8_quant_write_at_kernel, true, LWM_EUNSUPPORTED,
                                           16, 1, kKv8WriteAlign, cache, src, B, cache_stride_b, src_stride_b, dst_row0_dev, row_offset,
                                           cache_rows, src_row0, nrows, row_elems, scale, scale_stride_b, H, stream);
}

int lwm_kv4_cache_write(void* cache, const void* src, int32_t B, int64_t cache_stride_b,
                        int64_t src_stride_b, int64_t dst_row0, int64_t src_row0, int64_t nrows,
                        int32_t row_elems, void* scale, int64_t scale_stride_b, int32_t H, void* stream) {
    return lwm::kvq_cache_write("kv4_cache_write", "kv4_quant_write", lwm::kv4_quant_write_kernel, false, LWM_EINVAL, 4, 4,
                                           kKv4WriteAlign, cache, src, B, cache_stride_b, src_stride_b, nullptr, dst_row0, 0, src_row0,
                                           nrows, row_elems, scale, scale_stride_b, H, stream);
}

int lwm_kv4_cache_write_at(void* cache, const void* src, int32_t B, int64_t cache_stride_b,
                           int64_t src_stride_b, const int32_t* dst_row0_dev, int64_t row_offset,
                           int64_t cache_rows, int64_t src_row0, int64_t nrows, int32_t row_elems,
                           void* scale, int64_t scale_stride_b, int32_t H, void* stream) {
    return lwm::kvq_cache_write("kv4_cache_write_at", "kv4_quant_write_at", lwm::kv4_quant_write_at_kernel, true, LWM_EINVAL, 4, 4,
                                           kKv4WriteAlign, cache, src, B, cache_stride_b, src_stride_b, dst_row0_dev, row_offset,
                                           cache_rows, src_row0, nrows, row_elems, scale, scale_stride_b, H, stream);
}

int lwm_attn_decode_kv8(const LwmKv8DecodeArgs* a, void* stream) {
    return lwm::kvq_attn_decode<lwm::Kv8Format>("attn_decode_kv8", lwm::attn_decode_kv8_kernel, LWM_EUNSUPPORTED, 0, true, 16, a, stream);
}

int lwm_attn_decode_kv4(const LwmKv4DecodeArgs* a, void* stream) {
    return lwm::kvq_attn_decode<lwm::Kv4Format>("attn_decode_kv4", lwm::attn_decode_kv4_kernel, LWM_EINVAL, 64, false, 16, a, stream);
}

int lwm_kv6_cache_write(void* cache, const void* src, int32_t B, int64_t cache_stride_b,
                        int64_t src_stride_b, int64_t dst_row0, int64_t src_row0, int64_t nrows,
                        int32_t row_elems, void* scale, int64_t scale_stride_b, int32_t H, void* stream) {
    return lwm::kvq_cache_write("kv6_cache_write", "kv6_quant_write", lwm::kv6_quant_write_kernel, false, LWM_EINVAL, 8, 4,
                                           kKv6WriteAlign, cache, src, B, cache_stride_b, src_stride_b, nullptr, dst_row0, 0, src_row0,
                                           nrows, row_elems, scale, scale_stride_b, H, stream);
}

int lwm_kv6_cache_write_at(void* cache, const void* src, int32_t B, int64_t cache_stride_b,
                           int64_t src_stride_b, const int32_t* dst_row0_dev, int64_t row_offset,
                           int64_t cache_rows, int64_t src_row0, int64_t nrows, int32_t row_elems,
                           void* scale, int64_t scale_stride_b, int32_t H, void* stream) {
    return lwm::kvq_cache_write("kv6_cache_write_at", "kv6_quant_write_at", lwm::kv6_quant_write_at_kernel, true, LWM_EINVAL, 8, 4,
                                           kKv6WriteAlign, cache, src, B, cache_stride_b, src_stride_b, dst_row0_dev, row_offset,
                                           cache_rows, src_row0, nrows, row_elems, scale, scale_stride_b, H, stream);
}

int lwm_attn_decode_kv6(const LwmKv6DecodeArgs* a, void* stream) {
    return lwm::kvq_attn_decode<lwm::Kv6Format>("attn_decode_kv6", lwm::attn_decode_kv6_kernel, LWM_EINVAL, 96, false, 8, a, stream);
}

int lwm_attn_prefill_kv6(const LwmKv6PrefillArgs* a, void* stream) {
    return lwm::kvq_attn_prefill("attn_prefill_kv6", lwm::attn_prefill_kv6_kernel, 96, false, 8, a, stream);
}

int lwm_attn_prefill_kv8(const LwmKv8PrefillArgs* a, void* stream) {
    return lwm::kvq_attn_prefill("attn_prefill_kv8", lwm::attn_prefill_kv8_kernel, 0, true, 16, a, stream);
}

static int check_bwd(const LwmAttnArgs* a) {
    using namespace lwm;
    int r;
    if ((r = check_common(a))) return r;
    if ((r = check_t4("dout", a->dout, true))) return r;
    if (!a->lse) return fail(LWM_EINVAL, "%s", "bwd: lse is null");
    if (!a->delta) return fail(LWM_EINVAL, "%s", "bwd: delta is null");
    if (a->delta_bytes && a->delta_bytes < lwm_attn_bwd_delta_bytes(a->B, a->H, a->Sq))
        return fail(LWM_EINVAL, "%s: delta holds %ld bytes, lwm_attn_bwd_delta_bytes(B,H,Sq) asks for %ld", "bwd", (long)a->delta_bytes,
                    (long)lwm_attn_bwd_delta_bytes(a->B, a->H, a->Sq));
    return 0;
}

int lwm_attn_bwd_delta(const LwmAttnArgs* a, void* stream) {
    using namespace lwm;
    if (!a) return fail(LWM_EINVAL, "%s", "args is null");
    if (a->D != kHeadDim) return fail(LWM_EUNSUPPORTED, "%s: head_dim %ld (only 128)", "delta", a->D);
    int r;
    if ((r = check_t4("out", a->out, true))) return r;
    if ((r = check_t4("dout", a->dout, true))) return r;
    if (!a->delta) return fail(LWM_EINVAL, "%s", "delta is null");
    if (!a->lse) return fail(LWM_EINVAL, "%s", "delta: lse is null (the statistics carry -lse * log2 e)");
    if (a->delta_bytes && a->delta_bytes < lwm_attn_bwd_delta_bytes(a->B, a->H, a->Sq))
        return fail(LWM_EINVAL, "%s: the buffer holds %ld bytes, lwm_attn_bwd_delta_bytes(B,H,Sq) asks for %ld", "delta", (long)a->delta_bytes,
                    (long)lwm_attn_bwd_delta_bytes(a->B, a->H, a->Sq));
    if (a->B <= 0 || a->H <= 0 || a->Sq <= 0) return LWM_OK;
    AttnParams p = to_params(a);
    long rows = (long)((int64_t)p.B * p.H * bwd_stat_pad(p.Sq));
    long blocks = (rows + (kDeltaThreads / 16) - 1) / (kDeltaThreads / 16);
    if (blocks > 8192) blocks = 8192;
    return launch("attn_bwd_delta", attn_bwd_delta_kernel, blocks, kDeltaThreads, 0, stream, p, a->delta);
}

// dS hand-over (attn_bwd64.h): 1 = this call takes it, 0 = it runs as without a workspace, < 0 = refused
static int ds_handover(const char* who, const LwmAttnArgs* a) {
    using namespace lwm;
    if (!a->ds_ws) return 0;
    if (a->segment_ids_k || a->key_valid || !a->final_out || a->carry_in || a->q_pieces > 1 || a->k_pieces > 1) return 0;
    const int64_t need = lwm_attn_bwd_ds_bytes(a->B, a->H, a->Sq, a->Sk, a->causal, a->q_start, a->k_start);
    if (need == 0) return 0;
    if (!aligned16(a->ds_ws)) return fail(LWM_EINVAL, "%s: ds_ws is not 16-byte aligned", who);
    if (a->ds_ws_bytes < need)
        return fail(LWM_EINVAL, "%s: ds_ws holds %ld bytes, lwm_attn_bwd_ds_bytes asks for %ld", who, (long)a->ds_ws_bytes, (long)need);
    return 1;
}

int lwm_attn_bwd_dq(const LwmAttnArgs* a, void* stream) {
    using namespace lwm;
    int r;
    if ((r = check_bwd(a))) return r;
    if (a->final_out) {
        if ((r = check_t4("dq", a->dq, true))) return r;
    } else if (!a->dq_acc) {
        return fail(LWM_EINVAL, "%s", "bwd_dq: final_out=0 needs dq_acc");
    }
    if (a->carry_in && !a->dq_acc) return fail(LWM_EINVAL, "%s", "bwd_dq: carry_in needs dq_acc");
    if (a->B == 0 || a->Sq == 0) return LWM_OK;
    AttnParams p = to_params(a);
    if ((r = ds_handover("bwd_dq", a)) < 0) return r;
    if (r) {      // dq = scale * dS k from the dS the dK/dV kernel left in the workspace: 64 queries per wave
        p.ds_ws = (char*)a->ds_ws;
        const long nqb = (p.Sq + kS4BQ - 1) / kS4BQ;
        return launch("attn_bwd_dq_ds", attn_bwd_dq_ds_kernel, nqb * p.H * p.B, kD4Threads, kS4LdsBytes, stream, p);
    }
    // one wave per SIMD, 32 queries per wave (attn_bwd64.h); the variant with key meta when a key can be masked for
    // another reason than causality (segments, padded keys, a ragged last 64-key step)
    const long nqb = (p.Sq + kQ4BQ - 1) / kQ4BQ;
    if (p.seg_k || p.key_valid || (p.Sk % kQ4BK) != 0)
        return launch("attn_bwd_dq4_meta", attn_bwd_dq4_meta_kernel, nqb * p.H * p.B, kD4Threads, kQ4LdsBytes, stream, p);
    return launch("attn_bwd_dq4", attn_bwd_dq4_kernel, nqb * p.H * p.B, kD4Threads, kQ4LdsBytes, stream, p);
}

int lwm_attn_bwd_dkdv(const LwmAttnArgs* a, void* stream) {
    using namespace lwm;
    int r;
    if ((r = check_bwd(a))) return r;
    if (a->final_out) {
        if ((r = check_t4("dk", a->dk, true))) return r;
        if ((r = check_t4("dv", a->dv, true))) return r;
    } else if (!a->dk_acc || !a->dv_acc) {
        return fail(LWM_EINVAL, "%s", "bwd_dkdv: final_out=0 needs dk_acc and dv_acc");
    }
    if (a->carry_in && (!a->dk_acc || !a->dv_acc))
        return fail(LWM_EINVAL, "%s", "bwd_dkdv: carry_in needs dk_acc and dv_acc");
    if (a->B == 0 || a->Sk == 0) return LWM_OK;
    AttnParams p = to_params(a);
    // one wave per SIMD, 32 keys per wave (attn_bwd64.h); the variant with key meta only when a key can be masked
    // for another reason than causality
    const long nkb = (p.Sk + kD4BK - 1) / kD4BK;
    if ((r = ds_handover("bwd_dkdv", a)) < 0) return r;
    if (r) {
        p.ds_ws = (char*)a->ds_ws;
        return launch("attn_bwd_dkdv4_ds", attn_bwd_dkdv4_ds_kernel, nkb * p.H * p.B, kD4Threads, kD4LdsBytes, stream, p);
    }
    if (p.seg_k || p.key_valid)
        return launch("attn_bwd_dkdv4_meta", attn_bwd_dkdv4_meta_kernel, nkb * p.H * p.B, kD4Threads, kD4LdsBytes, stream, p);
    return launch("attn_bwd_dkdv4", attn_bwd_dkdv4_kernel, nkb * p.H * p.B, kD4Threads, kD4LdsBytes, stream, p);
}

int64_t lwm_attn_bwd_delta_bytes(int32_t B, int32_t H, int32_t Sq) {
    if (B <= 0 || H <= 0 || Sq <= 0) return 0;
    return (int64_t)B * H * 2 * lwm::bwd_stat_pad(Sq) * (int64_t)sizeof(float);
}

int64_t lwm_attn_bwd_ds_bytes(int32_t B, int32_t H, int32_t Sq, int32_t Sk, int32_t causal, int64_t q_start, int64_t k_start) {
    using namespace lwm;
    if (B <= 0 || H <= 0 || Sq <= 0 || Sk <= 0 || (Sq % kD4BQ) || (Sk % kD4BK)) return 0;
    return ds_ws_bytes(B, H, Sq, Sk, causal ? 1 : 0, q_start, k_start);
}

int lwm_cast_f32_to_bf16(const float* src, void* dst, int64_t n, void* stream) {
    using namespace lwm;
    if (n < 0) return fail(LWM_EINVAL, "%s", "cast: n < 0");
    if (n == 0) return LWM_OK;
    if (!src || !dst) return fail(LWM_EINVAL, "%s", "cast: null pointer");
    if (!aligned16(src) || !aligned16(dst)) return fail(LWM_EINVAL, "%s", "cast: misaligned");
    long blocks = (long)((n / 8 + kCastThreads - 1) / kCastThreads);
    if (blocks < 1) blocks = 1;
    if (blocks > 4096) blocks = 4096;
    return launch("cast_f32_to_bf16", cast_f32_to_bf16_kernel, blocks, kCastThreads, 0, stream, src,
                  (bf16_t*)dst, n);
}

int lwm_sum_f32_to_bf16(const float* const* srcs, int32_t n_src, void* dst, int64_t n, void* stream) {
    using namespace lwm;
    if (n < 0) return fail(LWM_EINVAL, "%s", "sum: n < 0");
    if (n_src < 1 || n_src > kSumMaxSrc) return fail(LWM_EINVAL, "sum%s: n_src=%ld not in [1,%ld]", "", (long)n_src, (long)kSumMaxSrc);
    if (n == 0) return LWM_OK;
    if (!srcs || !dst) return fail(LWM_EINVAL, "%s", "sum: null pointer");
    if (!aligned16(dst)) return fail(LWM_EINVAL, "%s", "sum: misaligned dst");
    SumSrcs ss = {};
    for (int i = 0; i < n_src; ++i) {
        if (!srcs[i] || !aligned16(srcs[i])) return fail(LWM_EINVAL, "sum%s: source %ld null or misaligned", "", (long)i);
        ss.p[i] = srcs[i];
    }
    long blocks = (long)((n / 8 + kCastThreads - 1) / kCastThreads);
    if (blocks < 1) blocks = 1;
    if (blocks > 4096) blocks = 4096;
    return launch("sum_f32_to_bf16", sum_f32_to_bf16_kernel, blocks, kCastThreads, 0, stream, ss, (int)n_src,
                  (bf16_t*)dst, n);
}

int lwm_rope_bf16(LwmTensor4 x, LwmTensor4 y, const float* table, const int32_t* pos, int32_t B,
                  int32_t S, int32_t H, int32_t D, int32_t max_pos, int32_t conj, void* stream) {
    using namespace lwm;
    int r;
    if ((r = check_t4("x", x, true))) return r;
    if ((r = check_t4("y", y, true))) return r;
    if (!table || !pos) return fail(LWM_EINVAL, "%s", "rope: null table / positions");
    if (B < 0 || S < 0 || H <= 0 || D <= 0 || (D & 7) || max_pos <= 0) return fail(LWM_EINVAL, "%s", "rope: bad dimension");
    if (!aligned16(table)) return fail(LWM_EINVAL, "%s", "rope: table misaligned");
    if (B == 0 || S == 0) return LWM_OK;
    RopeParams p;
    p.x = (const bf16_t*)x.ptr; p.y = (bf16_t*)y.ptr; p.table = table; p.pos = pos;
    p.x_sb = x.stride_b; p.x_ss = x.stride_s; p.x_sh = x.stride_h;
    p.y_sb = y.stride_b; p.y_ss = y.stride_s; p.y_sh = y.stride_h;
    p.B = B; p.S = S; p.H = H; p.D = D; p.max_pos = max_pos; p.conj = conj ? 1 : 0;
    long blocks = (long)(((int64_t)B * S * H * (D / 8) + 255) / 256);
    if (blocks > 65536) blocks = 65536;
    return launch("rope", rope_kernel, blocks, 256, 0, stream, p);
}

static long rms_blocks(int64_t rows) { return (long)(rows < 2048 ? rows : 2048); }

int lwm_rmsnorm_fwd_bf16(const void* x, const void* w, void* y, float* rstd, int64_t rows, int32_t C,
                         float eps, void* stream) {
    using namespace lwm;
    if (!x || !w || !y) return fail(LWM_EINVAL, "%s", "rmsnorm: null pointer");
    if (rows < 0 || C <= 0 || (C & 7) || C > 8192) return fail(LWM_EUNSUPPORTED, "%s: C=%ld (need C%%8==0, C<=8192)", "rmsnorm", C);
    if (!aligned16(x) || !aligned16(w) || !aligned16(y)) return fail(LWM_EINVAL, "%s", "rmsnorm: misaligned");
    if (rows == 0) return LWM_OK;
    RmsParams p;
    memset(&p, 0, sizeof(p));
    p.x = (const bf16_t*)x; p.w = (const bf16_t*)w; p.y = (bf16_t*)y; p.rstd = rstd;
    p.rows = rows; p.C = C; p.eps = eps;
    long blocks = rows < 65536 ? (long)rows : 65536;
    return launch("rmsnorm_fwd", rmsnorm_fwd_kernel, blocks, 256, 16, stream, p);
}

int64_t lwm_rmsnorm_bwd_workspace_bytes(int64_t rows, int32_t C) {
    if (rows <= 0 || C <= 0) return 0;
    return (int64_t)rms_blocks(rows) * C * (int64_t)sizeof(float);
}

int lwm_rmsnorm_bwd_res_bf16(const void* x, const void* w, const void* g, const float* rstd, const void* res,
                             void* dx, void* dw, void* workspace, int64_t rows, int32_t C, void* stream) {
    using namespace lwm;
    if (!x || !w || !g || !rstd || !dx || !dw || !workspace) return fail(LWM_EINVAL, "%s", "rmsnorm_bwd: null pointer");
    if (rows <= 0 || C <= 0 || (C & 7) || C > 8192) return fail(LWM_EUNSUPPORTED, "%s: C=%ld", "rmsnorm_bwd", C);
    if (!aligned16(x) || !aligned16(w) || !aligned16(g) || !aligned16(dx) || !aligned16(workspace) || !aligned16(res))
        return fail(LWM_EINVAL, "%s", "rmsnorm_bwd: misaligned");
    RmsParams p;
    memset(&p, 0, sizeof(p));
    p.x = (const bf16_t*)x; p.w = (const bf16_t*)w; p.g = (const bf16_t*)g; p.y = (bf16_t*)dx;
    p.res = (const bf16_t*)res;
    p.rstd = (float*)rstd; p.dw_part = (float*)workspace; p.rows = rows; p.C = C;
    const long nblk = rms_blocks(rows);
    int r = launch("rmsnorm_bwd", rmsnorm_bwd_kernel, nblk, 256, 16, stream, p);
    if (r) return r;
    return launch("rmsnorm_dw_reduce", rmsnorm_dw_reduce_kernel, (C + 31) / 32, 256, 8 * 32 * 4, stream,
                  (const float*)workspace, (bf16_t*)dw, (int)nblk, (int)C);
}

int lwm_rmsnorm_bwd_bf16(const void* x, const void* w, const void* g, const float* rstd, void* dx,
                         void* dw, void* workspace, int64_t rows, int32_t C, void* stream) {
    return lwm_rmsnorm_bwd_res_bf16(x, w, g, rstd, nullptr, dx, dw, workspace, rows, C, stream);
}

// how the tiles of a (K, N) weight gradient are split over the device: whole rounds of one tile per CU, the rest stream-K
static void wgrad_plan(int64_t S, int64_t K, int64_t N, lwm::WgradParams& p) {
    using namespace lwm;
    p.S = (int32_t)S; p.K = (int32_t)K; p.N = (int32_t)N;
    p.tiles_m = (int32_t)(K / kWgBM); p.tiles_n = (int32_t)(N / kWgBN);
    p.nst = (int32_t)(S / kWgBK);
    const long cus = device_cu_count(), tiles = (long)p.tiles_m * p.tiles_n;
    p.direct_tiles = (int32_t)(tiles / cus * cus);
    const long rest = tiles - p.direct_tiles;
    p.sk_blocks = rest ? (int32_t)cus : 0;
    p.sk_q = rest ? (int32_t)((rest * p.nst + cus - 1) / cus) : 0;
}

int64_t lwm_wgrad_workspace_bytes(int64_t S, int64_t K, int64_t N) {
    using namespace lwm;
    if (S <= 0 || K <= 0 || N <= 0 || (S % kWgBK) || (K % kWgBM) || (N % kWgBN)) return 0;
    WgradParams p;
    wgrad_plan(S, K, N, p);
    return (int64_t)2 * p.sk_blocks * kWgTileFloats * 4;
}

int lwm_wgrad_bf16(const void* x, int64_t ldx, const void* g, int64_t ldg, void* dw, int64_t lddw, int64_t S, int64_t K,
                   int64_t N, void* workspace, int64_t workspace_bytes, void* stream) {
    using namespace lwm;
    if (!x || !g || !dw) return fail(LWM_EINVAL, "%s", "wgrad: null pointer");
    if (S <= 0 || K <= 0 || N <= 0 || (S % kWgBK) || (K % kWgBM) || (N % kWgBN) || S > 0x7fffffff || K > 0x7fffffff || N > 0x7fffffff)
        return fail(LWM_EUNSUPPORTED, "%s: S %% 32, K %% 256, N %% 256 must be 0 (K=%ld N=%ld)", "wgrad", (long)K, (long)N);
    if (ldx < K || ldg < N || lddw < N || (ldx & 7) || (ldg & 7) || !aligned16(x) || !aligned16(g) || ((uintptr_t)dw & 1) ||
        (int64_t)kWgBK * (ldx > ldg ? ldx : ldg) * 2 > 0x7fffffff)
        return fail(LWM_EINVAL, "%s", "wgrad: leading dimensions must cover a row and be multiples of 8; 16-byte aligned operands");
    WgradParams p;
    p.x = (const bf16_t*)x; p.g = (const bf16_t*)g; p.dw = (bf16_t*)dw; p.ldx = ldx; p.ldg = ldg; p.lddw = lddw;
    wgrad_plan(S, K, N, p);
    p.ws = (float*)workspace;
    if (p.sk_blocks && (!workspace || !aligned16(workspace) || workspace_bytes < (int64_t)2 * p.sk_blocks * kWgTileFloats * 4))
        return fail(LWM_EINVAL, "%s: workspace of lwm_wgrad_workspace_bytes() = %ld bytes needed", "wgrad",
                    (long)((int64_t)2 * p.sk_blocks * kWgTileFloats * 4));
    // Two waves per SIMD, 64 x 128 each (default), or LWM_WGRAD_WAVES=4: one wave per SIMD, 128 x 128 each -- a third fewer
    // fragment reads per MFMA, but every stall of the only wave is the matrix pipe's: 3 % behind (profiles/r06_wgrad.md)
    const char* wv = getenv("LWM_WGRAD_WAVES");
    const int waves = wv && atoi(wv) == 4 ? 4 : 8;
    const long rest = (long)p.tiles_m * p.tiles_n - p.direct_tiles;
    int rc;
    if (waves == 8) {
        rc = launch("wgrad_bf16", wgrad_bf16_kernel<8>, (long)p.direct_tiles + p.sk_blocks, 512, kWgLdsBytes, stream, p);
        if (rc || !p.sk_blocks) return rc;
        return launch("wgrad_fixup", wgrad_fixup_kernel<8>, rest, 512, kWgLdsBytes, stream, p);
    }
    rc = launch("wgrad_bf16", wgrad_bf16_kernel<4>, (long)p.direct_tiles + p.sk_blocks, 256, kWgLdsBytes, stream, p);
    if (rc || !p.sk_blocks) return rc;
    return launch("wgrad_fixup", wgrad_fixup_kernel<4>, rest, 256, kWgLdsBytes, stream, p);
}

int lwm_transpose_bf16(const void* src, int64_t ld_src, void* dst, int64_t ld_dst, int64_t rows, int64_t cols,
                       void* stream) {
    using namespace lwm;
    if (!src || !dst) return fail(LWM_EINVAL, "%s", "transpose: null pointer");
    if (rows < 0 || cols < 0 || (rows & 63) || (cols & 63) || rows > ((int64_t)1 << 36) || cols > ((int64_t)1 << 36))
        return fail(LWM_EUNSUPPORTED, "%s: rows=%ld cols=%ld (multiples of 64)", "transpose", (long)rows, (long)cols);
    if (ld_src < cols || ld_dst < rows || (ld_src & 7) || (ld_dst & 7) || !aligned16(src) || !aligned16(dst))
        return fail(LWM_EINVAL, "%s", "transpose: leading dimensions must cover a row and be multiples of 8; 16-byte aligned bases");
    if (rows == 0 || cols == 0) return LWM_OK;
    TransposeParams p;
    p.src = (const bf16_t*)src; p.dst = (bf16_t*)dst; p.ld_src = ld_src; p.ld_dst = ld_dst;
    p.tiles_r = (int32_t)(rows / 64); p.tiles_c = (int32_t)(cols / 64);
    int64_t tiles = (int64_t)p.tiles_r * p.tiles_c;
    long blocks = (long)(tiles < 16384 ? tiles : 16384);
    return launch("transpose_bf16", transpose_bf16_kernel, blocks, 256, 64 * kTrPitchWords * 4, stream, p);
}

static int swiglu_check(const char* what, int64_t n, const void* p0, const void* p1, const void* p2) {
    using namespace lwm;
    if (!p0 || !p1 || !p2) return fail(LWM_EINVAL, "%s: null pointer", what);
    if (n < 0 || (n & 7)) return fail(LWM_EINVAL, "%s: n must be a non-negative multiple of 8", what);
    if (!aligned16(p0) || !aligned16(p1) || !aligned16(p2)) return fail(LWM_EINVAL, "%s: misaligned", what);
    return 0;
}

int lwm_swiglu_fwd_bf16(const void* a, const void* b, void* y, int64_t n, void* stream) {
    using namespace lwm;
    int r;
    if ((r = swiglu_check("swiglu_fwd", n, a, b, y))) return r;
    if (n == 0) return LWM_OK;
    long blocks = (long)((n / 8 + 255) / 256);
    if (blocks > 65536) blocks = 65536;
    return launch("swiglu_fwd", swiglu_fwd_kernel, blocks, 256, 0, stream, (const bf16_t*)a, (const bf16_t*)b,
                  (bf16_t*)y, n);
}

int lwm_swiglu_bwd_bf16(const void* a, const void* b, const void* g, void* da, void* db, int64_t n,
                        void* stream) {
    using namespace lwm;
    int r;
    if ((r = swiglu_check("swiglu_bwd", n, a, b, g))) return r;
    if ((r = swiglu_check("swiglu_bwd", n, da, db, g))) return r;
    if (n == 0) return LWM_OK;
    long blocks = (long)((n / 8 + 255) / 256);
    if (blocks > 65536) blocks = 65536;
    return launch("swiglu_bwd", swiglu_bwd_kernel, blocks, 256, 0, stream, (const bf16_t*)a, (const bf16_t*)b,
                  (const bf16_t*)g, (bf16_t*)da, (bf16_t*)db, n);
}

static int swiglu_ld_check(const char* what, int64_t rows, int64_t cols, const void* const* ptrs, const int64_t* lds, int n) {
    using namespace lwm;
    if (rows < 0 || cols < 0 || (cols & 7) || cols > 0x7fffffff) return fail(LWM_EINVAL, "%s: cols must be a non-negative multiple of 8", what);
    for (int i = 0; i < n; ++i) {
        if (!ptrs[i]) return fail(LWM_EINVAL, "%s: null pointer", what);
        if (!aligned16(ptrs[i]) || (lds[i] & 7) || lds[i] < cols) return fail(LWM_EINVAL, "%s: misaligned base or leading dimension", what);
    }
    return 0;
}

int lwm_swiglu_fwd_ld_bf16(const void* a, int64_t lda, const void* b, int64_t ldb, void* y, int64_t ldy, int64_t rows,
                           int64_t cols, void* stream) {
    using namespace lwm;
    const void* ptrs[3] = {a, b, y};
    const int64_t lds[3] = {lda, ldb, ldy};
    int r;
    if ((r = swiglu_ld_check("swiglu_fwd_ld", rows, cols, ptrs, lds, 3))) return r;
    if (rows == 0 || cols == 0) return LWM_OK;
    SwigluLdParams p;
    memset(&p, 0, sizeof(p));
    p.a = (const bf16_t*)a; p.b = (const bf16_t*)b; p.y = (bf16_t*)y; p.lda = lda; p.ldb = ldb; p.ldy = ldy;
    p.rows = rows; p.cols = (int32_t)cols;
    long blocks = (long)((rows * (cols / 8) + 255) / 256);
    if (blocks > 65536) blocks = 65536;
    return launch("swiglu_fwd_ld", swiglu_fwd_ld_kernel, blocks, 256, 0, stream, p);
}

int lwm_swiglu_bwd_ld_bf16(const void* a, int64_t lda, const void* b, int64_t ldb, const void* g, int64_t ldg, void* da,
                           int64_t ldda, void* db, int64_t lddb, int64_t rows, int64_t cols, void* stream) {
    using namespace lwm;
    const void* ptrs[5] = {a, b, g, da, db};
    const int64_t lds[5] = {lda, ldb, ldg, ldda, lddb};
    int r;
    if ((r = swiglu_ld_check("swiglu_bwd_ld", rows, cols, ptrs, lds, 5))) return r;
    if (rows == 0 || cols == 0) return LWM_OK;
    SwigluLdParams p;
    memset(&p, 0, sizeof(p));
    p.a = (const bf16_t*)a; p.b = (const bf16_t*)b; p.g = (const bf16_t*)g; p.da = (bf16_t*)da; p.db = (bf16_t*)db;
    p.lda = lda; p.ldb = ldb; p.ldg = ldg; p.ldda = ldda; p.lddb = lddb; p.rows = rows; p.cols = (int32_t)cols;
    long blocks = (long)((rows * (cols / 8) + 255) / 256);
    if (blocks > 65536) blocks = 65536;
    return launch("swiglu_bwd_ld", swiglu_bwd_ld_kernel, blocks, 256, 0, stream, p);
}

int64_t lwm_gemv_workspace_bytes(int32_t rows, int32_t K, int32_t N) {
    if (rows <= 0 || K <= 0 || N <= 0) return 0;
    return (int64_t)((K + lwm::kGemvKT - 1) / lwm::kGemvKT) * rows * N * (int64_t)sizeof(float);
}

}  // extern "C"
namespace lwm {
// The seven fused projection entries (gemv.h, gemv_w8.h, gemv_w4.h, gemv_w6.h, gemm_rows.h) share their checks, the K partition of GemvParams and
// the launch pair with gemv_reduce_kernel.  What differs per entry is written down here.
struct ProjEntry {
    const char* tag;           // opens every text of lwm_last_error()
    const char* kname;         // the streaming kernel, as launch() names it
    int max_rows;
    bool zero_rows_ok;         // no rows: LWM_OK and nothing is launched (else below the range)
    int nt;                    // columns of W per workgroup
    bool x16;                  // x and norm_weight are read 16 bytes at a time (else by the element)
    bool one_res;              // a residual needs a single matrix (else it belongs to its matrix)
    bool gemv_texts;           // the GEMV entries' wording of the range refusal, and their ss_out text with "%%" as they print it
    bool names_scales;         // the null-matrix refusal names the scale table (the rows entries do in both formats)
    int lds_fixed, lds_per_row;        // dynamic LDS of the streaming kernel: LDS per workgroup is occupancy, so not levelled
};

static const void* const* proj_scales(const LwmGemvArgs*) { return nullptr; }
static const void* const* proj_scales(const LwmGemvW8Args* a) { return (const void* const*)a->w_scale; }
static const void* const* proj_scales(const LwmGemvW4Args* a) { return (const void* const*)a->w_scale; }
static const void* const* proj_scales(const LwmGemvW6Args* a) { return (const void* const*)a->w_scale; }
static const GemvParams& proj_params(void (*)(GemvParams), const GemvW8Params& pp) { return pp.g; }
static const GemvW8Params& proj_params(void (*)(GemvW8Params), const GemvW8Params& pp) { return pp; }
static GemvW4Params proj_params(void (*)(GemvW4Params), const GemvW8Params& pp) {      // (the same pointers, typed as bytes; GemvW6Params too)
    GemvW4Params p4;
    p4.g = pp.g;
    for (int i = 0; i < kGemvMaxMats; ++i) { p4.q[i] = pp.q[i]; p4.scale[i] = (const uint8_t*)pp.scale[i]; }
    return p4;
}

// A = LwmGemvArgs with a kernel over GemvParams, or LwmGemvW8Args / LwmGemvW4Args / LwmGemvW6Args with a kernel over
// GemvW8Params / GemvW4Params = GemvW6Params (scale tables exist).
// The checks run in the order every entry has run them; the texts are format strings over the tag.
template <class A, class P>
static int proj_run(const ProjEntry& e, void (*kernel)(P), const A* a, void* stream) {
    static_assert(kRowsThreads == kGemvThreads, "one workgroup size");
    const char* who = e.tag;
    if (!a) return fail(LWM_EINVAL, "%s: args is null", who);
    const void* const* w_scale = proj_scales(a);
    const bool w8 = w_scale != nullptr;
    const int32_t nmat = a->nmat, rows = a->rows, K = a->K;
    if (!a->x || !a->workspace) return fail(LWM_EINVAL, "%s: null pointer", who);
    if (nmat < 1 || nmat > kGemvMaxMats) return fail(LWM_EINVAL, "%s: 1..3 matrices per call", who);
    if (rows < 0 || K <= 0) return fail(LWM_EINVAL, "%s: bad dimension", who);
    if ((rows < 1 && !e.zero_rows_ok) || rows > e.max_rows || (K & 31) || K > 8 * 12 * kGemvKT)
        return fail(LWM_EUNSUPPORTED, e.gemv_texts ? "%s: rows=%ld K=%ld (need rows <= 4, K %% 32 == 0, K <= 12288)"
                                                   : "%s: rows=%ld K=%ld (need 1 <= rows <= 32, K %% 32 == 0, K <= 12288)", who, rows, K);
    if (!aligned16(a->workspace) || a->ldx < K || (e.x16 && (!aligned16(a->x) || (a->ldx & 7))))
        return fail(LWM_EINVAL, e.x16 ? "%s: misaligned workspace or x, or bad ldx (need ldx >= K, ldx %% 8 == 0)"
                                      : "%s: misaligned workspace or bad ldx", who);
    if (a->norm_weight && ((e.x16 && !aligned16(a->norm_weight)) || !a->ss_in || a->ss_n < 1 || a->ss_n > 64 || !(a->eps >= 0.0f)))
        return fail(LWM_EINVAL, e.x16 ? "%s: norm_weight needs 16-byte alignment, ss_in with 1..64 partials per row and eps >= 0"
                                      : "%s: norm_weight needs ss_in with 1..64 partials per row and eps >= 0", who);
    if (a->ss_out && (nmat != 1 || !a->y[0] || (a->N[0] % kGemvSsCols)))
        return fail(LWM_EINVAL, e.gemv_texts ? "%s: ss_out needs one matrix with a bf16 output and N %%%% 128 == 0"
                                             : "%s: ss_out needs one matrix with a bf16 output and N %% 128 == 0", who);
    GemvW8Params pp;
    memset(&pp, 0, sizeof(pp));
    GemvParams& p = pp.g;
    p.x = (const bf16_t*)a->x; p.part = (float*)a->workspace; p.ldx = a->ldx; p.R = rows; p.K = K; p.nmat = nmat;
    p.KS = (K + kGemvKT - 1) / kGemvKT;
    p.gamma = (const bf16_t*)a->norm_weight; p.ss_in = a->ss_in; p.ss_n = a->ss_n; p.eps = a->eps; p.ss_out = a->ss_out;
    int64_t off = 0;
    long grid = 0, quads = 0;
    for (int i = 0; i < nmat; ++i) {
        const int32_t n = a->N[i];
        float* yf = a->y_f32[i];
        void* yb = a->y[i];
        if (!a->w[i] || (w8 && !w_scale[i]) || (!yb && !yf))
            return fail(LWM_EINVAL, e.names_scales ? "%s: null matrix, null scale table or no output" : "%s: null matrix or no output", who);
        if (n <= 0 || (n & 7)) return fail(LWM_EUNSUPPORTED, "%s: N=%ld (need N %% 8 == 0)", who, n);
        if (!aligned16(a->w[i]) || (w8 && !aligned16(w_scale[i])) || (yf && !aligned16(yf)) ||
            (yb && ((((uintptr_t)yb) & 7) || (a->ldy[i] & 3) || a->ldy[i] < n)))
            return fail(LWM_EINVAL, "%s: misaligned pointer or bad leading dimension", who);
        if (a->residual[i] && ((e.one_res && nmat != 1) || !yb || (((uintptr_t)a->residual[i]) & 7) || (a->ldres[i] & 3) || a->ldres[i] < n))
            return fail(LWM_EINVAL, e.one_res ? "%s: a residual needs one matrix with a bf16 output, 8-byte alignment and ldres >= N, a multiple of 4"
                                              : "%s: a residual needs a bf16 output, 8-byte alignment and ldres >= N, a multiple of 4", who);
        if (w8) { pp.q[i] = (const uint8_t*)a->w[i]; pp.scale[i] = (const float*)w_scale[i]; }
        else p.w[i] = (const bf16_t*)a->w[i];
        p.y[i] = (bf16_t*)yb; p.y_f32[i] = yf; p.ldy[i] = yb ? a->ldy[i] : 0; p.N[i] = n;
        p.res[i] = (const bf16_t*)a->residual[i]; p.ldres[i] = a->ldres[i];
        p.part_off[i] = off;
        off += (int64_t)p.KS * rows * n;
        p.blk0[i] = (int32_t)grid;
        p.quad0[i] = (int32_t)quads;
        grid += (long)p.KS * ((n + e.nt - 1) / e.nt);
        quads += (long)rows * (n >> 2);
    }
    p.blk0[nmat] = (int32_t)grid;
    p.quad0[nmat] = (int32_t)quads;
    if (rows == 0) return LWM_OK;
    int r = launch(e.kname, kernel, grid, kGemvThreads, (size_t)(e.lds_fixed + rows * e.lds_per_row), stream, proj_params(kernel, pp));
    if (r) return r;
    return launch("gemv_reduce", gemv_reduce_kernel, (quads * 8 + 255) / 256, 256, 64, stream, p);
}

static const ProjEntry kProjGemv = {"gemv", "gemv_bf16", kGemvMaxRows, true, kGemvNT, false, false, true, false,
                                    3 * kGemvMaxRows * kGemvNT * 4, 0};
static const ProjEntry kProjGemvW8 = {"gemv_w8", "gemv_w8", kGemvMaxRows, true, kGemvW8NT, false, false, true, true,
                                      0, 3 * kGemvW8NT * 4};
static const ProjEntry kProjGemvW4 = {"gemv_w4", "gemv_w4", kGemvMaxRows, true, kGemvNT, false, false, true, true,
                                      0, 3 * kGemvNT * 4};
static const ProjEntry kProjGemvW6 = {"gemv_w6", "gemv_w6", kGemvMaxRows, true, kGemvNT, false, false, true, true,
                                      0, 3 * kGemvNT * 4};
static const ProjEntry kProjRows = {"gemm_rows", "gemm_rows_bf16", kRowsMax, false, kRowsNT, true, true, false, true,
                                    kRowsLdsBytes, 0};
static const ProjEntry kProjRowsW8 = {"gemm_rows_w8", "gemm_rows_w8", kRowsMax, false, kRowsNT, true, true, false, true,
                                      kRowsLdsBytes, 0};
static const ProjEntry kProjRowsW6 = {"gemm_rows_w6", "gemm_rows_w6", kRowsMax, false, kRowsNT, true, true, false, true,
                                      kRowsLdsBytes, 0};

// lwm_w8_quantise / lwm_w4_quantise / lwm_w6_quantise: the checks, the params, the grid and the launch.  P = the kernel's
// params (w, q, scale, rounded, K, N); n_div = the columns one lane converts, nt = the columns of one workgroup.
template <typename P, typename S>
static int weight_quantise(const char* tag, int n_div, int nt, size_t lds_bytes, void (*kernel)(P), const void* w, void* q, S* scale,
                           void* rounded, int32_t K, int32_t N, void* stream) {
    if (!w || !q || !scale || !rounded) return fail(LWM_EINVAL, "%s: null pointer", tag);
    if (K <= 0 || N <= 0) return fail(LWM_EINVAL, "%s: bad dimension", tag);
    if ((K & 31) || K > 8 * 12 * kGemvKT || (N % n_div))
        return fail(LWM_EUNSUPPORTED, "%s: K=%ld N=%ld (need K %% 32 == 0, K <= 12288, N %% 8 == 0)", tag, K, N);
    if (!aligned16(w) || !aligned16(q) || !aligned16(scale) || !aligned16(rounded)) return fail(LWM_EINVAL, "%s: misaligned pointer", tag);
    P p;
    p.w = (const bf16_t*)w; p.q = (uint8_t*)q; p.scale = scale; p.rounded = (bf16_t*)rounded; p.K = K; p.N = N;
    const long grid = (long)((K + kGemvKT - 1) / kGemvKT) * ((N + nt - 1) / nt);
    return launch(tag, kernel, grid, 256, lds_bytes, stream, p);
}
}  // namespace lwm
extern "C" {

int lwm_gemv_fused_bf16(const LwmGemvArgs* a, void* stream) { return lwm::proj_run(lwm::kProjGemv, lwm::gemv_bf16_kernel, a, stream); }

int lwm_gemv_multi_bf16(const void* x, int64_t ldx, int32_t nmat, const void* const* w, void* const* y, const int64_t* ldy,
                        float* const* y_f32, const int32_t* N, void* workspace, int32_t rows, int32_t K, void* stream) {
    using namespace lwm;
    if (!x || !w || !N || !workspace || (!y && !y_f32)) return fail(LWM_EINVAL, "%s", "gemv: null pointer");
    if (nmat < 1 || nmat > kGemvMaxMats) return fail(LWM_EINVAL, "%s", "gemv: 1..3 matrices per call");
    LwmGemvArgs a;
    memset(&a, 0, sizeof(a));
    a.x = x; a.ldx = ldx; a.nmat = nmat; a.workspace = workspace; a.rows = rows; a.K = K;
    for (int i = 0; i < nmat; ++i) {
        a.w[i] = w[i];
        a.y[i] = y ? y[i] : nullptr;
        if (a.y[i] && !ldy) return fail(LWM_EINVAL, "%s", "gemv: misaligned pointer or bad leading dimension");
        a.ldy[i] = (y && ldy) ? ldy[i] : 0;
        a.y_f32[i] = y_f32 ? y_f32[i] : nullptr;
        a.N[i] = N[i];
    }
    return lwm_gemv_fused_bf16(&a, stream);
}

int lwm_gemv_bf16(const void* x, int64_t ldx, const void* w, void* y, int64_t ldy, float* y_f32, void* workspace,
                  int32_t rows, int32_t K, int32_t N, void* stream) {
    return lwm_gemv_multi_bf16(x, ldx, 1, &w, y ? &y : nullptr, &ldy, y_f32 ? &y_f32 : nullptr, &N, workspace, rows, K, stream);
}

int lwm_w8_quantise(const void* w, void* q, float* scale, void* rounded, int32_t K, int32_t N, void* stream) {
    return lwm::weight_quantise("w8_quantise", lwm::kGemvW8CPL, lwm::kW8QuantNT, 4 * 64 * 32, lwm::w8_quantise_kernel, w, q, scale, rounded, K, N, stream);
}

int lwm_gemv_fused_w8(const LwmGemvW8Args* a, void* stream) { return lwm::proj_run(lwm::kProjGemvW8, lwm::gemv_w8_kernel, a, stream); }

int lwm_w4_quantise(const void* w, void* q, void* scale_e8m0, void* rounded, int32_t K, int32_t N, void* stream) {
    return lwm::weight_quantise("w4_quantise", 8, lwm::kW4QuantNT, 0, lwm::w4_quantise_kernel, w, q, (uint8_t*)scale_e8m0, rounded, K, N, stream);
}

int lwm_gemv_fused_w4(const LwmGemvW4Args* a, void* stream) { return lwm::proj_run(lwm::kProjGemvW4, lwm::gemv_w4_kernel, a, stream); }

int lwm_w6_quantise(const void* w, void* q, void* scale_e8m0, void* rounded, int32_t K, int32_t N, void* stream) {
    return lwm::weight_quantise("w6_quantise", 8, lwm::kW4QuantNT, 0, lwm::w6_quantise_kernel, w, q, (uint8_t*)scale_e8m0, rounded, K, N, stream);
}

int lwm_gemv_fused_w6(const LwmGemvW6Args* a, void* stream) { return lwm::proj_run(lwm::kProjGemvW6, lwm::gemv_w6_kernel, a, stream); }

// 1..32 rows on the matrix pipe (gemm_rows.h)
int64_t lwm_gemm_rows_workspace_bytes(int32_t rows, int32_t K, int32_t N) { return lwm_gemv_workspace_bytes(rows, K, N); }

int lwm_gemm_rows_fused_bf16(const LwmGemvArgs* a, void* stream) { return lwm::proj_run(lwm::kProjRows, lwm::gemm_rows_bf16_kernel, a, stream); }

int lwm_gemm_rows_fused_w8(const LwmGemvW8Args* a, void* stream) { return lwm::proj_run(lwm::kProjRowsW8, lwm::gemm_rows_w8_kernel, a, stream); }

int lwm_gemm_rows_fused_w6(const LwmGemvW6Args* a, void* stream) { return lwm::proj_run(lwm::kProjRowsW6, lwm::gemm_rows_w6_kernel, a, stream); }

int lwm_softmax_ce_bf16(const void* logits, const int32_t* target, const float* weight, float* nll,
                        int32_t* correct, void* dlogits, int64_t rows, int32_t V, void* stream) {
    using namespace lwm;
    if (!logits || !target || !nll) return fail(LWM_EINVAL, "%s", "softmax_ce: null pointer");
    if (rows < 0 || V <= 0 || (V & 7) || V > 32768)
        return fail(LWM_EUNSUPPORTED, "%s: V=%ld (need V%%8==0, V<=32768)", "softmax_ce", V);
    if (!aligned16(logits) || (dlogits && !aligned16(dlogits))) return fail(LWM_EINVAL, "%s", "softmax_ce: misaligned");
    if (rows == 0) return LWM_OK;
    CeParams p;
    p.logits = (const bf16_t*)logits; p.target = target; p.weight = weight; p.nll = nll; p.correct = correct;
    p.dlogits = (bf16_t*)dlogits; p.rows = rows; p.V = V;
    long blocks = rows < 65536 ? (long)rows : 65536;
    return launch("softmax_ce", softmax_ce_kernel, blocks, kCeThreads, 128, stream, p);
}

int lwm_sample_tokens(const LwmSampleArgs* a, void* stream) {
    using namespace lwm;
    if (!a) return fail(LWM_EINVAL, "%s", "sample_tokens: args is null");
    if (!a->logits) return fail(LWM_EINVAL, "%s", "sample_tokens: logits is null");
    if (a->V < 1 || a->V > (1 << 30)) return fail(LWM_EINVAL, "%s: V = %ld (need 1 <= V <= 2^30)", "sample_tokens", a->V);
    if (a->rows < 1 || a->ld < a->V) return fail(LWM_EINVAL, "%s: rows = %ld, ld = %ld (need rows >= 1, ld >= V)", "sample_tokens", a->rows, (long)a->ld);
    if (a->top_k < 0) return fail(LWM_EINVAL, "%s: top_k = %ld < 0", "sample_tokens", a->top_k);
    if (!(a->temperature >= 0.0f)) return fail(LWM_EINVAL, "%s", "sample_tokens: temperature must be >= 0 (0 = greedy)");
    if (!(a->top_p >= 0.0f)) return fail(LWM_EINVAL, "%s", "sample_tokens: top_p must be >= 0 (0 or >= 1 = no filter)");
    if (a->cfg_scale && (a->rows & 1))
        return fail(LWM_EINVAL, "%s: rows = %ld is odd (cfg_scale: conditional rows, then as many unconditional ones)", "sample_tokens", a->rows);
    const int32_t B = a->cfg_scale ? a->rows / 2 : a->rows;
    if (B > 65535) return fail(LWM_EINVAL, "%s: %ld output rows (at most 65535)", "sample_tokens", B);
    if (!a->tokens && !a->seq) return fail(LWM_EINVAL, "%s", "sample_tokens: no output (tokens and seq are both null)");
    if (a->tokens && a->copies < 1) return fail(LWM_EINVAL, "%s: copies = %ld < 1", "sample_tokens", a->copies);
    if (a->seq && (a->seq_cols < 0 || a->seq_ld < a->seq_cols)) return fail(LWM_EINVAL, "%s", "sample_tokens: bad seq_cols / seq_ld");
    if (a->force_period < 0) return fail(LWM_EINVAL, "%s: force_period = %ld < 0", "sample_tokens", a->force_period);
    const auto mis = [](const void* p, uintptr_t n) { return ((uintptr_t)p & (n - 1)) != 0; };
    if (mis(a->logits, 4) || mis(a->cfg_scale, 4) || mis(a->step_dev, 4) || mis(a->tokens, 8) || mis(a->seq, 8))
        return fail(LWM_EINVAL, "%s", "sample_tokens: misaligned pointer (logits, cfg_scale, step_dev: 4 bytes; tokens, seq: 8)");
    SampleParams p;
    p.logits = a->logits; p.ld = a->ld; p.V = a->V; p.B = B; p.cfg = a->cfg_scale != nullptr; p.cfg_scale = a->cfg_scale;
    p.temperature = a->temperature; p.top_k = a->top_k; p.top_p = a->top_p;
    p.key0 = (uint32_t)a->seed; p.key1 = (uint32_t)(a->seed >> 32);
    p.step_dev = a->step_dev; p.step_base = a->step_base; p.step = a->step;
    p.force_period = a->force_period; p.force_token = a->force_token;
    p.done = a->done; p.eos = a->eos; p.pad = a->pad;
    p.tokens = a->tokens; p.copies = a->copies;
    p.seq = a->seq; p.seq_ld = a->seq_ld; p.seq_cols = a->seq_cols;
    // the top-p phase is a kernel of its own (with its mass tables in LDS): a launch with top-p off runs the code it ran
    // before the phase existed
    if (a->temperature > 0.0f && a->top_p > 0.0f && a->top_p < 1.0f)
        return launch("sample_tokens", sample_top_p_kernel, B, kSampleThreads, kSampleTopPLdsBytes, stream, p);
    return launch("sample_tokens", sample_kernel, B, kSampleThreads, kSampleLdsBytes, stream, p);
}

// the arguments both AdamW entries share, checked before any launch; -> the kernel's parameters
static int adamw_params(const char* name, const LwmAdamWArgs* a, lwm::AdamWParams* p) {
    using namespace lwm;
    if (!a) return fail(LWM_EINVAL, "%s: args is null", name);
    if (a->n_tensors < 0 || a->n_chunks < 0) return fail(LWM_EINVAL, "%s: n_tensors = %ld, n_chunks = %ld (need >= 0)", name, (long)a->n_tensors, (long)a->n_chunks);
    if (a->n_chunks > 0 && (!a->tensors || !a->chunks || a->n_tensors == 0))
        return fail(LWM_EINVAL, "%s: null tensor table or chunk table", name);
    if (!(a->lr >= 0.0) || !isfinite(a->lr)) return fail(LWM_EINVAL, "%s: lr must be finite and >= 0", name);
    if (!(a->eps >= 0.0) || !isfinite(a->eps)) return fail(LWM_EINVAL, "%s: eps must be finite and >= 0", name);
    if (!(a->weight_decay >= 0.0) || !isfinite(a->weight_decay)) return fail(LWM_EINVAL, "%s: weight_decay must be finite and >= 0", name);
    if (!(a->beta1 >= 0.0 && a->beta1 < 1.0) || !(a->beta2 >= 0.0 && a->beta2 < 1.0))
        return fail(LWM_EINVAL, "%s: beta1 and beta2 must lie in [0, 1)", name);
    if (a->max_norm != a->max_norm) return fail(LWM_EINVAL, "%s: max_norm is NaN", name);
    if (!a->norms || !a->grad_partials || !a->param_partials) return fail(LWM_EINVAL, "%s: null norms or partials workspace", name);
    if (a->grad_partials_len < a->n_chunks || a->param_partials_len < a->n_chunks)
        return fail(LWM_EINVAL, "%s: a partials workspace is smaller than the chunk count %ld", name, (long)a->n_chunks);
    if ((((uintptr_t)a->tensors | (uintptr_t)a->grad_partials | (uintptr_t)a->param_partials) & 7) ||
        (((uintptr_t)a->chunks | (uintptr_t)a->norms) & 3))
        return fail(LWM_EINVAL, "%s: misaligned pointer (tensors, partials: 8 bytes; chunks, norms: 4)", name);
    memset(p, 0, sizeof(*p));
    p->tensors = a->tensors; p->chunks = a->chunks; p->n_tensors = a->n_tensors; p->n_chunks = a->n_chunks;
    p->norms = a->norms;
    p->lr = (float)a->lr; p->beta1 = (float)a->beta1; p->om_beta1 = (float)(1.0 - a->beta1);
    p->beta2 = (float)a->beta2; p->om_beta2 = (float)(1.0 - a->beta2); p->eps = (float)a->eps;
    p->decay = (float)(1.0 - a->lr * a->weight_decay);
    return 0;
}

static long adamw_blocks(int32_t n_chunks) { return n_chunks < lwm::kAdamWMaxBlocks ? n_chunks : lwm::kAdamWMaxBlocks; }

int lwm_adamw_grad_norm(const LwmAdamWArgs* a, void* stream) {
    using namespace lwm;
    AdamWParams p;
    int r;
    if ((r = adamw_params("adamw_grad_norm", a, &p))) return r;
    p.partials = a->grad_partials;
    if ((r = launch("adamw_grad_sq", adamw_grad_sq_kernel, adamw_blocks(p.n_chunks), kAdamWThreads, kAdamWLdsBytes, stream, p))) return r;
    return launch("adamw_grad_norm", adamw_norm_kernel, 1, kNormThreads, kAdamWLdsBytes, stream, (const double*)a->grad_partials,
                  p.n_chunks, a->norms, (int32_t)0, (float)a->max_norm);
}

int lwm_adamw_step(const LwmAdamWArgs* a, void* stream) {
    using namespace lwm;
    AdamWParams p;
    int r;
    if ((r = adamw_params("adamw_step", a, &p))) return r;
    p.partials = a->param_partials;
    if ((r = launch("adamw_update", adamw_update_kernel, adamw_blocks(p.n_chunks), kAdamWThreads, kAdamWLdsBytes, stream, p))) return r;
    return launch("adamw_param_norm", adamw_norm_kernel, 1, kNormThreads, kAdamWLdsBytes, stream, (const double*)a->param_partials,
                  p.n_chunks, a->norms, (int32_t)2, 0.0f);
}

int lwm_adamw_chunk(void) { return lwm::kAdamWChunk; }

// ---------------------------------------------------------------- dropout (dropout.h)
// the checks of the four entries, in the order include/lwm_hip.h lists them; -> the kernel's parameters
static int dropout_params(const char* name, const LwmDropoutArgs* a, bool with_res, lwm::DropoutParams* p) {
    using namespace lwm;
    if (!a) return fail(LWM_EINVAL, "%s: args is null", name);
    if (!a->x || !a->y) return fail(LWM_EINVAL, "%s: x or y is null", name);
    if (a->B < 0 || a->S < 0 || a->C < 0) return fail(LWM_EINVAL, "%s: negative dimension", name);
    if (a->s_offset < 0 || a->s_offset + a->S > ((int64_t)1 << 32))
        return fail(LWM_EINVAL, "%s: s_offset = %ld (need 0 <= s_offset and s_offset + S <= 2^32: a counter word)", name, (long)a->s_offset);
    if (a->C & 7) return fail(LWM_EINVAL, "%s: C = %ld is not a multiple of 8", name, (long)a->C);
    if (!aligned16(a->x) || !aligned16(a->y) || (with_res && !aligned16(a->res))) return fail(LWM_EINVAL, "%s: misaligned pointer", name);
    if (a->thr16 > 65535u) return fail(LWM_EINVAL, "%s: thr16 = %ld (at most 65535)", name, (long)a->thr16);
    if (!isfinite(a->inv) || !(a->inv >= 1.0f)) return fail(LWM_EINVAL, "%s: inv must be finite and >= 1", name);
    p->x = a->x; p->res = with_res ? a->res : nullptr; p->y = a->y;
    p->nvec = (int64_t)a->B * a->S * (a->C / 8);
    p->S = (uint32_t)a->S; p->Cv = (uint32_t)(a->C / 8);
    p->s_offset = (uint32_t)a->s_offset; p->site = a->site; p->key0 = a->key0; p->key1 = a->key1;
    p->thr16 = a->thr16; p->inv = a->inv;
    return 0;
}

static int dropout_launch(const char* name, const LwmDropoutArgs* a, bool f32, bool with_res, void* stream) {
    using namespace lwm;
    DropoutParams p;
    int r;
    if ((r = dropout_params(name, a, with_res, &p))) return r;
    if (p.nvec == 0) return LWM_OK;
    // a bounded grid of 256-vector tiles, 8 blocks per compute unit; the blocks stride over the rest
    const int64_t tiles = (p.nvec + 255) / 256, cap = 8 * device_cu_count();
    const long blocks = (long)(tiles < cap ? tiles : cap);
    if (f32) {
        if (p.res) return launch(name, dropout_kernel<true, true>, blocks, 256, 0, stream, p);
        return launch(name, dropout_kernel<true, false>, blocks, 256, 0, stream, p);
    }
    if (p.res) return launch(name, dropout_kernel<false, true>, blocks, 256, 0, stream, p);
    return launch(name, dropout_kernel<false, false>, blocks, 256, 0, stream, p);
}

int lwm_dropout_add_bf16(const LwmDropoutArgs* a, void* stream) { return dropout_launch("dropout_add_bf16", a, false, a && a->res, stream); }
int lwm_dropout_add_f32(const LwmDropoutArgs* a, void* stream) { return dropout_launch("dropout_add_f32", a, true, a && a->res, stream); }
// dx = dropout'(g): x = g, y = dx; `res` is not read (its gradient is g itself: no kernel)
int lwm_dropout_bwd_bf16(const LwmDropoutArgs* a, void* stream) { return dropout_launch("dropout_bwd_bf16", a, false, false, stream); }
int lwm_dropout_bwd_f32(const LwmDropoutArgs* a, void* stream) { return dropout_launch("dropout_bwd_f32", a, true, false, stream); }

const char* lwm_last_error(void) { return lwm::g_err; }
int lwm_version(void) { return 650; }
int lwm_sizeof(int which) {
    return which == 0 ? (int)sizeof(LwmAttnArgs) : which == 1 ? (int)sizeof(LwmConvArgs) : which == 2 ? (int)sizeof(LwmRingArgs) : which == 3 ? (int)sizeof(LwmGemvArgs) : which == 4 ? (int)sizeof(LwmSampleArgs) : which == 5 ? (int)sizeof(LwmKv8DecodeArgs) : which == 6 ? (int)sizeof(LwmKv8PrefillArgs) : which == 7 ? (int)sizeof(LwmAdamWArgs) : which == 8 ? (int)sizeof(LwmAdamWTensor) : which == 9 ? (int)sizeof(LwmGemvW8Args) : which == 10 ? (int)sizeof(LwmKv4DecodeArgs) : which == 11 ? (int)sizeof(LwmGemvW4Args) : which == 12 ? (int)sizeof(LwmFramesArgs) : which == 13 ? (int)sizeof(LwmKv6DecodeArgs) : which == 14 ? (int)sizeof(LwmKv6PrefillArgs) : which == 15 ? (int)sizeof(LwmGemvW6Args) : which == 16 ? (int)sizeof(LwmDropoutArgs) : -1;
}

}  // extern "C"
