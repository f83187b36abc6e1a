// optim.h -- the optimiser phase of a training step: the global gradient norm with its clipping coefficient, and the
// AdamW update on f32 master weights (f32 moments, an optional bf16 working copy written in the same pass), over a LIST
// of tensors in one launch per phase.  Two tables in device memory drive both phases: one LwmAdamWTensor per tensor,
// and a chunk table that cuts the tensors into pieces of kAdamWChunk elements -- (tensor, chunk of that tensor) pairs
// walked by a grid-stride loop, so the launch shape does not depend on how the parameters are split into tensors.
//
// Every sum is taken in a fixed order in f64 and there are no floating-point atomics: a chunk's partial depends on the
// chunk alone (not on the grid), the partials are summed by one workgroup in a fixed tree.  The same inputs give the
// same bits on every run and on every replica of a data-parallel job.
//
// The per-element arithmetic is f32 with one rounding per operation (no fused multiply-add), in the order that
// tests/_adamw_ref.py restates.
//
// Expects wave_ops.h (the product's or the host emulation's) and lwm_hip.h to be included first.
#pragma once

namespace lwm {

constexpr int kAdamWThreads = 256;
constexpr int kAdamWChunk = 8192;                    // elements of one chunk: 4 passes of 8 elements per thread
constexpr int kAdamWMaxBlocks = 2048;                // 8 workgroups per CU: 8 waves per SIMD in flight
constexpr int kNormThreads = 1024;
constexpr int kAdamWLdsBytes = 8 * (kNormThreads / 64);   // one f64 per wave (both kernels' reductions)
static_assert(kAdamWChunk % (8 * kAdamWThreads) == 0, "a full chunk is whole passes of 8 elements per thread");

struct AdamWParams {
    const LwmAdamWTensor* tensors;
    const int32_t* chunks;       // [n_chunks][2]: tensor, chunk of that tensor
    int32_t n_tensors, n_chunks;
    double* partials;            // [n_chunks]
    const float* norms;          // norms[1] = the clipping coefficient (phase B)
    float lr, beta1, om_beta1, beta2, om_beta2, eps, decay;
};

LWM_DEVICE double shfl_xor_f64(double x, int m) {
    const uint64_t u = __builtin_bit_cast(uint64_t, x);
    const uint32_t lo = (uint32_t)shfl_xor_i((int)(uint32_t)u, m), hi = (uint32_t)shfl_xor_i((int)(uint32_t)(u >> 32), m);
    return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}

// x summed over the workgroup in a fixed tree (butterfly over the lanes, then the waves in order); the sum is returned
// to thread 0 only.  Every thread of the workgroup must call it.
LWM_DEVICE double block_sum_f64(double x, lds_t lds, int tid, int n_waves) {
#pragma clang fp contract(off)
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x += shfl_xor_f64(x, m);
    if ((tid & 63) == 0) lds_write_f64(lds + 8 * (tid >> 6), x);
    block_sync();
    double s = 0.0;
    if (tid == 0)
        for (int w = 0; w < n_waves; ++w) s += lds_read_f64(lds + 8 * w);
    block_sync();            // the next sum writes the same words
    return s;
}

LWM_DEVICE float bf16_bits_to_f32(uint32_t b) { return __builtin_bit_cast(float, b << 16); }

// gradient entries [i, i + 8) as f32; i is a multiple of 8 and the base is 16-byte aligned: 16-byte loads
LWM_DEVICE void load_grad8(const void* g, bool bf16, int64_t i, float (&o)[8]) {
    if (bf16) {
        const u32x4 w = global_load_b128((const uint16_t*)g + i);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            o[2 * j] = bf16_bits_to_f32(w[j] & 0xffffu);
            o[2 * j + 1] = bf16_bits_to_f32(w[j] >> 16);
        }
    } else {
        const f32x4 a = global_load_f32x4((const float*)g + i), b = global_load_f32x4((const float*)g + i + 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            o[j] = a[j];
            o[4 + j] = b[j];
        }
    }
}
LWM_DEVICE float load_grad1(const void* g, bool bf16, int64_t i) {
    return bf16 ? bf16_bits_to_f32(((const uint16_t*)g)[i]) : ((const float*)g)[i];
}

// the chunk `c` of the table: its tensor, the offset of its first element and its length (0: an entry that names no
// element of any tensor -- skipped, nothing is read or written through it)
LWM_DEVICE int adamw_chunk(const AdamWParams& p, int c, const LwmAdamWTensor*& T, int64_t& off) {
    const int t = p.chunks[2 * c], ci = p.chunks[2 * c + 1];
    if (t < 0 || t >= p.n_tensors || ci < 0) return 0;
    T = p.tensors + t;
    off = (int64_t)ci * kAdamWChunk;
    const int64_t left = T->numel - off;
    return left <= 0 ? 0 : left < kAdamWChunk ? (int)left : kAdamWChunk;
}

// ---- phase A: partials[c] = sum of g^2 over chunk c, in f64
LWM_KERNEL(kAdamWThreads) void adamw_grad_sq_kernel(AdamWParams p) {
#pragma clang fp contract(off)
    const int tid = thread_idx();
    const lds_t lds = dyn_lds();
    for (int c = block_idx_x(); c < p.n_chunks; c += grid_dim_x()) {
        const LwmAdamWTensor* T = nullptr;
        int64_t off = 0;
        const int n = adamw_chunk(p, c, T, off);
        double acc = 0.0;
        if (n > 0) {
            const bool gb = T->grad_bf16 != 0;
            const void* const G = T->grad;
            const int n8 = n & ~7;
            for (int i = 8 * tid; i < n8; i += 8 * kAdamWThreads) {
                float g[8];
                load_grad8(G, gb, off + i, g);
#pragma unroll
                for (int j = 0; j < 8; ++j) acc += (double)g[j] * (double)g[j];
            }
            if (tid < n - n8) {          // the scalar tail of a tensor's last chunk
                const float g = load_grad1(G, gb, off + n8 + tid);
                acc += (double)g * (double)g;
            }
        }
        const double s = block_sum_f64(acc, lds, tid, kAdamWThreads / 64);
        if (tid == 0) p.partials[c] = s;
    }
}

// the scalars of one tensor's update
struct AdamWScalars {
    float coef, beta1, om_beta1, beta2, om_beta2, sqrt_bc2, eps, decay, step;
    bool decays;
};

// one element: clip, moments, decoupled decay, update -- every operation rounded on its own
LWM_DEVICE void adamw_elem(float& p, float& m, float& v, float g, const AdamWScalars& s) {
#pragma clang fp contract(off)
    g = g * s.coef;
    m = m * s.beta1 + g * s.om_beta1;
    v = v * s.beta2 + (g * g) * s.om_beta2;
    const float den = sqrtf(v) / s.sqrt_bc2 + s.eps;
    if (s.decays) p = p * s.decay;
    p = p - s.step * (m / den);
}

// ---- phase B: the update of every element of chunk c; partials[c] = sum of the new p^2, in f64
LWM_KERNEL(kAdamWThreads) void adamw_update_kernel(AdamWParams p) {
#pragma clang fp contract(off)
    const int tid = thread_idx();
    const lds_t lds = dyn_lds();
    AdamWScalars s;
    s.coef = p.norms[1];
    s.beta1 = p.beta1; s.om_beta1 = p.om_beta1; s.beta2 = p.beta2; s.om_beta2 = p.om_beta2;
    s.eps = p.eps; s.decay = p.decay;
    for (int c = block_idx_x(); c < p.n_chunks; c += grid_dim_x()) {
        const LwmAdamWTensor* T = nullptr;
        int64_t off = 0;
        const int n = adamw_chunk(p, c, T, off);
        double acc = 0.0;
        if (n > 0) {
            const bool gb = T->grad_bf16 != 0;
            s.decays = T->decay != 0;
            s.sqrt_bc2 = T->sqrt_bias_corr2;
            s.step = p.lr / T->bias_corr1;
            const void* const G = T->grad;
            float* const P = T->master + off;
            float* const M = T->exp_avg + off;
            float* const V = T->exp_avg_sq + off;
            uint16_t* const W = T->copy_bf16 ? (uint16_t*)T->copy_bf16 + off : nullptr;
            const int n8 = n & ~7;
            for (int i = 8 * tid; i < n8; i += 8 * kAdamWThreads) {
                float g[8];
                load_grad8(G, gb, off + i, g);
                f32x4 p4[2] = {global_load_f32x4(P + i), global_load_f32x4(P + i + 4)};
                f32x4 m4[2] = {global_load_f32x4(M + i), global_load_f32x4(M + i + 4)};
                f32x4 v4[2] = {global_load_f32x4(V + i), global_load_f32x4(V + i + 4)};
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    float pe = p4[j >> 2][j & 3], me = m4[j >> 2][j & 3], ve = v4[j >> 2][j & 3];
                    adamw_elem(pe, me, ve, g[j], s);
                    p4[j >> 2][j & 3] = pe; m4[j >> 2][j & 3] = me; v4[j >> 2][j & 3] = ve;
                    acc += (double)pe * (double)pe;
                }
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    global_store_f32x4(P + i + 4 * h, p4[h]);
                    global_store_f32x4(M + i + 4 * h, m4[h]);
                    global_store_f32x4(V + i + 4 * h, v4[h]);
                }
                if (W) {
                    u32x4 w;
#pragma unroll
                    for (int j = 0; j < 4; ++j) w[j] = pack_bf16x2(p4[j >> 1][2 * (j & 1)], p4[j >> 1][2 * (j & 1) + 1]);
                    global_store_b128(W + i, w);
                }
            }
            if (tid < n - n8) {          // the scalar tail of a tensor's last chunk
                const int i = n8 + tid;
                float pe = P[i], me = M[i], ve = V[i];
                adamw_elem(pe, me, ve, load_grad1(G, gb, off + i), s);
                P[i] = pe; M[i] = me; V[i] = ve;
                acc += (double)pe * (double)pe;
                if (W) W[i] = (uint16_t)(pack_bf16x2(pe, 0.0f) & 0xffffu);
            }
        }
        const double sum = block_sum_f64(acc, lds, tid, kAdamWThreads / 64);
        if (tid == 0) p.partials[c] = sum;
    }
}

// ---- one workgroup: the partials summed in a fixed order in f64, then
//   which = 0: norms[0] = the gradient norm, norms[1] = min(1, max_norm / (norm + 1e-6)) (1 when max_norm <= 0)
//   which = 2: norms[2] = the parameter norm
LWM_KERNEL(kNormThreads) void adamw_norm_kernel(const double* partials, int32_t n, float* norms, int32_t which, float max_norm) {
#pragma clang fp contract(off)
    const int tid = thread_idx();
    double acc = 0.0;
    for (int i = tid; i < n; i += kNormThreads) acc += partials[i];
    const double s = block_sum_f64(acc, dyn_lds(), tid, kNormThreads / 64);
    if (tid != 0) return;
    const float norm = (float)sqrt(s);
    if (which == 0) {
        norms[0] = norm;
        float coef = 1.0f;
        if (max_norm > 0.0f) {
            const float c = max_norm / (norm + 1e-6f);
            coef = c > 1.0f ? 1.0f : c;          // (a NaN norm stays a NaN coefficient, as torch's clamp keeps it)
        }
        norms[1] = coef;
    } else {
        norms[2] = norm;
    }
}

}  // namespace lwm
