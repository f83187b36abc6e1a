// sample.h -- the token sampler of the decode loop: classifier-free guidance, temperature, top-k, top-p and a categorical
// draw for one output row per workgroup (lwm/vision_llama.py:476-560 _sample_vision; lwm/vision_chat.py:201-213
// generate(do_sample=True)), with the bookkeeping of a decode step (forced end-of-frame code, done / pad, the next
// step's input ids) in the same launch.  The draw is Gumbel-max over a counter-based Philox4x32-10 stream keyed by
// (seed, entry, row, step): no host state, so a step that reads `step` from device memory can be captured in a
// hipGraph and replayed.  The token depends only on (logits, cfg, T, k, p, seed, row, step) -- not on the launch shape
// or on the order in which threads finish: every reduction is a fixed tree and every argmax breaks ties to the
// lowest index.
//
// Expects wave_ops.h (the product's or the host emulation's) to be included first.
#pragma once
#include "philox.h"      // philox4x32_10: the generator, shared with dropout.h

namespace lwm {

constexpr int kSampleThreads = 1024;
constexpr int kSampleWaves = kSampleThreads / 64;
// entries a lane keeps in registers, in groups of 4 consecutive ones (one Philox call each): V <= 32768 is read once;
// entries past that are re-read from memory by every pass
constexpr int kSampleGroups = 8;
// LDS: [waves][16] digit counts | [16] digit totals | [waves][2] argmax candidates
constexpr int kSampleLdsBytes = 4 * (kSampleWaves * 16 + 16 + kSampleWaves * 2);
// ... | [waves][16] digit masses | [16] digit mass totals (f64), behind the above: a launch with top-p on
constexpr int kSampleTopPLdsBytes = kSampleLdsBytes + 8 * (kSampleWaves * 16 + 16);

struct SampleParams {
    const float* logits;
    int64_t ld;
    int32_t V, B, cfg;           // cfg: rows [0, B) conditional, [B, 2B) unconditional, mixed by cfg_scale[b]
    const float* cfg_scale;
    float temperature;           // 0 = greedy
    int32_t top_k;               // 0 or >= V = no filter
    float top_p;                 // 0 < top_p < 1: the nucleus filter over the top-k survivors; else none
    uint32_t key0, key1;         // Philox key = the 64-bit seed
    const int32_t* step_dev;     // step = *step_dev - step_base, or `step` when null
    int32_t step_base, step;
    int32_t force_period, force_token;
    uint8_t* done;
    int64_t eos, pad;            // eos < 0: none
    int64_t* tokens;             // [copies][B] or null
    int32_t copies;
    int64_t* seq;                // [B][seq_ld], column `step` when 0 <= step < seq_cols; or null
    int64_t seq_ld;
    int32_t seq_cols;
};

// u = ((x >> 9) + 1/2) * 2^-23: 23 bits, so u is exact in f32 and lies in [2^-24, 1 - 2^-24] -- never 0 or 1.
// g = -log(-log(u)) is then within [-2.82, 16.64].
LWM_HD float gumbel_of(uint32_t x) {
    const float u = ((float)(x >> 9) + 0.5f) * 0x1p-23f;
    return -logf(-logf(u));
}

// order-preserving f32 -> u32 (both zeros map to +0's key)
LWM_HD uint32_t order_key(float x) {
    const uint32_t u = __builtin_bit_cast(uint32_t, x == 0.0f ? 0.0f : x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
LWM_HD float order_value(uint32_t k) {
    return __builtin_bit_cast(float, (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// the (guided) logit of entry j of output row b, evaluated as the eager code does -- u + s * (c - u), three roundings
LWM_DEVICE float sample_logit(const SampleParams& p, int b, int j) {
#pragma clang fp contract(off)
    const float c = p.logits[(int64_t)b * p.ld + j];
    if (!p.cfg) return c;
    const float u = p.logits[(int64_t)(b + p.B) * p.ld + j];
    const float s = p.cfg_scale[b];
    return u + s * (c - u);
}

// the key an entry is ranked by: the logit (greedy) or logit / T
LWM_DEVICE uint32_t sample_key(const SampleParams& p, int b, int j, bool greedy) {
    if (j >= p.V) return 0;
    const float l = sample_logit(p, b, j);
    return order_key(greedy ? l : l / p.temperature);
}

// w = exp(s - smax) of the top-p masses, in f64 from an f32 exponential: d = s - smax is exact in f64 (to 2^-53 where the
// exponents lie far apart), expf takes its f32 rounding dh and the remainder d - dh (|.| <= 2^-24 |d| < 6.2e-6 wherever
// w > 0) enters to first order, its square (< 2e-11) dropped.  w is then within the exponential's own error of exp(d):
// 2 ulps = 2^-22 relative at most (the device's expf is documented at 1).  s = -inf gives 0.  (The rounds hold it as an
// f32: one more rounding, 2^-24.)
LWM_DEVICE double sample_weight(float s, float smax) {
    const double d = (double)s - (double)smax;
    const float dh = (float)d;
    const float e = expf(dh);
    return e == 0.0f ? 0.0 : (double)e * (1.0 + (d - (double)dh));
}

LWM_DEVICE double shfl_xor_d(double x, int m) {
    const uint64_t u = __builtin_bit_cast(uint64_t, x);
    const uint32_t lo = (uint32_t)shfl_xor_i((int)(uint32_t)u, m), hi = (uint32_t)shfl_xor_i((int)(uint32_t)(u >> 32), m);
    return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}

LWM_DEVICE void argmax_offer(uint32_t k, int j, uint32_t& bk, int& bj) {
    if (k > bk || (k == bk && j < bj)) {
        bk = k;
        bj = j;
    }
}

// kTopP: the top-p phase is compiled in (sample_top_p_kernel) or not at all (sample_kernel)
template <bool kTopP>
LWM_DEVICE void sample_body(const SampleParams& p) {
    const int b = block_idx_x(), tid = thread_idx(), lane = tid & 63, wave = tid >> 6;
    const lds_t lds = dyn_lds();
    const lds_t lds_cnt = lds, lds_tot = lds + 4 * kSampleWaves * 16, lds_arg = lds_tot + 4 * 16;
    const bool greedy = !(p.temperature > 0.0f);
    const int V = p.V;
    const int step = p.step_dev ? *p.step_dev - p.step_base : p.step;
    // entry j = 4 * (g * kSampleThreads + tid) + e of group g
    const auto entry = [&](int g, int e) { return 4 * (g * kSampleThreads + tid) + e; };
    const int n_groups = (int)(((int64_t)V + 4 * kSampleThreads - 1) / (4 * kSampleThreads));

    // (groups past n_groups hold no entry of this row: skipped by a wave-uniform branch in every pass)
    uint32_t key[kSampleGroups][4];
#pragma unroll
    for (int g = 0; g < kSampleGroups; ++g)
#pragma unroll
        for (int e = 0; e < 4; ++e) key[g][e] = g < n_groups ? sample_key(p, b, entry(g, e), greedy) : 0u;

    // ---- top-k: the k-th largest key by a radix select, 4-bit digits from the top, 8 rounds.  Counts are kept per
    // lane, reduced over the wave by shuffles and over the waves through LDS -- integer sums, no atomics.
    uint32_t thr = 0;
    if (!greedy && p.top_k > 0 && p.top_k < V) {
        uint32_t prefix = 0, mask = 0;
        int remaining = p.top_k;
        for (int shift = 28; shift >= 0; shift -= 4) {
            int cnt[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) cnt[i] = 0;
            uint64_t lo = 0, hi = 0;         // 8-bit counters: digits 0-7 in lo, 8-15 in hi (<= 4 * groups per lane)
            const auto count = [&](uint32_t k, int j) {
                if (j < V && (k & mask) == prefix) {
                    const uint32_t d = (k >> shift) & 15u;
                    const uint64_t inc = 1ull << ((d & 7u) * 8u);
                    if (d & 8u) hi += inc;
                    else lo += inc;
                }
            };
            const auto flush = [&]() {
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    cnt[i] += (int)((lo >> (8 * i)) & 255u);
                    cnt[8 + i] += (int)((hi >> (8 * i)) & 255u);
                }
                lo = hi = 0;
            };
#pragma unroll
            for (int g = 0; g < kSampleGroups; ++g)
                if (g < n_groups)
#pragma unroll
                    for (int e = 0; e < 4; ++e) count(key[g][e], entry(g, e));
            flush();
            for (int g = kSampleGroups; g < n_groups; ++g) {
                for (int e = 0; e < 4; ++e) count(sample_key(p, b, entry(g, e), false), entry(g, e));
                flush();
            }
            // transposed wave reduction: each step over lane bits 5..2 halves the digits a lane carries; then lane l
            // holds digit (l >> 2) & 15 summed over the 16 lanes that differ in those bits, and two more steps finish
#pragma unroll
            for (int w = 8, m = 32; w >= 1; w >>= 1, m >>= 1) {
                const bool up = (lane & m) != 0;
#pragma unroll
                for (int i = 0; i < w; ++i) {
                    const int send = up ? cnt[i] : cnt[i + w];
                    const int keep = up ? cnt[i + w] : cnt[i];
                    cnt[i] = keep + shfl_xor_i(send, m);
                }
            }
            int c = cnt[0];
            c += shfl_xor_i(c, 2);
            c += shfl_xor_i(c, 1);
            if ((lane & 3) == 0) lds_write_i32(lds_cnt + 4 * (wave * 16 + (lane >> 2)), c);
            block_sync();
            if (tid < 16) {
                int t = 0;
                for (int w = 0; w < kSampleWaves; ++w) t += lds_read_i32(lds_cnt + 4 * (w * 16 + tid));
                lds_write_i32(lds_tot + 4 * tid, t);
            }
            block_sync();
            int d = 15;
            for (; d > 0; --d) {
                const int t = lds_read_i32(lds_tot + 4 * d);
                if (t >= remaining) break;
                remaining -= t;
            }
            prefix |= (uint32_t)d << shift;
            mask |= 15u << shift;
        }
        thr = prefix;            // keep every entry >= the k-th largest: ties at the threshold all stay
    }

    // ---- top-p over the top-k survivors K = {key >= thr}: entry j stays iff M(j) < top_p * Z, with w = exp(s - max s),
    // Z the sum of w over K and M(j) the sum over the entries of K strictly above j.  The same radix descent over the
    // keys, carrying per-digit MASSES (f64) in place of counts: going down the digits of a round, `above` gathers the
    // mass of the digits passed, and the lowest digit whose mass above is still below top_p * Z is taken.  The final
    // prefix is a threshold (not necessarily a key of the row): every key >= it has M < top_p * Z, every key below it
    // has not.  Equal keys share one M.  A sum that is no number (a +inf or NaN logit, or no finite one) stops no
    // descent: the threshold ends at 0 and K stays whole.
    if (kTopP && !greedy && p.top_p > 0.0f && p.top_p < 1.0f) {
        const lds_t lds_mass = lds_arg + 4 * kSampleWaves * 2, lds_mtot = lds_mass + 8 * kSampleWaves * 16;
        uint32_t kmax = 0;       // the row's largest key (entries past V carry key 0, the smallest); it lies in K
#pragma unroll
        for (int g = 0; g < kSampleGroups; ++g)
#pragma unroll
            for (int e = 0; e < 4; ++e) kmax = key[g][e] > kmax ? key[g][e] : kmax;
        for (int g = kSampleGroups; g < n_groups; ++g)
            for (int e = 0; e < 4; ++e) {
                const uint32_t k = sample_key(p, b, entry(g, e), false);
                kmax = k > kmax ? k : kmax;
            }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const uint32_t o = (uint32_t)shfl_xor_i((int)kmax, m);
            kmax = o > kmax ? o : kmax;
        }
        if (lane == 0) lds_write_i32(lds_arg + 8 * wave, (int)kmax);
        block_sync();
        for (int w = 0; w < kSampleWaves; ++w) {
            const uint32_t o = (uint32_t)lds_read_i32(lds_arg + 8 * w);
            kmax = o > kmax ? o : kmax;
        }
        const float smax = order_value(kmax);
        // the weights of the register-held entries, once, rounded to f32 (0 outside K)
        float wt[kSampleGroups][4];
#pragma unroll
        for (int g = 0; g < kSampleGroups; ++g)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                wt[g][e] = g < n_groups && entry(g, e) < V && key[g][e] >= thr ? (float)sample_weight(order_value(key[g][e]), smax) : 0.0f;

        uint32_t prefix = 0, mask = 0;
        double above = 0.0, pz = 0.0;
        for (int shift = 28; shift >= 0; shift -= 4) {
            double ms[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) ms[i] = 0.0;
            // (opaque: or the f64 values of the held weights are hoisted out of the rounds, 64 registers, and spill)
            const auto add = [&](uint32_t k, float w_held) {
                const float w = __builtin_bit_cast(float, opaque(__builtin_bit_cast(uint32_t, w_held)));
                if ((k & mask) == prefix) {
                    const uint32_t d = (k >> shift) & 15u;
#pragma unroll
                    for (int i = 0; i < 16; ++i) ms[i] += (double)(d == (uint32_t)i ? w : 0.0f);
                }
            };
#pragma unroll
            for (int g = 0; g < kSampleGroups; ++g)
                if (g < n_groups)
#pragma unroll
                    for (int e = 0; e < 4; ++e) add(key[g][e], wt[g][e]);
            // (entries past the register-held ones: key and weight again in every round, as the top-k counts them)
            for (int g = kSampleGroups; g < n_groups; ++g)
                for (int e = 0; e < 4; ++e) {
                    const uint32_t k = sample_key(p, b, entry(g, e), false);
                    add(k, entry(g, e) < V && k >= thr ? (float)sample_weight(order_value(k), smax) : 0.0f);
                }
            // the transposed wave reduction of the counts, on f64 sums: a fixed tree
#pragma unroll
            for (int w = 8, m = 32; w >= 1; w >>= 1, m >>= 1) {
                const bool up = (lane & m) != 0;
#pragma unroll
                for (int i = 0; i < w; ++i) {
                    const double send = up ? ms[i] : ms[i + w];
                    const double keep = up ? ms[i + w] : ms[i];
                    ms[i] = keep + shfl_xor_d(send, m);
                }
            }
            double c = ms[0];
            c += shfl_xor_d(c, 2);
            c += shfl_xor_d(c, 1);
            if ((lane & 3) == 0) lds_write_f64(lds_mass + 8 * (wave * 16 + (lane >> 2)), c);
            block_sync();
            if (tid < 16) {
                double t = 0.0;
                for (int w = 0; w < kSampleWaves; ++w) t += lds_read_f64(lds_mass + 8 * (w * 16 + tid));
                lds_write_f64(lds_mtot + 8 * tid, t);
            }
            block_sync();
            if (shift == 28) {   // the first round's digits hold all of K
                double z = 0.0;
                for (int d = 15; d >= 0; --d) z += lds_read_f64(lds_mtot + 8 * d);
                pz = (double)p.top_p * z;
            }
            int d = 15;
            for (; d > 0; --d) {
                const double t = lds_read_f64(lds_mtot + 8 * d);
                if (above + t >= pz) break;
                above += t;
            }
            prefix |= (uint32_t)d << shift;
            mask |= 15u << shift;
        }
        thr = prefix > thr ? prefix : thr;
    }

    // ---- argmax of the key (greedy) or of logit / T + Gumbel noise over the kept entries, lowest index on ties
    uint32_t bk = 0;
    int bj = 0x7fffffff;
    const auto visit = [&](int g, const uint32_t (&k)[4]) {
        if (greedy) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (entry(g, e) < V) argmax_offer(k[e], entry(g, e), bk, bj);
            return;
        }
        uint32_t x[4] = {(uint32_t)(g * kSampleThreads + tid), (uint32_t)b, (uint32_t)step, 0u};
        philox4x32_10(x, p.key0, p.key1);
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (entry(g, e) < V && k[e] >= thr)
                argmax_offer(order_key(order_value(k[e]) + gumbel_of(x[e])), entry(g, e), bk, bj);
    };
#pragma unroll
    for (int g = 0; g < kSampleGroups; ++g)
        if (g < n_groups) visit(g, key[g]);
    for (int g = kSampleGroups; g < n_groups; ++g) {
        uint32_t k[4];
        for (int e = 0; e < 4; ++e) k[e] = sample_key(p, b, entry(g, e), greedy);
        visit(g, k);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const uint32_t ok = (uint32_t)shfl_xor_i((int)bk, m);
        const int oj = shfl_xor_i(bj, m);
        argmax_offer(ok, oj, bk, bj);
    }
    if (lane == 0) {
        lds_write_i32(lds_arg + 8 * wave, (int)bk);
        lds_write_i32(lds_arg + 8 * wave + 4, bj);
    }
    block_sync();
    if (tid != 0) return;
    for (int w = 1; w < kSampleWaves; ++w)
        argmax_offer((uint32_t)lds_read_i32(lds_arg + 8 * w), lds_read_i32(lds_arg + 8 * w + 4), bk, bj);

    // ---- bookkeeping of the decode step
    int64_t tok = bj < V ? bj : V - 1;
    if (p.force_period > 0 && (step + 1) % p.force_period == 0) tok = p.force_token;
    if (p.done) {
        if (p.done[b]) tok = p.pad;
        if (p.eos >= 0 && tok == p.eos) p.done[b] = 1;
    }
    if (p.tokens)
        for (int c = 0; c < p.copies; ++c) p.tokens[(int64_t)c * p.B + b] = tok;
    if (p.seq && step >= 0 && step < p.seq_cols) p.seq[(int64_t)b * p.seq_ld + step] = tok;
}

LWM_KERNEL(kSampleThreads) void sample_kernel(SampleParams p) { sample_body<false>(p); }
// the launch of 0 < top_p < 1: a launch without it runs the code it ran before the phase existed
LWM_KERNEL(kSampleThreads) void sample_top_p_kernel(SampleParams p) { sample_body<true>(p); }

}  // namespace lwm
