// vqgan_api.inc -- C ABI of the VQGAN primitives (include/lwm_hip.h): argument
// validation, tile-shape selection, launches.  Included by lwm_vqgan.hip (product)
// and tests/emu/lwm_emu.cpp (host emulation, test-only).

#include "frames.h"
#include "vqgan_conv_bf16.h"

namespace lwm {

static bool vq_aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

#ifdef LWM_EMU      // (the product's is in launch.h)
static int copy_to_device(void* dst, const void* src, size_t bytes, void* stream) {
    (void)stream;
    memcpy(dst, src, bytes);
    return 0;
}
#endif

// workspace of the frame preprocessor: [h bounds | h coeffs | v bounds | v coeffs | scale] as 4-byte words, rounded up
// to 16 bytes, then the uint8 intermediate image
static int64_t frames_table_bytes(int64_t size, int64_t hks, int64_t vks) {
    const int64_t words = (hks ? size * (2 + hks) : 0) + (vks ? size * (2 + vks) : 0) + 256;
    return (words * 4 + 15) & ~(int64_t)15;
}
static int64_t frames_istride(int64_t size) { return (size * 3 + 3) & ~(int64_t)3; }

// one pass's tables against its input length; *lo / *hi: the input samples [lo, hi) that the pass reads
static int frames_check_pass(const char* which, const int32_t* bounds, const int32_t* coeffs, int32_t ksize, int32_t size,
                             int32_t n_in, int32_t skip_first, int32_t* lo, int32_t* hi) {
    if (ksize < 0) return fail(LWM_EINVAL, "frames: %s pass: negative ksize", which);
    if (ksize == 0) {
        if (bounds || coeffs) return fail(LWM_EINVAL, "frames: %s pass: ksize 0 with tables", which);
        if (skip_first < 0 || (int64_t)skip_first + size > n_in)
            return fail(LWM_EINVAL, "frames: %s pass skipped: window at %ld leaves the input of %ld", which, skip_first, n_in);
        *lo = skip_first;
        *hi = skip_first + size;
        return LWM_OK;
    }
    if (!bounds || !coeffs) return fail(LWM_EINVAL, "frames: %s pass: null table", which);
    *lo = n_in;
    *hi = 0;
    for (int32_t i = 0; i < size; ++i) {
        const int64_t first = bounds[2 * i], taps = bounds[2 * i + 1];
        if (first < 0 || taps < 1 || taps > ksize || first + taps > n_in)
            return fail(LWM_EINVAL, "frames: %s pass: bounds of output %ld leave the input or exceed ksize", which, i);
        if (first < *lo) *lo = (int32_t)first;
        if (first + taps > *hi) *hi = (int32_t)(first + taps);
    }
    return LWM_OK;
}

// number of statistics slices for a GroupNorm over HW pixels
static int gn_slices(int64_t HW) {
    int64_t ns = (HW + 63) / 64;
    if (ns < 1) ns = 1;
    if (ns > 256) ns = 256;
    return (int)ns;
}

}  // namespace lwm

extern "C" {

// what the two convolution entries check alike, and their ConvParams; B == 0 leaves p->M == 0: nothing to launch
static int conv_params(const LwmConvArgs* a, lwm::ConvParams* pp) {
    using namespace lwm;
    ConvParams& p = *pp;
    p.M = 0;
    if (!a) return fail(LWM_EINVAL, "%s", "conv: args is null");
    if (!a->x || !a->w || !a->y) return fail(LWM_EINVAL, "%s", "conv: null tensor");
    if (a->B < 0 || a->Hin <= 0 || a->Win <= 0 || a->Cin <= 0 || a->Cout <= 0 || a->KH <= 0 ||
        a->KW <= 0 || a->stride <= 0 || a->pad < 0 || a->up_shift < 0 || a->up_shift > 4 ||
        a->Ho <= 0 || a->Wo <= 0)
        return fail(LWM_EINVAL, "%s", "conv: bad dimension");
    if (!vq_aligned16(a->x) || !vq_aligned16(a->w) || !vq_aligned16(a->y) ||
        (a->residual && !vq_aligned16(a->residual)))
        return fail(LWM_EINVAL, "%s", "conv: pointer not 16-byte aligned");
    if (a->B == 0) return LWM_OK;
    // (the kernels address a pixel inside its image with 32 bits; the image base is 64-bit)
    if ((int64_t)a->Hin * a->Win * a->Cin >= (1LL << 31) || (int64_t)a->Ho * a->Wo * a->Cout >= (1LL << 31))
        return fail(LWM_EUNSUPPORTED, "%s: one image holds 2^31 elements or more (H x W = %ld x %ld)", "conv", (long)a->Hin, (long)a->Win);
    p.x = a->x; p.w = a->w; p.bias = a->bias; p.res = a->residual; p.y = a->y;
    p.B = a->B; p.Hin = a->Hin; p.Win = a->Win; p.Cin = a->Cin; p.Cout = a->Cout;
    p.KH = a->KH; p.KW = a->KW; p.stride = a->stride; p.pad = a->pad; p.up_shift = a->up_shift;
    p.Ho = a->Ho; p.Wo = a->Wo; p.clip = a->clip ? 1 : 0;
    p.M = (int64_t)a->B * a->Ho * a->Wo;
    if (((p.M + 31) / 32) * (((int64_t)p.Cout + 31) / 32) > 0x7fffffffLL) return fail(LWM_EINVAL, "%s", "conv: grid too large");
    return LWM_OK;
}

int lwm_conv2d_nhwc_f32(const LwmConvArgs* a, void* stream) {
    using namespace lwm;
    ConvParams p;
    if (const int r = conv_params(a, &p)) return r;
    if (!p.M) return LWM_OK;
    auto tiles = [&](int bm, int bn) { return ((p.M + bm - 1) / bm) * ((p.Cout + bn - 1) / bn); };
    const bool vec = (p.Cin % 4 == 0) && (p.Cout % 4 == 0);
    // 3x3 stride-1 SAME (optionally over the x2-upsampled image) with 128 / 256 input channels: halo patch
    // resident in LDS (vqgan_conv.h::conv_patch_body)
#ifndef LWM_CONV_NO_PATCH
    if (p.KH == 3 && p.KW == 3 && p.stride == 1 && p.pad == 1 && p.Ho == (p.Hin << p.up_shift) &&
        p.Wo == (p.Win << p.up_shift) && p.Wo % 16 == 0) {
        // (persistent: one workgroup per CU walks the tiles)
        auto patch_grid = [&](long tiles) { return tiles < device_cu_count() ? tiles : device_cu_count(); };
        if (p.Cin == 128 && p.Cout % PatchC128::BN == 0 && p.Ho % (PatchC128::BM / 16) == 0 && p.M / PatchC128::BM * (p.Cout / PatchC128::BN) >= device_cu_count() / 2)
            return launch(p.res ? "conv_patch_c128_res" : "conv_patch_c128", p.res ? conv_patch_c128_res : conv_patch_c128,
                          patch_grid(p.M / PatchC128::BM * (p.Cout / PatchC128::BN)), PatchC128::NT, PatchC128::LDS_BYTES, stream, p);
        if (p.Cin == 256 && p.Cout % PatchC256::BN == 0 && p.Ho % (PatchC256::BM / 16) == 0 && p.M / PatchC256::BM * (p.Cout / PatchC256::BN) >= device_cu_count() / 2)
            return launch(p.res ? "conv_patch_c256_res" : "conv_patch_c256", p.res ? conv_patch_c256_res : conv_patch_c256,
                          patch_grid(p.M / PatchC256::BM * (p.Cout / PatchC256::BN)), PatchC256::NT, PatchC256::LDS_BYTES, stream, p);
    }
#endif
    // the two ends of the network (vqgan_conv.h): 3 input channels / 3 output channels
    if (p.KH == 3 && p.KW == 3 && p.Cin <= 4 && p.Cout % 64 == 0)
        return launch("conv_cin4_n64", conv_cin4_n64, (p.M + 4 * kCinPB * 32 - 1) / (4 * kCinPB * 32) * (p.Cout / 64), 256, 0, stream, p);
    if (p.KH == 3 && p.KW == 3 && p.stride == 1 && p.pad == 1 && p.Ho == (p.Hin << p.up_shift) && p.Wo == (p.Win << p.up_shift) &&
        p.Wo % 16 == 0 && p.Ho % 4 == 0 && p.Cin == 128 && p.Cout == 3)
        return launch("conv_patch_c128_out3", conv_patch_c128_out3, p.M / 64, 256, PatchOutC128::LDS_BYTES, stream, p);
    if (p.Cout <= 32)
        return launch("conv_igemm_128x32_g", conv_igemm_128x32_g, tiles(128, 32), 256,
                      ConvCfg<4, 1, 1, 1>::LDS_BYTES, stream, p);
    if (p.Cout <= 64)
        return vec ? launch("conv_igemm_128x64", conv_igemm_128x64, tiles(128, 64), 256,
                            ConvCfg<4, 1, 1, 2>::LDS_BYTES, stream, p)
                   : launch("conv_igemm_128x64_g", conv_igemm_128x64_g, tiles(128, 64), 256,
                            ConvCfg<4, 1, 1, 2>::LDS_BYTES, stream, p);
    if (tiles(128, 128) < device_cu_count())  // too few workgroups for the machine: smaller pixel tile
        return vec ? launch("conv_igemm_32x128", conv_igemm_32x128, tiles(32, 128), 256,
                            ConvCfg<1, 4, 1, 1>::LDS_BYTES, stream, p)
                   : launch("conv_igemm_32x128_g", conv_igemm_32x128_g, tiles(32, 128), 256,
                            ConvCfg<1, 4, 1, 1>::LDS_BYTES, stream, p);
#ifndef LWM_CONV_NO_BDIRECT
    // (its staging offsets are 32-bit, relative to the image of a tile's first pixel: the images a 128-pixel tile can reach)
    if (vec && p.Cin % 32 == 0 && p.Cout % 128 == 0 &&
        (128 / ((int64_t)p.Ho * p.Wo) + 2) * ((int64_t)p.Hin * p.Win * p.Cin * 4) < 0xE0000000LL)
        return launch("conv_igemm_128x128_bd", conv_igemm_128x128_bd, tiles(128, 128), 256, 3 * ConvCfg<2, 2, 2, 2>::A_BYTES, stream, p);
#endif
    return vec ? launch("conv_igemm_128x128", conv_igemm_128x128, tiles(128, 128), 256,
                        ConvCfg<2, 2, 2, 2>::LDS_BYTES, stream, p)
               : launch("conv_igemm_128x128_g", conv_igemm_128x128_g, tiles(128, 128), 256,
                        ConvCfg<2, 2, 2, 2>::LDS_BYTES, stream, p);
}

int lwm_conv2d_nhwc_bf16(const LwmConvArgs* a, void* stream) {
    using namespace lwm;
    ConvParams p;      // (p.w: the bf16 pack, vqgan_conv_bf16.h)
    if (const int r = conv_params(a, &p)) return r;
    if (a->Cin % 32 || a->Cout % 32)
        return fail(LWM_EUNSUPPORTED, "%s: Cin=%ld Cout=%ld (need Cin %% 32 == 0 and Cout %% 32 == 0; lwm_conv2d_nhwc_f32 serves the rest)",
                    "conv_bf16", (long)a->Cin, (long)a->Cout);
    if (!p.M) return LWM_OK;
    // (its staging offsets are 32-bit, relative to the image of a tile's first pixel: the images a 128-pixel tile can
    //  reach; its B offsets are 32-bit inside the pack)
    if ((128 / ((int64_t)p.Ho * p.Wo) + 2) * ((int64_t)p.Hin * p.Win * p.Cin * 4) >= 0xE0000000LL ||
        (int64_t)p.KH * p.KW * p.Cin * p.Cout * 2 >= 0xE0000000LL)
        return fail(LWM_EUNSUPPORTED, "%s: an image or the packed kernel is too large for 32-bit staging offsets (H x W = %ld x %ld)",
                    "conv_bf16", (long)a->Hin, (long)a->Win);
    auto tiles = [&](int bm, int bn) { return ((p.M + bm - 1) / bm) * ((p.Cout + bn - 1) / bn); };
    if (p.Cout == 32)
        return launch("conv16_igemm_128x32", conv16_igemm_128x32, tiles(128, 32), 256, Conv16T128x32::LDS_BYTES, stream, p);
    if (p.Cout <= 64 || tiles(128, 128) < device_cu_count())     // narrow, or too few workgroups for the machine
        return launch("conv16_igemm_64x64", conv16_igemm_64x64, tiles(64, 64), 256, Conv16T64x64::LDS_BYTES, stream, p);
    return launch("conv16_igemm_128x128", conv16_igemm_128x128, tiles(128, 128), 256, Conv16T128x128::LDS_BYTES, stream, p);
}

int64_t lwm_groupnorm_workspace_bytes(int32_t B, int64_t HW, int32_t C, int32_t G) {
    (void)C;
    if (B <= 0 || HW <= 0 || G <= 0) return 0;
    // slice partials [B][NS][G][2] f64, then mean / rstd [B][G][2] f32
    return (int64_t)B * lwm::gn_slices(HW) * G * 2 * (int64_t)sizeof(double) + (int64_t)B * G * 2 * (int64_t)sizeof(float);
}

int lwm_groupnorm_silu_f32(const float* x, const float* gamma, const float* beta, float* y,
                           void* workspace, int32_t B, int64_t HW, int32_t C, int32_t G, float eps,
                           int32_t silu, void* stream) {
    using namespace lwm;
    if (!x || !gamma || !beta || !y || !workspace) return fail(LWM_EINVAL, "%s", "groupnorm: null pointer");
    if (B < 0 || HW <= 0 || C <= 0 || G <= 0 || G > 64 || C % G) return fail(LWM_EINVAL, "%s", "groupnorm: bad dimension");
    if ((C / G) % 4 || C > 4 * kGnThreads)
        return fail(LWM_EUNSUPPORTED, "%s: C=%ld G=%ld (need (C/G)%%4==0, C<=1024)", "groupnorm", C, G);
    if (!vq_aligned16(x) || !vq_aligned16(y) || (((uintptr_t)workspace) & 7))
        return fail(LWM_EINVAL, "%s", "groupnorm: misaligned pointer");
    if (B == 0) return LWM_OK;
    GnParams p;
    p.x = x; p.gamma = gamma; p.beta = beta; p.y = y; p.part = (double*)workspace;
    p.B = B; p.C = C; p.G = G; p.silu = silu ? 1 : 0; p.HW = HW; p.eps = eps;
    p.NS = gn_slices(HW);
    p.slice = (HW + p.NS - 1) / p.NS;
    p.NS = (int)((HW + p.slice - 1) / p.slice);  // no empty slices
    p.aslice = p.slice;
    p.stats = (float*)(p.part + (int64_t)B * gn_slices(HW) * G * 2);
    int r = launch("gn_stats", gn_stats_kernel, (long)B * p.NS, kGnThreads, kGnThreads * 16, stream, p);
    if (r) return r;
    r = launch("gn_finalize", gn_finalize_kernel, (long)B * G, 64, (size_t)p.NS * 16, stream, p);
    if (r) return r;
    const int64_t nas = (HW + p.aslice - 1) / p.aslice;
    return launch("gn_apply", gn_apply_kernel, (long)B * nas, kGnThreads, 0, stream, p);
}

int lwm_vq_sqnorm_f32(const float* codebook, float* se, int32_t E, int32_t D, void* stream) {
    using namespace lwm;
    if (!codebook || !se || E <= 0 || D <= 0) return fail(LWM_EINVAL, "%s", "vq_sqnorm: bad argument");
    return launch("vq_sqnorm", vq_sqnorm_kernel, (E + 255) / 256, 256, 0, stream, codebook, se, (int)E, (int)D);
}

int lwm_vq_argmin_f32(const float* z, const float* codebook, const float* se, int32_t* idx,
                      int64_t N, int32_t E, int32_t D, void* stream) {
    using namespace lwm;
    if (!z || !codebook || !se || !idx) return fail(LWM_EINVAL, "%s", "vq_argmin: null pointer");
    if (D != kVqD) return fail(LWM_EUNSUPPORTED, "%s: embed dim %ld (only 64)", "vq_argmin", D);
    if (N < 0 || E <= 0) return fail(LWM_EINVAL, "%s", "vq_argmin: bad dimension");
    if (!vq_aligned16(z) || !vq_aligned16(codebook)) return fail(LWM_EINVAL, "%s", "vq_argmin: misaligned");
    if (N == 0) return LWM_OK;
    return launch("vq_argmin", vq_argmin_kernel, (long)((N + 31) / 32), kVqThreads, 8 * 32 * 8, stream,
                  z, codebook, se, idx, N, (int)E);
}

int lwm_vq_gather_f32(const float* codebook, const int32_t* idx, const float* z, float* out,
                      int64_t N, int32_t E, int32_t D, void* stream) {
    using namespace lwm;
    if (!codebook || !idx || !out) return fail(LWM_EINVAL, "%s", "vq_gather: null pointer");
    if (N < 0 || E <= 0 || D <= 0 || D % 4) return fail(LWM_EINVAL, "%s", "vq_gather: bad dimension");
    if (!vq_aligned16(codebook) || !vq_aligned16(out) || (z && !vq_aligned16(z)))
        return fail(LWM_EINVAL, "%s", "vq_gather: misaligned");
    if (N == 0) return LWM_OK;
    long blocks = (long)((N * (D / 4) + 255) / 256);
    if (blocks > 8192) blocks = 8192;
    return launch("vq_gather", vq_gather_kernel, blocks, 256, 0, stream, codebook, idx, z, out, N, (int)D, (int)E);
}

int64_t lwm_frames_preprocess_workspace_bytes(int32_t T, int32_t H, int32_t size, int32_t h_ksize, int32_t v_ksize) {
    if (T < 1 || H < 1 || size < 1 || h_ksize < 0 || v_ksize < 0) return 0;
    // (the intermediate image holds at most all H rows of the `size` cropped columns)
    return lwm::frames_table_bytes(size, h_ksize, v_ksize) + (int64_t)T * H * lwm::frames_istride(size);
}

int lwm_frames_preprocess_u8(const LwmFramesArgs* a, void* stream) {
    using namespace lwm;
    if (!a) return fail(LWM_EINVAL, "%s", "frames: args is null");
    if (!a->frames || !a->out || !a->workspace || !a->scale) return fail(LWM_EINVAL, "%s", "frames: null pointer");
    if (a->T < 1 || a->H < 1 || a->W < 1 || a->size < 1) return fail(LWM_EINVAL, "%s", "frames: T, H, W, size must be >= 1");
    if ((int64_t)a->H * a->W * 3 >= (1LL << 31) || a->size > 16384)
        return fail(LWM_EUNSUPPORTED, "%s: one frame holds 2^31 bytes or more, or size > 16384 (H x W = %ld x %ld)", "frames", (long)a->H, (long)a->W);
    // every table entry is checked here, on the host, before anything is launched: the kernels index with them
    int32_t clo, chi, rlo, rhi;
    int r;
    if ((r = frames_check_pass("horizontal", a->h_bounds, a->h_coeffs, a->h_ksize, a->size, a->W, a->left, &clo, &chi))) return r;
    if ((r = frames_check_pass("vertical", a->v_bounds, a->v_coeffs, a->v_ksize, a->size, a->H, a->top, &rlo, &rhi))) return r;
    if (!vq_aligned16(a->workspace)) return fail(LWM_EINVAL, "%s", "frames: workspace not 16-byte aligned");
    if (a->workspace_bytes < lwm_frames_preprocess_workspace_bytes(a->T, a->H, a->size, a->h_ksize, a->v_ksize))
        return fail(LWM_EINVAL, "frames: workspace of %s%ld bytes, need %ld", "", (long)a->workspace_bytes,
                    (long)lwm_frames_preprocess_workspace_bytes(a->T, a->H, a->size, a->h_ksize, a->v_ksize));

    FramesParams p;
    p.frames = a->frames; p.out = a->out;
    p.T = a->T; p.H = a->H; p.W = a->W; p.size = a->size; p.hks = a->h_ksize; p.vks = a->v_ksize;
    p.left = a->left; p.top = a->top;
    p.total = (int64_t)a->T * a->H * a->W * 3;
    p.row0 = rlo; p.nrows = rhi - rlo;
    p.istride = (int32_t)frames_istride(a->size);
    p.nstrips = (a->size + kFrCols - 1) / kFrCols;
    p.nrblocks = (p.nrows + kFrRowsPerWg - 1) / kFrRowsPerWg;
    // the widest input span of a strip of output columns sizes the staged rows (+ the misalignment of a row's first
    // byte, + the dword that frames_px reads past a pixel)
    int32_t span = 0;
    for (int32_t s = 0; s < p.nstrips; ++s) {
        const int32_t x0 = s * kFrCols, x1 = x0 + kFrCols < a->size ? x0 + kFrCols : a->size;
        int32_t lo = a->W, hi = 0;
        if (!a->h_ksize) { lo = x0; hi = x1; }
        for (int32_t i = x0; a->h_ksize && i < x1; ++i) {
            const int32_t first = a->h_bounds[2 * i], end = first + a->h_bounds[2 * i + 1];
            lo = first < lo ? first : lo;
            hi = end > hi ? end : hi;
        }
        span = hi - lo > span ? hi - lo : span;
    }
    p.span_dw = (span * 3 + 6) / 4 + 2;
    const size_t lds = frames_hpass_lds(p.hks, p.span_dw);
    if (lds > 160 * 1024)
        return fail(LWM_EUNSUPPORTED, "%s: a strip of output columns reads %ld input columns with %ld taps: over the LDS", "frames", (long)span, (long)a->h_ksize);
    const int64_t hgrid = (int64_t)a->T * p.nrblocks * p.nstrips;
    const int64_t vgrid = (int64_t)a->T * (((int64_t)a->size * (p.istride / 4) + kFrThreads - 1) / kFrThreads);
    if (hgrid > 0x7fffffffLL || vgrid > 0x7fffffffLL) return fail(LWM_EINVAL, "%s", "frames: grid too large");

    // tables -> the head of the workspace, in the order of frames_table_bytes
    int32_t* w = (int32_t*)a->workspace;
    auto put = [&](const void* src, int64_t words) -> const int32_t* {
        const int32_t* at = w;
        if (!r) r = copy_to_device(w, src, (size_t)words * 4, stream);
        w += words;
        return at;
    };
    p.hb = p.hk = p.vb = p.vk = nullptr;
    if (a->h_ksize) { p.hb = put(a->h_bounds, (int64_t)a->size * 2); p.hk = put(a->h_coeffs, (int64_t)a->size * a->h_ksize); }
    if (a->v_ksize) { p.vb = put(a->v_bounds, (int64_t)a->size * 2); p.vk = put(a->v_coeffs, (int64_t)a->size * a->v_ksize); }
    p.scale = (const float*)put(a->scale, 256);
    if (r) return r;
    p.inter = (uint8_t*)a->workspace + frames_table_bytes(a->size, a->h_ksize, a->v_ksize);
    if ((r = launch("frames_hpass", frames_hpass_kernel, (long)hgrid, kFrThreads, lds, stream, p))) return r;
    return launch("frames_vpass", frames_vpass_kernel, (long)vgrid, kFrThreads, 0, stream, p);
}

}  // extern "C"
