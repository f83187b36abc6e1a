"""numpy restatement of lwm_amd.cli.vision_chat._process_frame (Pillow's antialiased bicubic resize of the short side,
centre crop, scale to [-1, 1]) -- the reference of the frame preprocessor's tests.  Independent of lwm_amd.frames; int64
accumulators.  TEST INFRASTRUCTURE ONLY.

Pillow's 8-bit resample (src/libImaging/Resample.c): per pass, f64 bicubic weights over a support scaled by the
downscaling factor, normalised, rounded to 22-bit fixed point; integer accumulation from 2^21, arithmetic shift by 22,
clamp to [0, 255].  Horizontal pass first, uint8 intermediate image, then the vertical pass; a pass whose output length
equals its input length is skipped."""
import functools
import math

import numpy as np

PRECISION_BITS = 22


def bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def pass_tables(n_in, n_out):
    """-> bounds (n_out, 2) int64 (first input sample, tap count), coeffs (n_out, ksize) int64 (zero past the taps)"""
    scale = n_in / n_out
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ss = 1.0 / filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((n_out, 2), np.int64)
    coeffs = np.zeros((n_out, ksize), np.int64)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in) - xmin
        w = [bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        bounds[xx] = xmin, xmax
        for x, v in enumerate(w):
            coeffs[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
    return bounds, coeffs


def target(h, w, size):
    """-> (nw, nh, left, top) of _process_frame"""
    if w < h:
        nw, nh = size, int(size * h / w)
    else:
        nh, nw = size, int(size * w / h)
    return nw, nh, round((nw - size) / 2), round((nh - size) / 2)


def resample_unclamped(img, bounds, coeffs, axis):
    """one pass along `axis` of an integer image: the accumulators after the shift, BEFORE the clamp (int64)"""
    img = np.moveaxis(np.asarray(img, np.int64), axis, 0)
    out = np.empty((len(bounds),) + img.shape[1:], np.int64)
    for i, (first, taps) in enumerate(bounds):
        k = coeffs[i, :taps].reshape((taps,) + (1,) * (img.ndim - 1))
        out[i] = ((1 << (PRECISION_BITS - 1)) + (img[first:first + taps] * k).sum(0)) >> PRECISION_BITS
    return np.moveaxis(out, 0, axis)


def process_frame(frame, size, want_unclamped=False):
    """frame (H, W, 3) uint8 -> (size, size, 3) f32: what _process_frame returns.  want_unclamped: also the list of the
    passes' unclamped accumulators (over the cropped window)"""
    frame = np.asarray(frame)
    assert frame.dtype == np.uint8 and frame.ndim == 3 and frame.shape[2] == 3
    h, w = frame.shape[:2]
    nw, nh, left, top = target(h, w, size)
    raw = []
    img = frame
    if nw != w:
        b, k = pass_tables(w, nw)
        acc = resample_unclamped(img, b[left:left + size], k[left:left + size], 1)
        raw.append(acc)
        img = np.clip(acc, 0, 255).astype(np.uint8)
    else:
        img = img[:, left:left + size]
    if nh != h:
        b, k = pass_tables(h, nh)
        acc = resample_unclamped(img, b[top:top + size], k[top:top + size], 0)
        raw.append(acc)
        img = np.clip(acc, 0, 255).astype(np.uint8)
    else:
        img = img[top:top + size]
    out = img.astype(np.float32) / np.float32(127.5) - np.float32(1)
    assert out.dtype == np.float32 and out.shape == (size, size, 3)
    return (out, raw) if want_unclamped else out


def process_frames(frames, size):
    return np.stack([process_frame(f, size) for f in frames])


# ---------------------------------------------------------------- the cases of the kernel tests
# (h, w, size): each the smallest shape that reaches one way to go wrong
SHAPES = [
    (37, 61, 16), (61, 37, 16),       # both passes, landscape and portrait
    (16, 16, 16),                     # nothing to resize: both passes skipped (the whole scale table)
    (16, 40, 16), (40, 16, 16),       # the short side already has `size` samples
    (9, 23, 16),                      # upscaling: 5 taps, windows clipped at both borders
    (32, 42, 16), (32, 46, 16),       # crop offsets 2.5 -> 2 and 3.5 -> 4, horizontally
    (42, 32, 16), (46, 32, 16),       # ... and vertically
    (300, 300, 16),                   # 77 taps
    (64, 400, 16),                    # 17 taps, crop from a wide resized image
    (5, 300, 16),                     # extreme aspect ratio, both passes upscale
]
PATTERNS = ("random", "zeros", "ones", "row_stripes", "col_stripes")
T = 3


def make_frames(h, w, pattern, seed=0):
    """(T, h, w, 3) uint8, the T frames different in content"""
    rng = np.random.default_rng([seed, h, w])
    if pattern == "random":
        f = rng.integers(0, 256, (T, h, w, 3), dtype=np.uint8)
        if h * w * 3 >= 256:
            f.reshape(T, -1)[0, :256] = np.arange(256, dtype=np.uint8)      # every byte value
        return f
    if pattern == "zeros":
        return np.zeros((T, h, w, 3), np.uint8)
    if pattern == "ones":
        return np.full((T, h, w, 3), 255, np.uint8)
    f = np.zeros((T, h, w, 3), np.uint8)
    for t in range(T):            # single-pixel stripes of 0 / 255, phase and polarity differ per frame
        if pattern == "row_stripes":
            f[t, (t & 1)::2] = 255
        else:
            f[t, :, (t & 1)::2] = 255
        if t == 2:
            f[t] = 255 - f[t]
            f[t, h // 2:, w // 2:] = rng.integers(0, 2, (h - h // 2, w - w // 2, 1), dtype=np.uint8) * 255
    return f


@functools.lru_cache(maxsize=None)
def expected(h, w, size, pattern):
    """process_frames(make_frames(h, w, pattern), size), computed once per session and read-only"""
    out = process_frames(make_frames(h, w, pattern), size)
    out.setflags(write=False)
    return out
