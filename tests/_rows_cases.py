"""The checks of lwm_gemm_rows_fused_bf16 / lwm_gemm_rows_fused_w8 (csrc/gemm_rows.h), written once over a small buffer
backend so that tests/test_emu_rows.py (host emulation, numpy buffers) and tests/test_gpu_rows.py (device buffers) run the
same code.  The refusal table runs against lwm_gemv_fused_bf16 / lwm_gemv_fused_w8 too (entry="gemv"), with what those
entries answer differently written down beside it.  TEST INFRASTRUCTURE ONLY.

A backend has lib() -> the bound C ABI, buf(array) -> a guarded, initialised buffer with .ptr, .read() (a numpy copy) and
.intact() (both guard bands untouched), and sync().  Every buffer a call can write is poison-filled first; run() asserts
after every call that no guard band and no byte of the workspace past the documented size was written, and that the
inputs are what they were."""
import ctypes as C

import numpy as np

from lwm_amd import _capi
from oracle import attention_ref as R
from tests import _w8_ref as W8

GUARD = 256
FILL = 0xA5
POISON16 = 0x7fc1                 # a bf16 NaN
POISON32 = 0x7fc12345             # an f32 NaN
TAIL = 64                         # floats of workspace past the documented size: must stay poison

KS_ = (32, 128, 160, 384)         # one partial; one full group; a short last group; three groups
NSETS = ((8,), (520,), (64, 1032), (520, 64, 1032))        # the minimum; a ragged last column tile; two and three matrices
ROWS = (1, 5, 15, 16, 17, 32)
SS_NS = ((128,), (384,))          # one matrix with N % 128 == 0 (ss_out): one and two column tiles


class HostBuf:
    def __init__(self, arr):
        arr = np.ascontiguousarray(arr)
        n = arr.nbytes
        raw = np.full(n + 2 * GUARD + 16, FILL, np.uint8)
        off = (-(raw.ctypes.data + GUARD)) % 16
        self.raw, self.lo, self.n = raw, off + GUARD, n
        self.view = raw[self.lo:self.lo + n].view(arr.dtype).reshape(arr.shape)
        self.view[...] = arr
        self.ptr = self.view.ctypes.data if n else raw.ctypes.data + self.lo

    def read(self):
        return self.view.copy()

    def intact(self):
        return bool((self.raw[:self.lo] == FILL).all() and (self.raw[self.lo + self.n:] == FILL).all())


class HostBackend:
    def lib(self):
        from tests import _emu
        return _emu.lib()

    def buf(self, arr):
        return HostBuf(arr)

    def sync(self):
        pass


def poison(shape, dtype):
    if np.dtype(dtype) == np.uint16:
        return np.full(shape, POISON16, np.uint16)
    return np.full(shape, POISON32, np.uint32).view(np.float32)


def is_poison(a):
    a = np.asarray(a)
    return bool((a.view(np.uint16) == POISON16).all()) if a.dtype == np.uint16 else bool((a.view(np.uint32) == POISON32).all())


def run(B, x, mats, *, entry="rows", w8=False, norm=None, residual=None, want_ss=False, want_f32=False, expect=_capi.LWM_OK):
    """One call.  x (rows, K) f32 of bf16 values; mats = [W (K, N) f32 of bf16 values] or, w8, [(q u8, scale f32)];
    norm = (ss_in (rows, n) f32, gamma (K,), eps); residual (rows, N_0); entry "rows" = the new entries, "gemv" = the GEMV's.
    -> dict(y=[uint16 bits or f32], ss=f32 or None, work=f32 partials as written)"""
    L = B.lib()
    rows, K = x.shape
    Ns = [(m[0] if w8 else m).shape[1] for m in mats]
    ws_fn = L.lwm_gemm_rows_workspace_bytes if entry == "rows" else L.lwm_gemv_workspace_bytes
    need = sum(ws_fn(rows, K, N) for N in Ns) // 4
    assert need == W8.groups(K) * rows * sum(Ns)
    xb = B.buf(R.to_bf16_bits(x))
    work = B.buf(poison((need + TAIL,), np.float32))
    a = (_capi.LwmGemvW8Args if w8 else _capi.LwmGemvArgs)()
    a.x, a.ldx, a.nmat, a.rows, a.K, a.workspace = xb.ptr, K, len(mats), rows, K, work.ptr
    inputs, ys = [(xb, R.to_bf16_bits(x))], []
    for i, m in enumerate(mats):
        if w8:
            q, s = B.buf(m[0]), B.buf(m[1])
            a.w[i], a.w_scale[i] = q.ptr, s.ptr
            inputs += [(q, m[0]), (s, m[1])]
        else:
            wb = B.buf(R.to_bf16_bits(m))
            a.w[i] = wb.ptr
            inputs.append((wb, R.to_bf16_bits(m)))
        a.N[i] = Ns[i]
        y = B.buf(poison((rows, Ns[i]), np.float32 if want_f32 else np.uint16))
        if want_f32:
            a.y_f32[i] = y.ptr
        else:
            a.y[i], a.ldy[i] = y.ptr, Ns[i]
        ys.append(y)
    if norm is not None:
        ss, gam, eps = norm
        ssa, gb = B.buf(np.asarray(ss, np.float32)), B.buf(R.to_bf16_bits(gam))
        a.norm_weight, a.ss_in, a.ss_n, a.eps = gb.ptr, ssa.ptr, ss.shape[1], eps
        inputs += [(ssa, np.asarray(ss, np.float32)), (gb, R.to_bf16_bits(gam))]
    if residual is not None:
        rb = B.buf(R.to_bf16_bits(residual))
        a.residual[0], a.ldres[0] = rb.ptr, Ns[0]
        inputs.append((rb, R.to_bf16_bits(residual)))
    sso = None
    if want_ss:
        sso = B.buf(poison((rows, Ns[0] // 128), np.float32))
        a.ss_out = sso.ptr
    name = ("lwm_gemm_rows_fused_" if entry == "rows" else "lwm_gemv_fused_") + ("w8" if w8 else "bf16")
    rc = getattr(L, name)(C.byref(a), None)
    B.sync()
    assert rc == expect, (name, rc, L.lwm_last_error())
    assert all(b.intact() for b, _ in inputs) and all(y.intact() for y in ys) and work.intact(), "a guard band was written"
    assert sso is None or sso.intact()
    for b, was in inputs:
        assert np.array_equal(b.read().view(np.uint8), np.ascontiguousarray(was).view(np.uint8)), "an input was modified"
    wk = work.read()
    assert is_poison(wk[need:]), "the workspace was written past its documented size"
    out = dict(y=[y.read() for y in ys], ss=None if sso is None else sso.read(), work=wk[:need])
    if rc == _capi.LWM_OK:
        assert not np.isnan(wk[:need]).any(), "a partial was left unwritten"
    return out


# ---------------------------------------------------------------- data
def exact_case(rows, K, Ns, seed=0):
    """small integers: |x| <= 4, |W| <= 8 (e4m3-exact), so every partial sum is an integer below 2^24"""
    rng = np.random.default_rng(7000 + 100 * K + 10 * sum(Ns) + rows + seed)
    x = rng.integers(-4, 5, size=(rows, K)).astype(np.float32)
    ws = [rng.integers(-8, 9, size=(K, N)).astype(np.float32) for N in Ns]
    return x, ws


def random_case(rows, K, Ns, seed=0):
    rng = np.random.default_rng(9000 + 100 * K + 10 * sum(Ns) + rows + seed)
    x = R.round_bf16(rng.standard_normal((rows, K)).astype(np.float32))
    ws = [R.round_bf16((rng.standard_normal((K, N)) * 0.5).astype(np.float32)) for N in Ns]
    return x, ws


def norm_case(x, n_ss, seed=5):
    """(ss_in (rows, n_ss) whose rows sum to about sum x^2, gamma (K,), eps)"""
    rng = np.random.default_rng(seed + n_ss)
    rows, K = x.shape
    gam = R.round_bf16((1.0 + 0.2 * rng.standard_normal(K)).astype(np.float32))
    ss = (rng.dirichlet(np.ones(n_ss), size=rows) * (x.astype(np.float64) ** 2).sum(-1, keepdims=True)).astype(np.float32)
    return ss, gam, 1e-6


def quantise(B, w):
    """w (K, N) f32 of bf16 values -> (q u8, scale f32, rounded f32 of bf16 values) through lwm_w8_quantise"""
    L = B.lib()
    K, N = w.shape
    src = B.buf(R.to_bf16_bits(w))
    q, s = B.buf(np.full((K, N), 0x7f, np.uint8)), B.buf(poison((W8.groups(K), N), np.float32))
    r = B.buf(poison((K, N), np.uint16))
    _capi.check(L, L.lwm_w8_quantise(src.ptr, q.ptr, s.ptr, r.ptr, K, N, None), "lwm_w8_quantise")
    B.sync()
    assert q.intact() and s.intact() and r.intact()
    return q.read(), s.read(), R.from_bf16_bits(r.read())


def bits(a):
    return np.asarray(a).view(np.uint16 if a.dtype == np.uint16 else np.uint32)


def same(a, b):
    return all(np.array_equal(bits(u), bits(v)) for u, v in zip(a["y"], b["y"])) and \
        (a["ss"] is None or np.array_equal(bits(a["ss"]), bits(b["ss"])))


# ---------------------------------------------------------------- the reduce kernel's ss_out, restated
def ss_out_ref(y):
    """y (rows, N) f32 of the bf16 outputs -> (rows, N / 128) f32: per 128 columns, every quad of four columns is an fmaf
    chain from zero; the 8 quads of a wave meet pairwise (quads q, q^1; then pairs; then fours) and the four waves' sums are
    added in wave order -- gemv_reduce_kernel + block_sum_256"""
    rows, N = y.shape
    out = np.zeros((rows, N // 128), np.float32)
    for r in range(rows):
        for c in range(N // 128):
            o = y[r, 128 * c:128 * (c + 1)].astype(np.float64).reshape(32, 4)
            sq = np.zeros(32, np.float32)
            for j in range(4):
                sq = (o[:, j] * o[:, j] + sq.astype(np.float64)).astype(np.float32)      # one rounding: the operands are short
            v = sq.reshape(4, 8)
            for m in (1, 2, 4):
                v = (v + v[:, np.arange(8) ^ m]).astype(np.float32)
            w = v[:, 0]
            out[r, c] = np.float32(np.float32(np.float32(w[0] + w[1]) + w[2]) + w[3])
    return out


# ---------------------------------------------------------------- 1. exact cases
def check_exact(B, rows, K, Ns):
    x, ws = exact_case(rows, K, Ns)
    ref = [x.astype(np.int64) @ w.astype(np.int64) for w in ws]
    assert max(np.abs(r).max() for r in ref) < 2 ** 24
    packs = [W8.quantise(w) for w in ws]
    assert all(np.array_equal(W8.dequant(q, s), w) for (q, s), w in zip(packs, ws))
    for w8, mats in ((False, ws), (True, packs)):
        f = run(B, x, mats, w8=w8, want_f32=True)
        b = run(B, x, mats, w8=w8)
        for i, r in enumerate(ref):
            assert np.array_equal(f["y"][i], r.astype(np.float32)), (w8, i)
            assert np.array_equal(b["y"][i], R.to_bf16_bits(r.astype(np.float32))), (w8, i)
        # the partials add up to the product too, each an exact integer
        assert np.array_equal(f["work"], b["work"])
    if rows <= 4:
        for f32 in (False, True):
            g = run(B, x, ws, entry="gemv", want_f32=f32)
            n = run(B, x, ws, want_f32=f32)
            assert all(np.array_equal(u, v) for u, v in zip(g["y"], n["y"])) and np.array_equal(g["work"], n["work"])


def check_exact_residual_ss(B, rows, K, Ns):
    (N,) = Ns
    x, (w,) = exact_case(rows, K, Ns, seed=1)
    res = np.random.default_rng(K + N + rows).integers(-300, 301, size=(rows, N)).astype(np.float32)
    res = R.round_bf16(res)
    prod = R.round_bf16((x.astype(np.int64) @ w.astype(np.int64)).astype(np.float32))
    want = R.round_bf16(prod + res)                       # bf16(bf16(x . W) + res): the f32 sum of two bf16 values is exact here
    for w8, mats in ((False, [w]), (True, [W8.quantise(w)])):
        o = run(B, x, mats, w8=w8, residual=res, want_ss=True)
        assert np.array_equal(o["y"][0], R.to_bf16_bits(want)), w8
        assert np.array_equal(bits(o["ss"]), bits(ss_out_ref(want))), w8
    if rows <= 4:
        assert same(run(B, x, [w], entry="gemv", residual=res, want_ss=True), o)


# ---------------------------------------------------------------- 2. random data against fp64
def _bound_check(out_f32, out_bf16, xs, ws, K):
    for i, w in enumerate(ws):
        ref = xs.astype(np.float64) @ w.astype(np.float64)
        mag = np.abs(xs).astype(np.float64) @ np.abs(w).astype(np.float64)
        bound = K * 2.0 ** -23 * mag                      # f32 accumulation in any order over exact bf16 x bf16 products
        err = np.abs(out_f32["y"][i].astype(np.float64) - ref)
        print(f"  matrix {i}: max err/bound f32 {np.max(err / np.maximum(bound, 1e-300)):.3g}")
        assert (err <= bound).all(), i
        errb = np.abs(R.from_bf16_bits(out_bf16["y"][i]).astype(np.float64) - ref)
        assert (errb <= bound + 2.0 ** -8 * np.abs(ref)).all(), i


def check_random(B, rows, K, Ns):
    x, ws = random_case(rows, K, Ns)
    _bound_check(run(B, x, ws, want_f32=True), run(B, x, ws), x, ws, K)


def gemv_normalised(B, x, norm):
    """the normalised x that lwm_gemv_fused_bf16 feeds its FMAs, read out through an identity matrix (every output is one
    product with 1 plus zeros: exact), four rows at a time"""
    rows, K = x.shape
    eye = np.eye(K, dtype=np.float32)
    ss, gam, eps = norm
    out = [run(B, x[r:r + 4], [eye], entry="gemv", norm=(ss[r:r + 4], gam, eps), want_f32=True)["y"][0] for r in range(0, rows, 4)]
    return np.concatenate(out)


def check_norm(B, rows, K, Ns, n_ss):
    x, ws = random_case(rows, K, Ns, seed=3)
    norm = norm_case(x, n_ss)
    xn = gemv_normalised(B, x, norm)
    assert np.array_equal(R.round_bf16(xn), xn)
    # (a sanity check of the reference itself: it IS the RMSNorm of x, to bf16 rounding)
    ss, gam, eps = norm
    approx = x / np.sqrt(ss.astype(np.float64).sum(-1, keepdims=True) / K + eps) * gam
    assert np.allclose(xn, approx, rtol=2.0 ** -6, atol=1e-6)
    # the new entry feeds the matrix pipe the same bits
    mine = run(B, x, [np.eye(K, dtype=np.float32)], norm=norm, want_f32=True)["y"][0]
    assert np.array_equal(bits(mine), bits(xn))
    _bound_check(run(B, x, ws, norm=norm, want_f32=True), run(B, x, ws, norm=norm), xn, ws, K)


# ---------------------------------------------------------------- 3. packs
def check_packs(B, rows, K, Ns):
    x, ws = W8.gemv_case(rows, K, Ns)
    qs = [quantise(B, w) for w in ws]
    packs, rounded = [(q, s) for q, s, _ in qs], [r for _, _, r in qs]
    for _, s in packs:
        assert (s >= 2.0 ** -40).all() and (s <= 2.0 ** 40).all()
    variants = [dict(), dict(want_f32=True), dict(norm=norm_case(x, 32))]
    if len(Ns) == 1 and Ns[0] % 128 == 0:
        res = R.round_bf16(np.random.default_rng(6).standard_normal((rows, Ns[0])).astype(np.float32) * 4.0)
        variants += [dict(residual=res, want_ss=True), dict(residual=res, want_ss=True, norm=norm_case(x, 1))]
    elif len(Ns) == 1:
        res = R.round_bf16(np.random.default_rng(6).standard_normal((rows, Ns[0])).astype(np.float32) * 4.0)
        variants += [dict(residual=res)]
    for kw in variants:
        got = run(B, x, packs, w8=True, **kw)
        ref = run(B, x, rounded, **kw)
        assert np.array_equal(bits(got["work"]), bits(ref["work"])), list(kw)          # every partial, bit for bit
        assert same(got, ref), list(kw)
        assert any(np.any(y) for y in got["y"])


# ---------------------------------------------------------------- 4. row independence
def check_row_independence(B, K, Ns, with_fused):
    x32, ws = random_case(32, K, Ns, seed=11)
    x32[9] = x32[30]                                      # duplicates inside one call
    x32[17] = x32[2]
    rng = np.random.default_rng(K + sum(Ns))
    kw32, res32, norm32 = {}, None, None
    if with_fused:
        res32 = R.round_bf16(rng.standard_normal((32, Ns[0])).astype(np.float32) * 4.0)
        res32[9], res32[17] = res32[30], res32[2]
        norm32 = norm_case(x32, 32)
        norm32[0][9], norm32[0][17] = norm32[0][30], norm32[0][2]
        kw32 = dict(residual=res32, norm=norm32)
    outs = (False,) if with_fused else (False, True)       # (a residual goes with a bf16 output)
    big = [run(B, x32, ws, want_f32=f, **kw32) for f in outs]
    for o in big:
        for y in o["y"]:
            assert np.array_equal(bits(y)[9], bits(y)[30]) and np.array_equal(bits(y)[17], bits(y)[2])
    for r, slot in ((0, 3), (7, 0), (15, 4), (16, 1), (21, 2), (31, 0)):
        x5 = R.round_bf16(rng.standard_normal((5, K)).astype(np.float32) * 3.0)        # other neighbours
        x5[slot] = x32[r]
        kw5 = {}
        if with_fused:
            res5 = R.round_bf16(rng.standard_normal((5, Ns[0])).astype(np.float32))
            res5[slot] = res32[r]
            n5 = norm_case(x5, 32, seed=77)
            n5[0][slot] = norm32[0][r]
            kw5 = dict(residual=res5, norm=(n5[0], norm32[1], norm32[2]))
        for f, o32 in zip(outs, big):
            o5 = run(B, x5, ws, want_f32=f, **kw5)
            for y5, y32 in zip(o5["y"], o32["y"]):
                assert np.array_equal(bits(y5)[slot], bits(y32)[r]), (r, slot, f)


# ---------------------------------------------------------------- 5. refusals
def valid_args(B, w8, rows=5, K=64, N=128):
    bufs = dict(x=B.buf(np.zeros((rows, K), np.uint16)), w=B.buf(np.zeros((K, N), np.uint8 if w8 else np.uint16)),
                s=B.buf(np.ones((1, N), np.float32)), y=B.buf(poison((rows, N), np.uint16)), yf=B.buf(poison((rows, N), np.float32)),
                work=B.buf(poison((2 * rows * N + TAIL,), np.float32)), res=B.buf(np.zeros((rows, N), np.uint16)),
                gam=B.buf(np.zeros((K,), np.uint16)), ss=B.buf(np.ones((rows, 4), np.float32)), sso=B.buf(poison((rows, 1), np.float32)))
    a = (_capi.LwmGemvW8Args if w8 else _capi.LwmGemvArgs)()
    a.x, a.ldx, a.nmat, a.rows, a.K = bufs["x"].ptr, K, 1, rows, K
    a.w[0], a.y[0], a.ldy[0], a.N[0], a.y_f32[0] = bufs["w"].ptr, bufs["y"].ptr, N, N, bufs["yf"].ptr
    if w8:
        a.w_scale[0] = bufs["s"].ptr
    a.workspace = bufs["work"].ptr
    return a, bufs


def untouched(bufs):
    return all(is_poison(bufs[k].read()) and bufs[k].intact() for k in ("y", "yf", "work", "sso"))


EINVAL, EUNSUP = _capi.LWM_EINVAL, _capi.LWM_EUNSUPPORTED


def _second_matrix(a, b):
    a.nmat = 2
    a.w[1], a.y[1], a.ldy[1], a.N[1] = a.w[0], a.y[0], a.ldy[0], a.N[0]
    if hasattr(a, "w_scale"):
        a.w_scale[1] = a.w_scale[0]


REFUSALS = {
    "rows 0": (EUNSUP, lambda a, b: setattr(a, "rows", 0)),
    "rows 33": (EUNSUP, lambda a, b: setattr(a, "rows", 33)),
    "negative rows": (EINVAL, lambda a, b: setattr(a, "rows", -1)),
    "K % 32": (EUNSUP, lambda a, b: setattr(a, "K", 48)),
    "K > 12288": (EUNSUP, lambda a, b: (setattr(a, "K", 12320), setattr(a, "ldx", 12320))),
    "N % 8": (EUNSUP, lambda a, b: a.N.__setitem__(0, 20)),
    "N <= 0": (EUNSUP, lambda a, b: a.N.__setitem__(0, 0)),
    "no matrices": (EINVAL, lambda a, b: setattr(a, "nmat", 0)),
    "four matrices": (EINVAL, lambda a, b: setattr(a, "nmat", 4)),
    "null x": (EINVAL, lambda a, b: setattr(a, "x", None)),
    "null w": (EINVAL, lambda a, b: a.w.__setitem__(0, None)),
    "null workspace": (EINVAL, lambda a, b: setattr(a, "workspace", None)),
    "misaligned x": (EINVAL, lambda a, b: setattr(a, "x", b["x"].ptr + 8)),
    "ldx % 8": (EINVAL, lambda a, b: setattr(a, "ldx", 68)),
    "ldx < K": (EINVAL, lambda a, b: setattr(a, "ldx", 32)),
    "misaligned w": (EINVAL, lambda a, b: a.w.__setitem__(0, b["w"].ptr + 8)),
    "misaligned workspace": (EINVAL, lambda a, b: setattr(a, "workspace", b["work"].ptr + 4)),
    "misaligned y": (EINVAL, lambda a, b: a.y.__setitem__(0, b["y"].ptr + 2)),
    "ldy < N": (EINVAL, lambda a, b: a.ldy.__setitem__(0, 16)),
    "misaligned y_f32": (EINVAL, lambda a, b: a.y_f32.__setitem__(0, b["yf"].ptr + 4)),
    "no output": (EINVAL, lambda a, b: (a.y.__setitem__(0, None), a.y_f32.__setitem__(0, None))),
    "norm without ss_in": (EINVAL, lambda a, b: setattr(a, "norm_weight", b["gam"].ptr)),
    "misaligned norm_weight": (EINVAL, lambda a, b: (setattr(a, "norm_weight", b["gam"].ptr + 2), setattr(a, "ss_in", b["ss"].ptr),
                                                     setattr(a, "ss_n", 4))),
    "norm with 65 partials": (EINVAL, lambda a, b: (setattr(a, "norm_weight", b["gam"].ptr), setattr(a, "ss_in", b["ss"].ptr),
                                                    setattr(a, "ss_n", 65))),
    "ss_out with two matrices": (EINVAL, lambda a, b: (_second_matrix(a, b), setattr(a, "ss_out", b["sso"].ptr))),
    "ss_out with N % 128": (EINVAL, lambda a, b: (a.N.__setitem__(0, 64), a.ldy.__setitem__(0, 64), setattr(a, "ss_out", b["sso"].ptr))),
    "residual with two matrices": (EINVAL, lambda a, b: (_second_matrix(a, b), a.residual.__setitem__(0, b["res"].ptr),
                                                         a.ldres.__setitem__(0, 128))),
    "residual without a bf16 output": (EINVAL, lambda a, b: (a.residual.__setitem__(0, b["res"].ptr), a.ldres.__setitem__(0, 128),
                                                             a.y.__setitem__(0, None))),
    "residual with ldres < N": (EINVAL, lambda a, b: (a.residual.__setitem__(0, b["res"].ptr), a.ldres.__setitem__(0, 16))),
    "misaligned residual": (EINVAL, lambda a, b: (a.residual.__setitem__(0, b["res"].ptr + 2), a.ldres.__setitem__(0, 128))),
}
W8_REFUSALS = {
    "null scales": (EINVAL, lambda a, b: a.w_scale.__setitem__(0, None)),
    "misaligned scales": (EINVAL, lambda a, b: a.w_scale.__setitem__(0, b["s"].ptr + 4)),
}


# What the GEMV entries (lwm_gemv_fused_bf16 / _w8) answer differently: x and norm_weight are read by the element and a
# residual belongs to its matrix, so these edits are ACCEPTED there; no rows is a call that does nothing; the limit is 4 rows.
GEMV_ACCEPTS = ("misaligned x", "ldx % 8", "misaligned norm_weight", "residual with two matrices")
GEMV_REFUSALS = {k: v for k, v in REFUSALS.items() if k not in GEMV_ACCEPTS + ("rows 0",)} | {
    "rows 5": (EUNSUP, lambda a, b: setattr(a, "rows", 5)),
}
ENTRY_ROWS = {"rows": 5, "gemv": 2}


def entry_fn(L, entry, w8):
    """-> (the C entry, the tag that opens its lwm_last_error() texts)"""
    if entry == "rows":
        return (L.lwm_gemm_rows_fused_w8, b"gemm_rows_w8: ") if w8 else (L.lwm_gemm_rows_fused_bf16, b"gemm_rows: ")
    return (L.lwm_gemv_fused_w8, b"gemv_w8: ") if w8 else (L.lwm_gemv_fused_bf16, b"gemv: ")


def check_refusal(B, w8, name, entry="rows"):
    L = B.lib()
    code, edit = (REFUSALS | GEMV_REFUSALS | W8_REFUSALS)[name]
    assert name in W8_REFUSALS or name in (REFUSALS if entry == "rows" else GEMV_REFUSALS)
    a, bufs = valid_args(B, w8, rows=ENTRY_ROWS[entry])
    edit(a, bufs)
    fn, tag = entry_fn(L, entry, w8)
    assert fn(C.byref(a), None) == code
    B.sync()
    assert L.lwm_last_error() and L.lwm_last_error().startswith(tag)
    assert untouched(bufs)


def check_gemv_accepts(B, w8, name):
    """the edits of GEMV_ACCEPTS, which the rows entries refuse, run on the GEMV entries (x = 0 or a guard band's small
    values against W = 0: every output is a zero); no rows: LWM_OK and nothing is written"""
    L = B.lib()
    a, bufs = valid_args(B, w8, rows=ENTRY_ROWS["gemv"])
    fn, _ = entry_fn(L, "gemv", w8)
    if name == "rows 0":
        a.rows = 0
        assert fn(C.byref(a), None) == _capi.LWM_OK
        B.sync()
        assert untouched(bufs)
        return
    REFUSALS[name][1](a, bufs)
    assert fn(C.byref(a), None) == _capi.LWM_OK, L.lwm_last_error()
    B.sync()
    used = a.nmat * a.rows * a.N[0]                         # (K = 64: one partial per output)
    assert (bufs["y"].read() == 0).all() and (bufs["yf"].read() == 0).all() and is_poison(bufs["work"].read()[used:])
    assert all(b.intact() for b in bufs.values())


def check_accepted(B, w8, entry="rows"):
    """... so the table above is not vacuous; a null struct is refused"""
    L = B.lib()
    rows = ENTRY_ROWS[entry]
    a, bufs = valid_args(B, w8, rows=rows)
    fn, tag = entry_fn(L, entry, w8)
    assert fn(C.byref(a), None) == _capi.LWM_OK
    B.sync()
    assert (bufs["y"].read() == 0).all() and (bufs["yf"].read() == 0).all() and is_poison(bufs["work"].read()[rows * 128:])
    assert all(b.intact() for b in bufs.values())
    assert fn(None, None) == EINVAL and L.lwm_last_error().startswith(tag)
    ws = L.lwm_gemm_rows_workspace_bytes if entry == "rows" else L.lwm_gemv_workspace_bytes
    assert ws(rows, 64, 128) == rows * 128 * 4 and ws(0, 64, 128) == 0
