"""The 4-bit (MXFP4) decode weights on the CPU: the numpy restatement of the format against the E2M1_VALUES table, the
quantiser and the GEMV of csrc/gemv_w4.h host-emulated through the C ABI -- the quantiser bitwise against the restatement,
the GEMV bitwise (outputs AND workspace partials) against lwm_gemv_fused_bf16 on the dequantised weights -- the refusals,
and the ABI mirror.  Every check is exact."""
import ctypes as C

import numpy as np
import pytest

from lwm_amd import _capi
from oracle import attention_ref as R
from tests import _emu, _kv4_ref as K4, _w4_ref as W4, _w8_ref as W8

POISON = 0x7fc1          # a bf16 NaN pattern / the top half of an f32 NaN


def emu_quantise(w, in_place=False):
    """w (K, N) f32 of bf16 values -> (codes u8 (K/4, N/8, 16), scale bytes u8 (K/32, N), rounded f32) through lwm_w4_quantise"""
    L = _emu.lib()
    K, N = w.shape
    wb = _emu.bf16_array(w)
    q = _emu.aligned((K // 4, N // 8, 16), np.uint8)
    s = _emu.aligned((K // 32, N), np.uint8)
    rb = wb if in_place else _emu.aligned((K, N), np.uint16)
    q[...] = 0xa5
    s[...] = 0
    _capi.check(L, L.lwm_w4_quantise(wb.ctypes.data, q.ctypes.data, s.ctypes.data, rb.ctypes.data, K, N, None), "lwm_w4_quantise")
    return q, s, R.from_bf16_bits(rb)


def emu_gemv(x, mats, *, w4, norm=None, residual=None, want_ss=False, want_f32=False, guard=0):
    """One call of lwm_gemv_fused_w4 (mats = [(codes, scale bytes)]) or lwm_gemv_fused_bf16 (mats = [w f32 of bf16 values])
    -> ([y], ss_out or None, the workspace partials).  guard > 0: every output and the workspace sit inside poisoned
    margins of `guard` elements, and the margins must come back as they went in."""
    L = _emu.lib()
    rows, K = x.shape
    n = len(mats)
    Ns = [(m[1] if w4 else m).shape[1] for m in mats]
    xb = _emu.bf16_array(x)
    guards = []

    def out(shape, dtype):
        size = int(np.prod(shape))
        buf = _emu.aligned((size + 2 * guard,), dtype)
        buf.view(np.uint16 if dtype == np.uint16 else np.uint32)[...] = POISON if dtype == np.uint16 else 0x7fc12345
        guards.append((buf, size))
        return buf[guard:guard + size].reshape(shape)

    assert guard % 8 == 0
    work = out((sum(max(L.lwm_gemv_workspace_bytes(rows, K, N), 16) for N in Ns) // 4,), np.float32)
    a = (_capi.LwmGemvW4Args if w4 else _capi.LwmGemvArgs)()
    a.x, a.ldx, a.nmat, a.rows, a.K, a.workspace = xb.ctypes.data, K, n, rows, K, work.ctypes.data
    keep, ys = [], []
    for i, m in enumerate(mats):
        if w4:
            q, s = _emu.aligned(m[0].shape, np.uint8), _emu.aligned(m[1].shape, np.uint8)
            q[...], s[...] = m
            a.w[i], a.w_scale[i] = q.ctypes.data, s.ctypes.data
            keep += [q, s]
        else:
            wb = _emu.bf16_array(m)
            a.w[i] = wb.ctypes.data
            keep.append(wb)
        a.N[i] = Ns[i]
        y = out((rows, Ns[i]), np.float32 if want_f32 else np.uint16)
        if want_f32:
            a.y_f32[i] = y.ctypes.data
        else:
            a.y[i], a.ldy[i] = y.ctypes.data, Ns[i]
        ys.append(y)
    if norm is not None:
        ss, gam, eps = norm
        ssa, gb = _emu.aligned(ss.shape, np.float32), _emu.bf16_array(gam)
        ssa[...] = ss
        a.norm_weight, a.ss_in, a.ss_n, a.eps = gb.ctypes.data, ssa.ctypes.data, ss.shape[1], eps
        keep += [ssa, gb]
    if residual is not None:
        rb = _emu.bf16_array(residual)
        a.residual[0], a.ldres[0] = rb.ctypes.data, Ns[0]
        keep.append(rb)
    sso = None
    if want_ss:
        sso = out((rows, Ns[0] // 128), np.float32)
        a.ss_out = sso.ctypes.data
    fn, name = (L.lwm_gemv_fused_w4, "lwm_gemv_fused_w4") if w4 else (L.lwm_gemv_fused_bf16, "lwm_gemv_fused_bf16")
    _capi.check(L, fn(C.byref(a), None), name)
    for buf, size in guards:
        pat = POISON if buf.dtype == np.uint16 else 0x7fc12345
        v = buf.view(np.uint16 if buf.dtype == np.uint16 else np.uint32)
        assert (v[:guard] == pat).all() and (v[guard + size:] == pat).all(), "a write outside its buffer"
    used = sum(L.lwm_gemv_workspace_bytes(rows, K, N) for N in Ns) // 4
    assert (work.view(np.uint32)[used:] == 0x7fc12345).all(), "a write past the workspace the entry asked for"
    return [y.copy() for y in ys], (None if sso is None else sso.copy()), work[:used].copy()


# ---------------------------------------------------------------- the restatement itself
def test_restatement_against_the_e2m1_table():
    from lwm_amd.kv4 import E2M1_VALUES
    table = np.array(E2M1_VALUES, np.float64)
    assert np.array_equal(K4.e2m1_decode(np.arange(16, dtype=np.uint8)), table)
    assert np.array_equal(np.signbit(K4.e2m1_decode(np.arange(16, dtype=np.uint8))), np.signbit(table))
    for name, w in W4.quantiser_cases():
        K, N = w.shape
        q, e = W4.quantise(w)
        assert q.shape == (K // 4, N // 8, 16) and q.dtype == np.uint8 and e.shape == (K // 32, N) and e.dtype == np.uint8, name
        s = np.repeat(2.0 ** (e.astype(np.float64) - 127), 32, axis=0)
        y = w.astype(np.float64) / s
        assert np.abs(y).max() <= 6, name                                               # nothing saturates
        codes = W4.unpack_codes(q, (K, N))
        assert np.array_equal(W4.pack_codes(codes), q), name                             # the two statements of the layout agree
        # nearest table entry, ties to the even code, the sign of zero kept
        d = np.abs(np.abs(y)[..., None] - table[:8])
        assert (np.abs(table[codes] - y) == d.min(-1)).all(), name
        tie = d.min(-1) == np.sort(d, -1)[..., 1]
        assert (codes[tie] % 2 == 0).all(), name
        assert np.array_equal(codes >> 3, np.signbit(w).astype(np.uint8)), name
        # the smallest power of two: half of it no longer fits (except at the lower clamp and for all-zero blocks)
        amax = np.abs(w.astype(np.float64)).reshape(K // 32, 32, N).max(1)
        sb = 2.0 ** (e.astype(np.float64) - 127)
        free = (amax > 0) & (e > 1)
        assert (amax[free] / (sb[free] / 2.0) > 6).all() and (amax / sb <= 6).all(), name
        assert (e[amax == 0] == 127).all() and e.min() >= 1 and e.max() <= 254, name
        assert np.array_equal(W4.dequant(q, e, (K, N)), table[codes] * s), name


def test_the_mantissa_threshold_and_the_clamp():
    (_, w), = [c for c in W4.quantiser_cases() if c[0].startswith("threshold")]
    q, e = W4.quantise(w)
    for c, ex in enumerate((-100, -20, 0, 1, 40, 100)):
        assert e[0, c] == 127 + ex - 2 and e[1, c] == 127 + ex - 1       # 1.5 * 2^e fits 2^(e-2); its bf16 successor does not
    assert e[0, 9] == 127 and W4.unpack_codes(q, w.shape)[5, 9] == 8      # an all-zero block; -0 keeps its sign
    assert e[0, 10] == 1                                                  # the lower clamp
    d = W4.dequant(q, e, w.shape)
    assert d[0, 10] == 2.0 ** -127 and d[4, 10] == 3 * 2.0 ** -126 and d[6, 10] == 0 and np.signbit(d[6, 10])


# ---------------------------------------------------------------- quantiser kernel
@pytest.mark.parametrize("case", W4.quantiser_cases(), ids=lambda c: c[0])
def test_quantiser_equals_the_restatement(case):
    name, w = case
    q_ref, e_ref = W4.quantise(w)
    r_ref = W4.rounded(q_ref, e_ref, w.shape)
    for in_place in (False, True):
        q, e, r = emu_quantise(w, in_place)
        assert np.array_equal(e, e_ref)
        assert np.array_equal(q, q_ref)
        assert np.array_equal(R.to_bf16_bits(r), R.to_bf16_bits(r_ref))              # bitwise: the sign of zero too


def test_quantising_twice_is_idempotent():
    """the rounded weights are a fixed point: e2m1(q) * s still fits 6 s in every block, and where the scale halves the
    codes double -- the values stay (a block that rounded to all zeros takes byte 127, the rule for amax == 0)"""
    for _, w in W4.quantiser_cases()[:2]:
        q, e, r = emu_quantise(w)
        q2, e2, r2 = emu_quantise(r)
        zero = np.abs(r).reshape(-1, 32, w.shape[1]).max(1) == 0
        assert np.array_equal(R.to_bf16_bits(r), R.to_bf16_bits(r2)) and (e2[~zero] <= e[~zero]).all() and (e2[zero] == 127).all()
        assert np.array_equal(W4.dequant(q2, e2, w.shape), W4.dequant(q, e, w.shape))


# ---------------------------------------------------------------- GEMV
def _packs(ws):
    packs = [W4.quantise(w) for w in ws]
    deq = [W4.dequant(q, e, w.shape).astype(np.float32) for (q, e), w in zip(packs, ws)]
    for d in deq:                                       # the test's domain: every rounded weight IS a bf16 value
        assert np.array_equal(R.round_bf16(d), d)
    for _, e in packs:
        assert e.min() >= 127 - 40 and e.max() <= 127 + 40
    return packs, deq


def _same(got, ref, f32):
    view = np.uint32 if f32 else np.uint16
    return all(np.array_equal(g.view(view), r.view(view)) for g, r in zip(got, ref))


@pytest.mark.parametrize("rows", [1, 2, 3, 4])
@pytest.mark.parametrize("K,Ns", W8.GEMV_SHAPES, ids=lambda v: str(v).replace(" ", ""))
def test_gemv_equals_the_bf16_gemv_on_the_rounded_weights(rows, K, Ns):
    x, ws = W4.gemv_case(rows, K, Ns)
    packs, deq = _packs(ws)
    for f32 in (False, True):
        got, _, work = emu_gemv(x, packs, w4=True, want_f32=f32, guard=64)
        ref, _, rwork = emu_gemv(x, deq, w4=False, want_f32=f32)
        assert np.array_equal(work.view(np.uint32), rwork.view(np.uint32))           # every partial, bit for bit
        assert _same(got, ref, f32)
        assert all(np.any(g) for g in got)


@pytest.mark.parametrize("rows", [1, 4])
@pytest.mark.parametrize("K,N", [(160, 48), (416, 2064)])
def test_gemv_norm_on_load(rows, K, N):
    x, ws = W4.gemv_case(rows, K, (N, 16))
    packs, deq = _packs(ws)
    rng = np.random.default_rng(5)
    gam = R.round_bf16((1.0 + 0.2 * rng.standard_normal(K)).astype(np.float32))
    for n_ss in (1, 5, 64):
        ss = np.zeros((rows, n_ss), np.float32)
        ss[...] = rng.dirichlet(np.ones(n_ss), size=rows) * (x.astype(np.float64) ** 2).sum(-1, keepdims=True)
        for f32 in (False, True):
            got, _, work = emu_gemv(x, packs, w4=True, norm=(ss, gam, 1e-6), want_f32=f32, guard=64)
            ref, _, rwork = emu_gemv(x, deq, w4=False, norm=(ss, gam, 1e-6), want_f32=f32)
            assert np.array_equal(work.view(np.uint32), rwork.view(np.uint32))
            assert _same(got, ref, f32)
        plain, _, _ = emu_gemv(x, packs, w4=True, want_f32=True)
        assert not np.array_equal(plain[0], got[0])                                   # the norm did something


@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("K,N", [(160, 128), (416, 1152)])
def test_gemv_residual_and_ss_out(rows, K, N):
    x, ws = W4.gemv_case(rows, K, (N,))
    packs, deq = _packs(ws)
    res = R.round_bf16(np.random.default_rng(6).standard_normal((rows, N)).astype(np.float32) * 4.0)
    (g,), gss, work = emu_gemv(x, packs, w4=True, residual=res, want_ss=True, guard=64)
    (r,), rss, rwork = emu_gemv(x, deq, w4=False, residual=res, want_ss=True)
    assert np.array_equal(work.view(np.uint32), rwork.view(np.uint32))
    assert np.array_equal(g, r) and np.array_equal(gss.view(np.uint32), rss.view(np.uint32))
    (plain,), _, _ = emu_gemv(x, packs, w4=True)
    assert not np.array_equal(plain, g)


def test_gemv_through_the_quantiser_kernel():
    """the two kernels together: quantise with the kernel, stream its codes, compare with the bf16 GEMV on ITS rounded weights"""
    x, (w,) = W4.gemv_case(2, 416, (1040,))
    q, e, r = emu_quantise(w)
    (g,), _, work = emu_gemv(x, [(q, e)], w4=True, want_f32=True)
    (y,), _, rwork = emu_gemv(x, [r], w4=False, want_f32=True)
    assert np.array_equal(g.view(np.uint32), y.view(np.uint32)) and np.array_equal(work.view(np.uint32), rwork.view(np.uint32))
    # and the rounding moved the result by no more than the format allows: neighbouring e2m1 values are at most 2 apart
    # (4 and 6), so |e2m1(w/s) - w/s| <= 1, and amax / s > 3 (half the scale would fit otherwise; the lower clamp is far
    # away here): |e2m1(w/s) s - w| <= s < amax / 3 per element of a block (far from tight; a sanity bound on the
    # scales' placement)
    exact = x.astype(np.float64) @ w.astype(np.float64)
    amax = np.repeat(np.abs(w.astype(np.float64)).reshape(-1, 32, w.shape[1]).max(1), 32, axis=0)
    assert (np.abs(g - exact) <= np.abs(x).astype(np.float64) @ (amax / 3.0) + 1e-30).all()


# ---------------------------------------------------------------- validation
def _valid_args(rows=2, K=64, N=32):
    bufs = dict(x=_emu.aligned((rows, K), np.uint16), q=_emu.aligned((K // 4, N // 8, 16), np.uint8), s=_emu.aligned((K // 32, N), np.uint8),
                y=_emu.aligned((rows, N), np.uint16), yf=_emu.aligned((rows, N), np.float32),
                work=_emu.aligned((rows * N,), np.float32), res=_emu.aligned((rows, N), np.uint16),
                gam=_emu.aligned((K,), np.uint16), ss=_emu.aligned((rows, 4), np.float32), sso=_emu.aligned((rows, 1), np.float32))
    bufs["s"][...] = 127
    a = _capi.LwmGemvW4Args()
    a.x, a.ldx, a.nmat, a.rows, a.K = bufs["x"].ctypes.data, K, 1, rows, K
    a.w[0], a.w_scale[0], a.y[0], a.ldy[0], a.N[0] = bufs["q"].ctypes.data, bufs["s"].ctypes.data, bufs["y"].ctypes.data, N, N
    a.y_f32[0] = bufs["yf"].ctypes.data
    a.workspace = bufs["work"].ctypes.data
    return a, bufs


def _poison(bufs):
    bufs["y"][...] = POISON
    bufs["yf"].view(np.uint32)[...] = 0x7fc12345
    bufs["work"].view(np.uint32)[...] = 0x7fc12345
    bufs["sso"].view(np.uint32)[...] = 0x7fc12345


def _untouched(bufs):
    return (bufs["y"] == POISON).all() and all((bufs[k].view(np.uint32) == 0x7fc12345).all() for k in ("yf", "work", "sso"))


EINVAL, EUNSUP = _capi.LWM_EINVAL, _capi.LWM_EUNSUPPORTED
REFUSALS = {
    "rows > 4": (EUNSUP, lambda a, b: setattr(a, "rows", 5)),
    "K % 32": (EUNSUP, lambda a, b: setattr(a, "K", 48)),
    "K > 12288": (EUNSUP, lambda a, b: (setattr(a, "K", 12320), setattr(a, "ldx", 12320))),
    "N % 8": (EUNSUP, lambda a, b: a.N.__setitem__(0, 20)),
    "N <= 0": (EUNSUP, lambda a, b: a.N.__setitem__(0, 0)),
    "misaligned codes": (EINVAL, lambda a, b: a.w.__setitem__(0, b["q"].ctypes.data + 8)),
    "misaligned scales": (EINVAL, lambda a, b: a.w_scale.__setitem__(0, b["s"].ctypes.data + 8)),
    "null scales": (EINVAL, lambda a, b: a.w_scale.__setitem__(0, None)),
    "null codes": (EINVAL, lambda a, b: a.w.__setitem__(0, None)),
    "null x": (EINVAL, lambda a, b: setattr(a, "x", None)),
    "null workspace": (EINVAL, lambda a, b: setattr(a, "workspace", None)),
    "misaligned workspace": (EINVAL, lambda a, b: setattr(a, "workspace", b["work"].ctypes.data + 4)),
    "ldx < K": (EINVAL, lambda a, b: setattr(a, "ldx", 32)),
    "no output": (EINVAL, lambda a, b: (a.y.__setitem__(0, None), a.y_f32.__setitem__(0, None))),
    "misaligned y": (EINVAL, lambda a, b: a.y.__setitem__(0, b["y"].ctypes.data + 2)),
    "ldy < N": (EINVAL, lambda a, b: a.ldy.__setitem__(0, 16)),
    "misaligned y_f32": (EINVAL, lambda a, b: a.y_f32.__setitem__(0, b["yf"].ctypes.data + 4)),
    "no matrices": (EINVAL, lambda a, b: setattr(a, "nmat", 0)),
    "four matrices": (EINVAL, lambda a, b: setattr(a, "nmat", 4)),
    "negative rows": (EINVAL, lambda a, b: setattr(a, "rows", -1)),
    "norm without ss_in": (EINVAL, lambda a, b: setattr(a, "norm_weight", b["gam"].ctypes.data)),
    "norm with 65 partials": (EINVAL, lambda a, b: (setattr(a, "norm_weight", b["gam"].ctypes.data), setattr(a, "ss_in", b["ss"].ctypes.data),
                                                    setattr(a, "ss_n", 65))),
    "ss_out with N % 128": (EINVAL, lambda a, b: setattr(a, "ss_out", b["sso"].ctypes.data)),
    "ss_out with two matrices": (EINVAL, lambda a, b: (setattr(a, "ss_out", b["sso"].ctypes.data), setattr(a, "nmat", 2))),
    "residual without a bf16 output": (EINVAL, lambda a, b: (a.residual.__setitem__(0, b["res"].ctypes.data), a.ldres.__setitem__(0, 32),
                                                             a.y.__setitem__(0, None))),
    "residual with ldres < N": (EINVAL, lambda a, b: (a.residual.__setitem__(0, b["res"].ctypes.data), a.ldres.__setitem__(0, 16))),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_gemv_refusals_touch_nothing(name):
    L = _emu.lib()
    code, edit = REFUSALS[name]
    a, bufs = _valid_args()
    edit(a, bufs)
    _poison(bufs)
    assert L.lwm_gemv_fused_w4(C.byref(a), None) == code
    assert L.lwm_last_error() and b"gemv_w4" in L.lwm_last_error()
    assert _untouched(bufs)


def test_the_unedited_arguments_are_accepted():
    """... so the table above is not vacuous; rows == 0 is a no-op; a null struct is refused"""
    L = _emu.lib()
    a, bufs = _valid_args()
    _poison(bufs)
    assert L.lwm_gemv_fused_w4(C.byref(a), None) == _capi.LWM_OK
    assert not (bufs["y"] == POISON).any() and (bufs["yf"] == 0).all()
    a.rows = 0
    _poison(bufs)
    assert L.lwm_gemv_fused_w4(C.byref(a), None) == _capi.LWM_OK and _untouched(bufs)
    assert L.lwm_gemv_fused_w4(None, None) == EINVAL


def test_quantiser_refusals_touch_nothing():
    L = _emu.lib()
    K, N = 64, 32
    w, r = _emu.aligned((K, N), np.uint16), _emu.aligned((K, N), np.uint16)
    q, s = _emu.aligned((K // 4, N // 8, 16), np.uint8), _emu.aligned((K // 32, N), np.uint8)

    def call(wp=None, qp=None, sp=None, rp=None, K=K, N=N):
        q[...], r[...], s[...] = 0xa5, POISON, 0xa5
        pick = lambda v, d: d.ctypes.data if v is None else v
        rc = L.lwm_w4_quantise(pick(wp, w), pick(qp, q), pick(sp, s), pick(rp, r), K, N, None)
        clean = (q == 0xa5).all() and (r == POISON).all() and (s == 0xa5).all()
        return rc, clean

    assert call() == (_capi.LWM_OK, False)
    for kw, code in ((dict(K=48), EUNSUP), (dict(K=12320), EUNSUP), (dict(N=20), EUNSUP), (dict(N=4), EUNSUP), (dict(K=0), EINVAL),
                     (dict(N=-16), EINVAL), (dict(wp=0), EINVAL), (dict(qp=0), EINVAL), (dict(sp=0), EINVAL), (dict(rp=0), EINVAL),
                     (dict(wp=w.ctypes.data + 2), EINVAL), (dict(qp=q.ctypes.data + 8), EINVAL),
                     (dict(sp=s.ctypes.data + 8), EINVAL), (dict(rp=r.ctypes.data + 8), EINVAL)):
        assert call(**kw) == (code, True), kw
        assert b"w4_quantise" in L.lwm_last_error()


def test_quantiser_writes_inside_its_buffers():
    """a ragged column tile (N = 528: the second tile has 16 columns) with poisoned margins around all three outputs"""
    L = _emu.lib()
    w = W4.quantiser_cases()[0][1]
    K, N = w.shape
    wb = _emu.bf16_array(w)
    G = 64
    qb, sb, rb = (_emu.aligned((n + 2 * G,), t) for n, t in ((K * N // 2, np.uint8), (K // 32 * N, np.uint8), (K * N, np.uint16)))
    qb[...], sb[...], rb[...] = 0xa5, 0xa5, POISON
    _capi.check(L, L.lwm_w4_quantise(wb.ctypes.data, qb[G:].ctypes.data, sb[G:].ctypes.data, rb[G:].ctypes.data, K, N, None), "lwm_w4_quantise")
    for buf, pat in ((qb, 0xa5), (sb, 0xa5), (rb, POISON)):
        assert (buf[:G] == pat).all() and (buf[-G:] == pat).all()
    q_ref, e_ref = W4.quantise(w)
    assert np.array_equal(qb[G:-G].reshape(q_ref.shape), q_ref) and np.array_equal(sb[G:-G].reshape(e_ref.shape), e_ref)


# ---------------------------------------------------------------- ABI
def test_abi_mirror():
    L = _emu.lib()
    assert L.lwm_version() >= 580
    assert L.lwm_sizeof(11) == C.sizeof(_capi.LwmGemvW4Args)
    assert C.sizeof(_capi.LwmGemvW4Args) == C.sizeof(_capi.LwmGemvArgs) + 3 * C.sizeof(C.c_void_p)
