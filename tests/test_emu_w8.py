"""The 8-bit (e4m3) decode weights on the CPU: the numpy restatement of the format against torch.float8_e4m3fn, the
quantiser and the GEMV of csrc/gemv_w8.h host-emulated through the C ABI -- the quantiser bitwise against the restatement,
the GEMV bitwise (outputs AND workspace partials) against lwm_gemv_fused_bf16 on the dequantised weights -- the refusals,
and the ABI mirror."""
import ctypes as C

import numpy as np
import pytest

from lwm_amd import _capi
from oracle import attention_ref as R
from tests import _emu, _kv8_ref as K8, _w8_ref as W8

POISON = 0x7fc1          # a bf16 NaN pattern / the top half of an f32 NaN


def emu_quantise(w, in_place=False):
    """w (K, N) f32 of bf16 values -> (q u8, scale f32, rounded f32) through lwm_w8_quantise"""
    L = _emu.lib()
    K, N = w.shape
    wb = _emu.bf16_array(w)
    q = _emu.aligned((K, N), np.uint8)
    s = _emu.aligned((W8.groups(K), N), np.float32)
    rb = wb if in_place else _emu.aligned((K, N), np.uint16)
    q[...] = 0x7f
    s[...] = np.nan
    _capi.check(L, L.lwm_w8_quantise(wb.ctypes.data, q.ctypes.data, s.ctypes.data, rb.ctypes.data, K, N, None), "lwm_w8_quantise")
    return q, s, R.from_bf16_bits(rb)


def emu_gemv(x, mats, *, w8, norm=None, residual=None, want_ss=False, want_f32=False):
    """One call of lwm_gemv_fused_w8 (mats = [(q, scale)]) or lwm_gemv_fused_bf16 (mats = [w f32 of bf16 values]) ->
    ([y], ss_out or None, the workspace partials)"""
    L = _emu.lib()
    rows, K = x.shape
    n = len(mats)
    Ns = [(m[0] if w8 else m).shape[1] for m in mats]
    xb = _emu.bf16_array(x)
    work = _emu.aligned((sum(max(L.lwm_gemv_workspace_bytes(rows, K, N), 16) for N in Ns) // 4,), np.float32)
    a = (_capi.LwmGemvW8Args if w8 else _capi.LwmGemvArgs)()
    a.x, a.ldx, a.nmat, a.rows, a.K, a.workspace = xb.ctypes.data, K, n, rows, K, work.ctypes.data
    keep, ys = [], []
    for i, m in enumerate(mats):
        if w8:
            q, s = _emu.aligned(m[0].shape, np.uint8), _emu.aligned(m[1].shape, np.float32)
            q[...], s[...] = m
            a.w[i], a.w_scale[i] = q.ctypes.data, s.ctypes.data
            keep += [q, s]
        else:
            wb = _emu.bf16_array(m)
            a.w[i] = wb.ctypes.data
            keep.append(wb)
        a.N[i] = Ns[i]
        y = _emu.aligned((rows, Ns[i]), np.float32 if want_f32 else np.uint16)
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
        sso = _emu.aligned((rows, Ns[0] // 128), np.float32)
        a.ss_out = sso.ctypes.data
    fn, name = (L.lwm_gemv_fused_w8, "lwm_gemv_fused_w8") if w8 else (L.lwm_gemv_fused_bf16, "lwm_gemv_fused_bf16")
    _capi.check(L, fn(C.byref(a), None), name)
    return [y.copy() for y in ys], sso, work


# ---------------------------------------------------------------- the restatement itself
def test_restatement_rounds_like_torch_float8():
    import torch
    for name, w in W8.quantiser_cases():
        q, s = W8.quantise(w)
        sx = np.repeat(s, W8.GROUP, axis=0)[:w.shape[0]]
        with np.errstate(under="ignore"):
            y = w / sx
        assert np.abs(y).max() <= 448, name
        ref = torch.from_numpy(y).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
        assert np.array_equal(q, ref), name
        assert not np.isin(q, (0x7f, 0xff)).any(), name                                   # never a NaN byte
        assert np.array_equal(np.frexp(s)[0], np.full(s.shape, 0.5, np.float32)), name    # powers of two
        # the smallest power of two: half of it no longer fits (except at the lower clamp and for all-zero groups)
        for g in range(s.shape[0]):
            amax = np.abs(w[g * 128:(g + 1) * 128]).max(0).astype(np.float64)
            free = (amax > 0) & (s[g] > 2.0 ** -126)
            assert (amax[free] / (s[g][free] / 2.0) > 448).all() and (amax / s[g] <= 448).all(), name
            assert (s[g][amax == 0] == 1).all(), name


def test_short_last_group_takes_its_own_rows_only():
    (_, w), = [c for c in W8.quantiser_cases() if c[0].startswith("short")]
    q, s = W8.quantise(w)
    assert s.shape == (2, 48) and s[1, 7] == 1 and s[1, 8] == 2.0 ** -5 and s[0, 9] == 1
    assert np.array_equal(W8.dequant(q, s)[128:, 8], w[128:, 8])


# ---------------------------------------------------------------- quantiser kernel
@pytest.mark.parametrize("case", W8.quantiser_cases(), ids=lambda c: c[0])
def test_quantiser_equals_the_restatement(case):
    name, w = case
    q_ref, s_ref = W8.quantise(w)
    r_ref = W8.rounded(q_ref, s_ref)
    for in_place in (False, True):
        q, s, r = emu_quantise(w, in_place)
        assert np.array_equal(q, q_ref)
        assert np.array_equal(s.view(np.uint32), s_ref.view(np.uint32))
        assert np.array_equal(R.to_bf16_bits(r), R.to_bf16_bits(r_ref))              # bitwise: the sign of zero too
    # negative zero keeps its sign in the bytes
    if name.startswith("edge_128"):
        assert (q_ref[[5, 10], 1] == 0x80).all()


def test_quantising_twice_keeps_the_values():
    """the rounded weights are a fixed point of the rounding (the scale of a group whose amax rounded down may halve, with
    the bytes doubling: the values stay)"""
    w = W8.quantiser_cases()[0][1]
    q, s, r = emu_quantise(w)
    q2, s2, r2 = emu_quantise(r)
    assert np.array_equal(R.to_bf16_bits(r), R.to_bf16_bits(r2)) and (s2 <= s).all()
    assert np.array_equal(W8.dequant(q2, s2), W8.dequant(q, s))


# ---------------------------------------------------------------- GEMV
def _packs(ws):
    packs = [W8.quantise(w) for w in ws]
    deq = [W8.dequant(q, s) for q, s in packs]
    for d in deq:                                       # the test's domain: every rounded weight IS a bf16 value
        assert np.array_equal(R.round_bf16(d), d)
    for _, s in packs:
        assert (s >= 2.0 ** -40).all() and (s <= 2.0 ** 40).all()
    return packs, deq


@pytest.mark.parametrize("rows", [1, 2, 3, 4])
@pytest.mark.parametrize("K,Ns", W8.GEMV_SHAPES, ids=lambda v: str(v).replace(" ", ""))
def test_gemv_equals_the_bf16_gemv_on_the_rounded_weights(rows, K, Ns):
    x, ws = W8.gemv_case(rows, K, Ns)
    packs, deq = _packs(ws)
    for f32 in (False, True):
        got, _, work = emu_gemv(x, packs, w8=True, want_f32=f32)
        ref, _, rwork = emu_gemv(x, deq, w8=False, want_f32=f32)
        assert np.array_equal(work.view(np.uint32), rwork.view(np.uint32))           # every partial, bit for bit
        for g, r in zip(got, ref):
            assert np.array_equal(g.view(np.uint32 if f32 else np.uint16), r.view(np.uint32 if f32 else np.uint16))
        assert any(np.any(g) for g in got)


@pytest.mark.parametrize("rows", [1, 4])
@pytest.mark.parametrize("K,N", [(160, 48), (416, 2064)])
def test_gemv_norm_on_load(rows, K, N):
    x, ws = W8.gemv_case(rows, K, (N, 16))
    packs, deq = _packs(ws)
    rng = np.random.default_rng(5)
    gam = R.round_bf16((1.0 + 0.2 * rng.standard_normal(K)).astype(np.float32))
    for n_ss in (1, 5, 64):
        ss = np.zeros((rows, n_ss), np.float32)
        parts = rng.dirichlet(np.ones(n_ss), size=rows) * (x.astype(np.float64) ** 2).sum(-1, keepdims=True)
        ss[...] = parts
        got, _, work = emu_gemv(x, packs, w8=True, norm=(ss, gam, 1e-6))
        ref, _, rwork = emu_gemv(x, deq, w8=False, norm=(ss, gam, 1e-6))
        assert np.array_equal(work.view(np.uint32), rwork.view(np.uint32))
        assert all(np.array_equal(g, r) for g, r in zip(got, ref))
        plain, _, _ = emu_gemv(x, packs, w8=True)
        assert not np.array_equal(plain[0], got[0])                                   # the norm did something


@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("K,N", [(160, 128), (416, 1152)])
def test_gemv_residual_and_ss_out(rows, K, N):
    x, ws = W8.gemv_case(rows, K, (N,))
    packs, deq = _packs(ws)
    res = R.round_bf16(np.random.default_rng(6).standard_normal((rows, N)).astype(np.float32) * 4.0)
    (g,), gss, work = emu_gemv(x, packs, w8=True, residual=res, want_ss=True)
    (r,), rss, rwork = emu_gemv(x, deq, w8=False, residual=res, want_ss=True)
    assert np.array_equal(work.view(np.uint32), rwork.view(np.uint32))
    assert np.array_equal(g, r) and np.array_equal(gss.view(np.uint32), rss.view(np.uint32))
    (plain,), _, _ = emu_gemv(x, packs, w8=True)
    assert not np.array_equal(plain, g)


def test_gemv_through_the_quantiser_kernel():
    """the two kernels together: quantise with the kernel, stream its bytes, compare with the bf16 GEMV on ITS rounded weights"""
    x, (w,) = W8.gemv_case(2, 416, (1040,))
    q, s, r = emu_quantise(w)
    (g,), _, work = emu_gemv(x, [(q, s)], w8=True, want_f32=True)
    (y,), _, rwork = emu_gemv(x, [r], w8=False, want_f32=True)
    assert np.array_equal(g.view(np.uint32), y.view(np.uint32)) and np.array_equal(work.view(np.uint32), rwork.view(np.uint32))
    # and the rounding moved the result by no more than the format allows: |e4m3(w/s) s - w| <= 2^-4 |w| for normal q, so
    # the product differs by at most 2^-4 sum |x||w| (far from tight; a sanity bound on the scales' placement)
    exact = x.astype(np.float64) @ w.astype(np.float64)
    bound = 2.0 ** -4 * (np.abs(x).astype(np.float64) @ np.abs(w).astype(np.float64)) + 1e-30
    assert (np.abs(g - exact) <= bound).all()


# ---------------------------------------------------------------- validation
def _valid_args(rows=2, K=64, N=32):
    bufs = dict(x=_emu.aligned((rows, K), np.uint16), q=_emu.aligned((K, N), np.uint8), s=_emu.aligned((1, N), np.float32),
                y=_emu.aligned((rows, N), np.uint16), yf=_emu.aligned((rows, N), np.float32),
                work=_emu.aligned((rows * N,), np.float32), res=_emu.aligned((rows, N), np.uint16),
                gam=_emu.aligned((K,), np.uint16), ss=_emu.aligned((rows, 4), np.float32), sso=_emu.aligned((rows, 1), np.float32))
    bufs["s"][...] = 1.0
    a = _capi.LwmGemvW8Args()
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
    "misaligned bytes": (EINVAL, lambda a, b: a.w.__setitem__(0, b["q"].ctypes.data + 8)),
    "misaligned scales": (EINVAL, lambda a, b: a.w_scale.__setitem__(0, b["s"].ctypes.data + 4)),
    "null scales": (EINVAL, lambda a, b: a.w_scale.__setitem__(0, None)),
    "null bytes": (EINVAL, lambda a, b: a.w.__setitem__(0, None)),
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
    assert L.lwm_gemv_fused_w8(C.byref(a), None) == code
    assert L.lwm_last_error() and b"gemv_w8" in L.lwm_last_error()
    assert _untouched(bufs)


def test_the_unedited_arguments_are_accepted():
    """... so the table above is not vacuous; rows == 0 is a no-op; a null struct is refused"""
    L = _emu.lib()
    a, bufs = _valid_args()
    _poison(bufs)
    assert L.lwm_gemv_fused_w8(C.byref(a), None) == _capi.LWM_OK
    assert not (bufs["y"] == POISON).any() and (bufs["yf"] == 0).all()
    a.rows = 0
    _poison(bufs)
    assert L.lwm_gemv_fused_w8(C.byref(a), None) == _capi.LWM_OK and _untouched(bufs)
    assert L.lwm_gemv_fused_w8(None, None) == EINVAL


def test_quantiser_refusals_touch_nothing():
    L = _emu.lib()
    K, N = 64, 32
    w, r = _emu.aligned((K, N), np.uint16), _emu.aligned((K, N), np.uint16)
    q, s = _emu.aligned((K, N), np.uint8), _emu.aligned((1, N), np.float32)

    def call(wp=None, qp=None, sp=None, rp=None, K=K, N=N):
        q[...], r[...] = 0x7f, POISON
        s.view(np.uint32)[...] = 0x7fc12345
        pick = lambda v, d: d.ctypes.data if v is None else v
        rc = L.lwm_w8_quantise(pick(wp, w), pick(qp, q), pick(sp, s), pick(rp, r), K, N, None)
        clean = (q == 0x7f).all() and (r == POISON).all() and (s.view(np.uint32) == 0x7fc12345).all()
        return rc, clean

    assert call() == (_capi.LWM_OK, False)
    for kw, code in ((dict(K=48), EUNSUP), (dict(K=12320), EUNSUP), (dict(N=20), EUNSUP), (dict(N=4), EUNSUP), (dict(K=0), EINVAL),
                     (dict(N=-16), EINVAL), (dict(wp=0), EINVAL), (dict(qp=0), EINVAL), (dict(sp=0), EINVAL), (dict(rp=0), EINVAL),
                     (dict(wp=w.ctypes.data + 2), EINVAL), (dict(qp=q.ctypes.data + 8), EINVAL),
                     (dict(sp=s.ctypes.data + 4), EINVAL), (dict(rp=r.ctypes.data + 8), EINVAL)):
        assert call(**kw) == (code, True), kw
        assert b"w8_quantise" in L.lwm_last_error()


# ---------------------------------------------------------------- ABI
def test_abi_mirror():
    L = _emu.lib()
    assert L.lwm_version() >= 550
    assert L.lwm_sizeof(9) == C.sizeof(_capi.LwmGemvW8Args)
    assert C.sizeof(_capi.LwmGemvW8Args) == C.sizeof(_capi.LwmGemvArgs) + 3 * C.sizeof(C.c_void_p)
