"""The kernels either side of attention at edge shapes and values, on the host emulator (tests/emu) through the C ABI:
the cases, the float64 references with their magnitudes and the per-element verdict are tests/_elem_cases.py's; the device
runs the same ones in tests/test_gpu_elem_edges.py.  Also here: the mutant self-check -- the verdict must FAIL a
reference with one term damaged, and the max-norm bounds the suite had before let most of those through."""
import ctypes as C

import numpy as np
import pytest

from lwm_amd import _capi
from oracle.attention_ref import from_bf16_bits, round_bf16, to_bf16_bits
from tests import _elem_cases as E, _emu

FLAVOURS = [pytest.param(False, id="bf16"), pytest.param(True, id="f32")]
PAD, POISON = 8, 0xFF


def _sfx(f32):
    return "f32" if f32 else "bf16"


def _fn(name, f32):
    return getattr(_emu.lib(), f"lwm_{name}_{_sfx(f32)}")


def _in(x, f32):
    a = _emu.aligned(np.shape(x), np.float32 if f32 else np.uint16)
    a[...] = x if f32 else to_bf16_bits(np.asarray(x, np.float32))
    return a


def _out(shape, f32):
    a = _emu.aligned(shape, np.float32 if f32 else np.uint16)
    a.view(np.uint8)[...] = POISON                       # (what the kernel must overwrite: NaN bits)
    return a


def _dec(a, f32):
    return np.array(a, np.float32) if f32 else from_bf16_bits(np.ascontiguousarray(a))


def _ok(rc, what):
    _capi.check(_emu.lib(), rc, what)


def _i32(x):
    a = _emu.aligned(np.shape(x), np.int32)
    a[...] = x
    return a


# ---------------------------------------------------------------- RoPE
def _rope_raw(xa, ya, tab, pos, conj, f32):
    B, S, H, D = xa.shape
    t4 = _emu._t4f if f32 else _emu._t4
    _ok(_fn("rope", f32)(t4(xa), t4(ya), tab.ctypes.data, pos.ctypes.data, B, S, H, D, tab.shape[0], int(conj), None), "lwm_rope")


_TABS = {}


def _tab(case):
    if case.name not in _TABS:
        _TABS[case.name] = _in(case.table, True)
    return _TABS[case.name]


@pytest.mark.parametrize("f32", FLAVOURS)
@pytest.mark.parametrize("case", E.rope_cases(), ids=repr)
def test_rope(case, f32):
    """forward and conjugate against fp64, per element; the same call on views into wider buffers whose gaps hold NaN
    bits (and in place, as the fused q | k rotation runs it): the contiguous call's bits, no gap byte touched"""
    v = E.Verdict("emu", f32)
    x = case.x(f32)
    tab, pos = _tab(case), _i32(case.pos)
    xa = _in(x, f32)
    dense = {}
    for conj in (False, True):
        ya = _out(x.shape, f32)
        _rope_raw(xa, ya, tab, pos, conj, f32)
        dense[conj] = ya
        E.verify_rope(case, _dec(ya, f32), conj, v)
    B, S, H, D = x.shape
    dt = np.float32 if f32 else np.uint16
    xbuf, ybuf = _emu.aligned((B, S, H, D + PAD), dt), _emu.aligned((B, S, H, D + PAD), dt)
    for conj in (False, True):
        for b in (xbuf, ybuf):
            b.view(np.uint8)[...] = POISON
        xbuf[..., :D] = xa
        _rope_raw(xbuf[..., :D], ybuf[..., :D], tab, pos, conj, f32)
        assert np.array_equal(np.ascontiguousarray(ybuf[..., :D]).view(np.uint8), dense[conj].view(np.uint8))
        _rope_raw(xbuf[..., :D], xbuf[..., :D], tab, pos, conj, f32)                 # in place
        assert np.array_equal(np.ascontiguousarray(xbuf[..., :D]).view(np.uint8), dense[conj].view(np.uint8))
        for b in (xbuf, ybuf):
            assert (np.ascontiguousarray(b[..., D:]).view(np.uint8) == POISON).all(), "a gap byte was written"


# ---------------------------------------------------------------- RMSNorm
def _rms(case, f32):
    L = _emu.lib()
    x, w, g, res = case.ops(f32)
    rows, Cc = x.shape
    xa, wa, ga = _in(x, f32), _in(w, f32), _in(g, f32)
    y, rstd = _out((rows, Cc), f32), _out((rows,), True)
    _ok(_fn("rmsnorm_fwd", f32)(xa.ctypes.data, wa.ctypes.data, y.ctypes.data, rstd.ctypes.data, rows, Cc, E.EPS, None), "rmsnorm_fwd")
    got = dict(y=_dec(y, f32), rstd=np.array(rstd))
    if case.fwd_only:
        return got
    ws = _emu.aligned((max(L.lwm_rmsnorm_bwd_workspace_bytes(rows, Cc), 16) // 4,), np.float32)
    ws[...] = np.nan                                     # (a partial nobody wrote must not be summed)
    dx, dw = _out((rows, Cc), f32), _out((Cc,), f32)
    _ok(_fn("rmsnorm_bwd", f32)(xa.ctypes.data, wa.ctypes.data, ga.ctypes.data, rstd.ctypes.data, dx.ctypes.data, dw.ctypes.data,
                                ws.ctypes.data, rows, Cc, None), "rmsnorm_bwd")
    got.update(dx=_dec(dx, f32), dw=_dec(dw, f32))
    if not f32:
        ra = _in(res, f32)
        ws[...] = np.nan
        dx1, dw1 = _out((rows, Cc), f32), _out((Cc,), f32)
        _ok(L.lwm_rmsnorm_bwd_res_bf16(xa.ctypes.data, wa.ctypes.data, ga.ctypes.data, rstd.ctypes.data, ra.ctypes.data, dx1.ctypes.data,
                                       dw1.ctypes.data, ws.ctypes.data, rows, Cc, None), "rmsnorm_bwd_res")
        got.update(dx_res=_dec(dx1, f32), dw_res=_dec(dw1, f32))
    return got


def _ids(names):
    """[(name, f32)] of both flavours as pytest params"""
    return [pytest.param(n, f32, id=f"{n if isinstance(n, str) else 'x'.join(map(str, n[:2]))}-{_sfx(f32)}")
            for f32 in (False, True) for n in names(f32)]


@pytest.mark.parametrize("shape,f32", _ids(E.rms_shapes))
def test_rmsnorm(shape, f32):
    case = E.rms_case(*shape)
    E.verify_rms(case, _rms(case, f32), E.Verdict("emu", f32))


# ---------------------------------------------------------------- SwiGLU
def _swiglu(case, f32):
    a, b, g = case.ops(f32)
    n = a.size
    aa, ba, ga = _in(a.reshape(-1), f32), _in(b.reshape(-1), f32), _in(g.reshape(-1), f32)
    y, da, db = (_out((n,), f32) for _ in range(3))
    _ok(_fn("swiglu_fwd", f32)(aa.ctypes.data, ba.ctypes.data, y.ctypes.data, n, None), "swiglu_fwd")
    _ok(_fn("swiglu_bwd", f32)(aa.ctypes.data, ba.ctypes.data, ga.ctypes.data, da.ctypes.data, db.ctypes.data, n, None), "swiglu_bwd")
    return dict(y=y, da=da, db=db)


@pytest.mark.parametrize("f32", FLAVOURS)
@pytest.mark.parametrize("case", E.swiglu_cases(), ids=repr)
def test_swiglu(case, f32):
    got = _swiglu(case, f32)
    E.verify_swiglu(case, {n: _dec(t, f32).reshape(case.shape) for n, t in got.items()}, E.Verdict("emu", f32))


@pytest.mark.parametrize("case", E.swiglu_halves_cases(), ids=repr)
def test_swiglu_halves(case):
    """gate | up as the halves of one (rows, 2F) buffer, d gate | d up into the halves of another, the output and the
    upstream gradient rows of wider buffers too, NaN bits in every gap: the flat kernels' bits, and those against fp64"""
    L = _emu.lib()
    a, b, g = case.ops(False)
    rows, F = a.shape
    flat = _swiglu(case, False)
    y13, d13 = _out((rows, 2 * F + PAD), False), _out((rows, 2 * F + PAD), False)
    yb, gb = _out((rows, F + PAD), False), _out((rows, F + PAD), False)
    y13[:, :F], y13[:, F:2 * F], gb[:, :F] = to_bf16_bits(a), to_bf16_bits(b), to_bf16_bits(g)
    ld = 2 * F + PAD
    _ok(L.lwm_swiglu_fwd_ld_bf16(y13.ctypes.data, ld, y13.ctypes.data + 2 * F, ld, yb.ctypes.data, F + PAD, rows, F, None), "swiglu_fwd_ld")
    _ok(L.lwm_swiglu_bwd_ld_bf16(y13.ctypes.data, ld, y13.ctypes.data + 2 * F, ld, gb.ctypes.data, F + PAD, d13.ctypes.data, ld,
                                 d13.ctypes.data + 2 * F, ld, rows, F, None), "swiglu_bwd_ld")
    assert np.array_equal(yb[:, :F].reshape(-1), flat["y"])
    assert np.array_equal(d13[:, :F].reshape(-1), flat["da"]) and np.array_equal(d13[:, F:2 * F].reshape(-1), flat["db"])
    for buf, used in ((y13, 2 * F), (d13, 2 * F), (yb, F), (gb, F)):
        assert (np.ascontiguousarray(buf[:, used:]).view(np.uint8) == POISON).all(), "a gap byte was written"
    E.verify_swiglu(case, dict(y=from_bf16_bits(np.ascontiguousarray(yb[:, :F])), da=from_bf16_bits(np.ascontiguousarray(d13[:, :F])),
                               db=from_bf16_bits(np.ascontiguousarray(d13[:, F:2 * F]))), E.Verdict("emu", False))


# ---------------------------------------------------------------- cross entropy
def _ce(logits, target, weight, f32):
    rows, V = logits.shape
    la, tg, w = _in(logits, f32), _i32(target), _in(weight, True)
    nll, cor, dl = _out((rows,), True), _emu.aligned((rows,), np.int32), _out((rows, V), f32)
    cor[...] = -1
    _ok(_fn("softmax_ce", f32)(la.ctypes.data, tg.ctypes.data, w.ctypes.data, nll.ctypes.data, cor.ctypes.data, dl.ctypes.data, rows, V,
                               None), "softmax_ce")
    return np.array(nll), np.array(cor), dl


@pytest.mark.parametrize("name,f32", _ids(E.ce_names))
def test_cross_entropy(name, f32):
    case = E.ce_case(name, f32)
    nll, cor, dl = _ce(case.logits(f32), case.target, case.weight, f32)
    E.verify_ce(case, (nll, cor, _dec(dl, f32)), E.Verdict("emu", f32))


@pytest.mark.parametrize("f32", FLAVOURS)
@pytest.mark.parametrize("poison", E.POISONS, ids=["nan", "+inf", "-inf"])
def test_cross_entropy_row_of_weight_zero_holding_non_finite_logits(poison, f32):
    """the kernel's part of the contract: such a row gets an exact 0 gradient, and no other row changes by a bit
    (the loss selects with where(weight > 0), lwm_amd/llama_ops.py: tests/test_gpu_elem_edges.py)"""
    V = 520
    x, tok, valid = E.ce_public_case(V, 5)
    xp, _, _ = E.ce_public_case(V, 5, poison)
    w = (valid / (valid.sum(-1, keepdims=True) * 2)).reshape(-1)
    x, xp = (t if f32 else round_bf16(t) for t in (x.reshape(-1, V), xp.reshape(-1, V)))
    nll0, cor0, dl0 = _ce(x, tok.reshape(-1), w, f32)
    nll1, cor1, dl1 = _ce(xp, tok.reshape(-1), w, f32)
    live = w > 0
    assert live.sum() == 5 and not np.isfinite(xp[~live]).all()
    assert np.array_equal(dl0.view(np.uint8), dl1.view(np.uint8)) and not dl1[~live].any()
    assert np.array_equal(nll0[live], nll1[live]) and np.array_equal(cor0[live], cor1[live])


# ---------------------------------------------------------------- GEMV family
def _gemv_fused_ld(x, ws, *, norm=None, residual=None, want_ss=False, want_f32=False, pad=0):
    """lwm_gemv_fused_bf16 with ldx / ldy / ldres = row + pad and NaN bits in the gaps -> ([y], ss or None); asserts the gaps"""
    L = _emu.lib()
    rows, K = x.shape
    Ns = [w.shape[1] for w in ws]
    xb = _out((rows, K + pad), False)
    xb[:, :K] = to_bf16_bits(x)
    wbs = [_in(w, False) for w in ws]
    work = _emu.aligned((sum(max(L.lwm_gemv_workspace_bytes(rows, K, N), 16) for N in Ns) // 4,), np.float32)
    work[...] = np.nan
    ys = [_out((rows, N) if want_f32 else (rows, N + pad), want_f32) for N in Ns]
    a = _capi.LwmGemvArgs()
    a.x, a.ldx, a.nmat, a.rows, a.K, a.workspace = xb.ctypes.data, K + pad, len(ws), rows, K, work.ctypes.data
    for i, N in enumerate(Ns):
        a.w[i], a.N[i] = wbs[i].ctypes.data, N
        if want_f32:
            a.y_f32[i] = ys[i].ctypes.data
        else:
            a.y[i], a.ldy[i] = ys[i].ctypes.data, N + pad
    keep = []
    if norm is not None:
        ss, gam, eps = norm
        ssa, gb = _in(ss, True), _in(gam, False)
        keep += [ssa, gb]
        a.norm_weight, a.ss_in, a.ss_n, a.eps = gb.ctypes.data, ssa.ctypes.data, ss.shape[1], eps
    if residual is not None:
        rb = _out((rows, Ns[0] + pad), False)
        rb[:, :Ns[0]] = to_bf16_bits(residual)
        keep.append(rb)
        a.residual[0], a.ldres[0] = rb.ctypes.data, Ns[0] + pad
    sso = None
    if want_ss:
        sso = _out((rows, Ns[0] // 128), True)
        a.ss_out = sso.ctypes.data
    _ok(L.lwm_gemv_fused_bf16(C.byref(a), None), "lwm_gemv_fused_bf16")
    out = []
    for y, N in zip(ys, Ns):
        if not want_f32:
            assert (np.ascontiguousarray(y[:, N:]).view(np.uint8) == POISON).all(), "a gap byte of y was written"
        out.append(np.array(y) if want_f32 else from_bf16_bits(np.ascontiguousarray(y[:, :N])))
    return out, (None if sso is None else np.array(sso))


@pytest.mark.parametrize("rows,K,N", E.GEMV_SHAPES)
def test_gemv(rows, K, N):
    x, w = E.gemv_ops(rows, K, N)
    yb, yf = _emu.gemv(x, w, want_f32=True)
    E.verify_gemv(f"gemv_{rows}x{K}x{N}", yb, yf, x, w, E.Verdict("emu", False))
    assert np.array_equal(_emu.gemv(x, w), yb)


def test_gemv_multi_unequal_widths():
    x = E.gemv_ops(2, 160, 256)[0]
    ws = [E.gemv_ops(2, 160, n, seed=i)[1] for i, n in enumerate((256, 64, 64))]
    for f32 in (True, False):
        got = _emu.gemv_multi(x, ws, want_f32=f32)
        for w, y in zip(ws, got):
            yb, yf = _emu.gemv(x, w, want_f32=True)
            assert np.array_equal(y, yf if f32 else yb)


@pytest.mark.parametrize("d,N", [(160, 384), (4096, 11008)])
def test_gemv_fused(d, N):
    """norm on load against RMSNorm -> gemv; residual against gemv + bf16 add (bit-equal); ss_out sums; every leading
    dimension wider than its row with NaN bits in the gaps"""
    rows = 2
    v = E.Verdict("emu", False)
    g = np.random.default_rng(d + N)
    x, w = E.gemv_ops(rows, d, N)
    gam = round_bf16((g.standard_normal(d) * 3 + 0.5).astype(np.float32))
    res = round_bf16(g.standard_normal((rows, N)).astype(np.float32))
    # the padded call with nothing fused equals the plain one
    (y0,), _ = _gemv_fused_ld(x, [w], pad=PAD)
    assert np.array_equal(y0, _emu.gemv(x, w))
    # residual + partial sums of squares
    (z,), sso = _gemv_fused_ld(x, [w], residual=res, want_ss=True, pad=PAD)
    want = round_bf16(_emu.gemv(x, w) + res)
    assert np.array_equal(z, want)
    assert sso.shape == (rows, N // 128)
    assert np.allclose(sso.sum(1), (want.astype(np.float64) ** 2).sum(1), rtol=1e-5)
    # norm on load: partial sums of squares in 1..64 pieces
    for n_ss in ((1, 5, 32) if d < 1024 else (32,)):
        parts = np.zeros((rows, n_ss), np.float32)
        for i, ch in enumerate(np.array_split(np.arange(d), n_ss)):
            parts[:, i] = (x[:, ch].astype(np.float64) ** 2).sum(1)
        (y1,), _ = _gemv_fused_ld(x, [w], norm=(parts, gam, E.EPS), pad=PAD)
        xn, _ = _emu.rmsnorm_fwd(x, gam, E.EPS)
        ref, mag = E.gemv_ref(xn, w)
        # (rstd from another summation order may move an element of the normalised x by a bf16 ulp: 2^-8 mag at most,
        # plus the rounding of the output)
        v(f"gemv_fused_{d}x{N}.norm_on_load_ss{n_ss}", y1, ref, mag)


# ---------------------------------------------------------------- grid caps and tails of the cast / sum helpers
def test_cast_and_sum_past_the_grid_cap_and_with_a_tail():
    """4096 blocks x 256 threads x 8 elements, three more vectors, and a tail of 5 that thread 0 walks (misc_kernels.h);
    lwm_sum_f32 has no tail loop and refuses an n that is no multiple of 4"""
    L = _emu.lib()
    n = 8 * (4096 * 256 + 3) + 5
    g = np.random.default_rng(3)
    srcs = [_in((g.standard_normal(n) * 10.0 ** s).astype(np.float32), True) for s in (0, -2, 1)]
    dst = _out((n,), False)
    _ok(L.lwm_cast_f32_to_bf16(srcs[0].ctypes.data, dst.ctypes.data, n, None), "cast")
    assert np.array_equal(dst, to_bf16_bits(srcs[0]))
    ptrs = (C.c_void_p * 3)(*[s.ctypes.data for s in srcs])
    dst = _out((n,), False)
    _ok(L.lwm_sum_f32_to_bf16(ptrs, 3, dst.ctypes.data, n, None), "sum")
    ordered = (srcs[0] + srcs[1]) + srcs[2]
    assert np.array_equal(dst, to_bf16_bits(ordered))
    assert L.lwm_sum_f32(ptrs, 3, dst.ctypes.data, n, None) == _capi.LWM_EINVAL
    n4 = 4 * (4096 * 256 + 3)
    d32 = _out((n4,), True)
    _ok(L.lwm_sum_f32(ptrs, 3, d32.ctypes.data, n4, None), "sum_f32")
    assert np.array_equal(d32, ordered[:n4])


# ---------------------------------------------------------------- the verdict fails what it must
def test_references_pass_their_own_verdict():
    for name, _, ref, mag, _ in E.mutants():
        E.check(f"self {name}", ref, ref, mag, 0.0)
        E.check(f"self bf16 {name}", round_bf16(ref.astype(np.float32)), ref, mag, E.BF16_TOL)


@pytest.mark.parametrize("idx", range(6), ids=[m[0] for m in E.mutants()])
def test_mutants_fail_the_verdict(idx):
    """each damaged reference misses the bf16 bound (and with it every tighter f32 / GEMV bound); printed beside it: the
    max-norm figure against the bound the suite held this output to before"""
    name, bad, ref, mag, old_bound = E.mutants()[idx]
    old = E.max_norm(bad, ref)
    print(f"{name}: max-norm {old:.3e} against the old bound {old_bound:.3e}: {'let through' if old <= old_bound else 'caught'}")
    with pytest.raises(E.VerdictError):
        E.check(f"mutant {name}", bad, ref, mag, E.BF16_TOL)
