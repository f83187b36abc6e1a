"""The checks of the 6-bit decode-weight entries (lwm_w6_quantise, lwm_gemv_fused_w6, lwm_gemm_rows_fused_w6), written once
over the buffer backend of tests/_rows_cases.py so that tests/test_emu_w6.py (host emulation) and tests/test_gpu_w6.py
(device buffers) run the same code.  Every buffer sits between guard bands, every output is poison-filled first, and every
comparison is of bits.  TEST INFRASTRUCTURE ONLY."""
import ctypes as C

import numpy as np

from lwm_amd import _capi
from oracle import attention_ref as R
from tests import _rows_cases as RC, _w6_ref as W6

bits = RC.bits


def quantise(B, w, in_place=False):
    """w (K, N) f32 of bf16 values -> (codes u8 (K/4, N/8, 24), scale bytes u8 (K/32, N), rounded bf16 bits u16) through
    lwm_w6_quantise"""
    L = B.lib()
    K, N = w.shape
    src = B.buf(R.to_bf16_bits(w))
    q, s = B.buf(np.full((K // 4, N // 8, W6.SLOT), 0xa5, np.uint8)), B.buf(np.zeros((K // 32, N), np.uint8))
    r = src if in_place else B.buf(RC.poison((K, N), np.uint16))
    _capi.check(L, L.lwm_w6_quantise(src.ptr, q.ptr, s.ptr, r.ptr, K, N, None), "lwm_w6_quantise")
    B.sync()
    assert src.intact() and q.intact() and s.intact() and r.intact(), "a guard band was written"
    if not in_place:
        assert np.array_equal(src.read(), R.to_bf16_bits(w)), "the input was modified"
    return q.read(), s.read(), r.read()


def run(B, x, mats, *, entry, w6, norm=None, residual=None, want_ss=False, want_f32=False):
    """One call of lwm_gemv_fused_* (entry "gemv") or lwm_gemm_rows_fused_* ("rows") over 6-bit packs (w6: mats =
    [(codes, scale bytes)]) or bf16 kernels (mats = [W f32 of bf16 values]) -> dict(y=[bits], ss, work) as _rows_cases.run"""
    L = B.lib()
    rows, K = x.shape
    Ns = [(m[1] if w6 else m).shape[1] for m in mats]
    need = sum(L.lwm_gemv_workspace_bytes(rows, K, N) for N in Ns) // 4
    xb = B.buf(R.to_bf16_bits(x))
    work = B.buf(RC.poison((need + RC.TAIL,), np.float32))
    a = (_capi.LwmGemvW6Args if w6 else _capi.LwmGemvArgs)()
    a.x, a.ldx, a.nmat, a.rows, a.K, a.workspace = xb.ptr, K, len(mats), rows, K, work.ptr
    inputs, ys = [(xb, R.to_bf16_bits(x))], []
    for i, m in enumerate(mats):
        if w6:
            q, s = B.buf(m[0]), B.buf(m[1])
            a.w[i], a.w_scale[i] = q.ptr, s.ptr
            inputs += [(q, m[0]), (s, m[1])]
        else:
            wb = B.buf(R.to_bf16_bits(m))
            a.w[i] = wb.ptr
            inputs.append((wb, R.to_bf16_bits(m)))
        a.N[i] = Ns[i]
        y = B.buf(RC.poison((rows, Ns[i]), np.float32 if want_f32 else np.uint16))
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
        sso = B.buf(RC.poison((rows, Ns[0] // 128), np.float32))
        a.ss_out = sso.ptr
    name = ("lwm_gemm_rows_fused_" if entry == "rows" else "lwm_gemv_fused_") + ("w6" if w6 else "bf16")
    _capi.check(L, getattr(L, name)(C.byref(a), None), name)
    B.sync()
    assert all(b.intact() for b, _ in inputs) and all(y.intact() for y in ys) and work.intact(), "a guard band was written"
    assert sso is None or sso.intact()
    for b, was in inputs:
        assert np.array_equal(b.read().view(np.uint8), np.ascontiguousarray(was).view(np.uint8)), "an input was modified"
    wk = work.read()
    assert RC.is_poison(wk[need:]), "the workspace was written past its documented size"
    assert not np.isnan(wk[:need]).any(), "a partial was left unwritten"
    return dict(y=[y.read() for y in ys], ss=None if sso is None else sso.read(), work=wk[:need])


_PACKS = {}


def packs_of(rows, K, Ns):
    """-> x, the reference's packs, their exact values as f32: computed once, shared, never modified"""
    key = (rows, K, tuple(Ns))
    if key not in _PACKS:
        x, ws = W6.gemv_case(rows, K, Ns)
        packs = [W6.quantise(w) for w in ws]
        deq = [W6.dequant(q, e, w.shape).astype(np.float32) for (q, e), w in zip(packs, ws)]
        for d in deq:                                   # the test's domain: every rounded weight IS a bf16 value
            assert np.array_equal(R.round_bf16(d), d)
        for _, e in packs:
            assert e.min() >= 127 - 40 and e.max() <= 127 + 40
        _PACKS[key] = (x, packs, deq)
    return _PACKS[key]


def equal(got, ref):
    """outputs, ss_out and every workspace partial, bit for bit"""
    return np.array_equal(bits(got["work"]), bits(ref["work"])) and RC.same(got, ref)


# ---------------------------------------------------------------- the checks
def check_quantiser(B, w):
    q_ref, e_ref = W6.quantise(w)
    r_ref = R.to_bf16_bits(W6.rounded(q_ref, e_ref, w.shape))
    for in_place in (False, True):
        q, e, r = quantise(B, w, in_place)
        assert np.array_equal(e, e_ref)
        assert np.array_equal(q, q_ref)
        assert np.array_equal(r, r_ref)                 # bitwise: the sign of zero too
    _, _, r2 = quantise(B, R.from_bf16_bits(r))         # the rounded weights are a fixed point
    assert np.array_equal(r2, r)


def check_gemv(B, rows, K, Ns):
    x, packs, deq = packs_of(rows, K, Ns)
    for f32 in (False, True):
        got = run(B, x, packs, entry="gemv", w6=True, want_f32=f32)
        ref = run(B, x, deq, entry="gemv", w6=False, want_f32=f32)
        assert equal(got, ref), f32
        assert all(np.any(y) for y in got["y"])


def check_gemv_norm(B, rows, K, N):
    x, packs, deq = packs_of(rows, K, (N, 16))
    plain = run(B, x, packs, entry="gemv", w6=True, want_f32=True)
    for n_ss in (1, 5, 64):
        norm = RC.norm_case(x, n_ss)
        for f32 in (False, True):
            got = run(B, x, packs, entry="gemv", w6=True, norm=norm, want_f32=f32)
            assert equal(got, run(B, x, deq, entry="gemv", w6=False, norm=norm, want_f32=f32)), (n_ss, f32)
        assert not np.array_equal(plain["y"][0], got["y"][0])                  # the norm did something


def residual_for(rows, N):
    return R.round_bf16(np.random.default_rng(6).standard_normal((rows, N)).astype(np.float32) * 4.0)


def check_gemv_residual_ss(B, rows, K, N):
    x, packs, deq = packs_of(rows, K, (N,))
    res = residual_for(rows, N)
    got = run(B, x, packs, entry="gemv", w6=True, residual=res, want_ss=True)
    assert equal(got, run(B, x, deq, entry="gemv", w6=False, residual=res, want_ss=True))
    assert not np.array_equal(run(B, x, packs, entry="gemv", w6=True)["y"][0], got["y"][0])


def check_through_the_quantiser(B):
    """the kernels together: quantise with the kernel, stream its codes through both entries, compare with the bf16 entries on
    ITS rounded weights; and the rounding moved no weight by amax / 15 or more"""
    x, (w,) = W6.gemv_case(2, 416, (1040,))
    q, e, r = quantise(B, w)
    rw = R.from_bf16_bits(r)
    for entry in ("gemv", "rows"):
        assert equal(run(B, x, [(q, e)], entry=entry, w6=True, want_f32=True), run(B, x, [rw], entry=entry, w6=False, want_f32=True)), entry
    amax = np.repeat(np.abs(w.astype(np.float64)).reshape(-1, 32, w.shape[1]).max(1), 32, axis=0)
    assert (np.abs(rw.astype(np.float64) - w) < amax / 15 + 1e-300).all()


ROWS_SHAPES = [(32, (16,)), (160, (264,)), (416, (16, 264))]     # one partial; a short last group; N one past the 256-column tile
ROWS_ROWS = (1, 5, 16, 17, 32)


def check_rows(B, rows, K, Ns):
    x, packs, deq = packs_of(rows, K, Ns)
    variants = [dict(), dict(want_f32=True), dict(norm=RC.norm_case(x, 32))]
    if len(Ns) == 1:
        variants.append(dict(residual=residual_for(rows, Ns[0])))
    for kw in variants:
        got = run(B, x, packs, entry="rows", w6=True, **kw)
        assert equal(got, run(B, x, deq, entry="rows", w6=False, **kw)), list(kw)
        assert any(np.any(y) for y in got["y"])


def check_rows_residual_ss(B, rows):
    x, packs, deq = packs_of(rows, 416, (384,))
    res = residual_for(rows, 384)
    kw = dict(residual=res, want_ss=True, norm=RC.norm_case(x, 5))
    assert equal(run(B, x, packs, entry="rows", w6=True, **kw), run(B, x, deq, entry="rows", w6=False, **kw))


def check_row_independence(B):
    """a row's bits are the same in a batch of 5 and in a batch of 32"""
    x32, packs, _ = packs_of(32, 416, (16, 264))
    big = run(B, x32, packs, entry="rows", w6=True, want_f32=True)
    rng = np.random.default_rng(3)
    for r, slot in ((0, 3), (16, 1), (31, 0)):
        x5 = R.round_bf16(rng.standard_normal((5, 416)).astype(np.float32) * 3.0)
        x5[slot] = x32[r]
        small = run(B, x5, packs, entry="rows", w6=True, want_f32=True)
        for y5, y32 in zip(small["y"], big["y"]):
            assert np.array_equal(bits(y5)[slot], bits(y32)[r]), (r, slot)


# ---------------------------------------------------------------- refusals: the tables of _rows_cases under the new tags
def valid_args(B, rows, K=64, N=128):
    bufs = dict(x=B.buf(np.zeros((rows, K), np.uint16)), w=B.buf(np.zeros((K // 4, N // 8, W6.SLOT), np.uint8)),
                s=B.buf(np.full((K // 32, N), 127, np.uint8)), y=B.buf(RC.poison((rows, N), np.uint16)),
                yf=B.buf(RC.poison((rows, N), np.float32)), work=B.buf(RC.poison((2 * rows * N + RC.TAIL,), np.float32)),
                res=B.buf(np.zeros((rows, N), np.uint16)), gam=B.buf(np.zeros((K,), np.uint16)),
                ss=B.buf(np.ones((rows, 4), np.float32)), sso=B.buf(RC.poison((rows, 1), np.float32)))
    a = _capi.LwmGemvW6Args()
    a.x, a.ldx, a.nmat, a.rows, a.K = bufs["x"].ptr, K, 1, rows, K
    a.w[0], a.w_scale[0], a.y[0], a.ldy[0], a.N[0], a.y_f32[0] = bufs["w"].ptr, bufs["s"].ptr, bufs["y"].ptr, N, N, bufs["yf"].ptr
    a.workspace = bufs["work"].ptr
    return a, bufs


def entry_fn(L, entry):
    return (L.lwm_gemm_rows_fused_w6, b"gemm_rows_w6: ") if entry == "rows" else (L.lwm_gemv_fused_w6, b"gemv_w6: ")


def refusal_names(entry):
    return list(RC.REFUSALS if entry == "rows" else RC.GEMV_REFUSALS) + list(RC.W8_REFUSALS)


def check_refusal(B, entry, name):
    """same edit, same code as the w8 entry gives, the text under the new tag (its wording is the shared front end's), and
    nothing written"""
    L = B.lib()
    code, edit = (RC.REFUSALS | RC.GEMV_REFUSALS | RC.W8_REFUSALS)[name]
    a, bufs = valid_args(B, RC.ENTRY_ROWS[entry])
    edit(a, bufs)
    fn, tag = entry_fn(L, entry)
    assert fn(C.byref(a), None) == code
    B.sync()
    text = L.lwm_last_error()
    assert text and text.startswith(tag)
    a8, bufs8 = RC.valid_args(B, True, rows=RC.ENTRY_ROWS[entry])
    edit(a8, bufs8)
    fn8, tag8 = RC.entry_fn(L, entry, True)
    assert fn8(C.byref(a8), None) == code and L.lwm_last_error()[len(tag8):] == text[len(tag):]
    assert RC.untouched(bufs)


def check_accepted(B, entry):
    """... so the tables are not vacuous; the GEMV takes no rows as a call that does nothing; a null struct is refused"""
    L = B.lib()
    rows = RC.ENTRY_ROWS[entry]
    a, bufs = valid_args(B, rows)
    fn, tag = entry_fn(L, entry)
    assert fn(C.byref(a), None) == _capi.LWM_OK, L.lwm_last_error()
    B.sync()
    assert (bufs["y"].read() == 0).all() and (bufs["yf"].read() == 0).all() and RC.is_poison(bufs["work"].read()[rows * 128:])
    assert all(b.intact() for b in bufs.values())
    if entry == "gemv":
        a, bufs = valid_args(B, rows)
        a.rows = 0
        assert fn(C.byref(a), None) == _capi.LWM_OK
        B.sync()
        assert RC.untouched(bufs)
    assert fn(None, None) == RC.EINVAL and L.lwm_last_error().startswith(tag)


def check_quantiser_refusals(B):
    L = B.lib()
    K, N = 64, 32
    w, r = B.buf(np.zeros((K, N), np.uint16)), B.buf(RC.poison((K, N), np.uint16))
    q, s = B.buf(np.full((K // 4, N // 8, W6.SLOT), 0xa5, np.uint8)), B.buf(np.full((K // 32, N), 0xa5, np.uint8))

    def call(wp=None, qp=None, sp=None, rp=None, K=K, N=N):
        pick = lambda v, d: d.ptr if v is None else v
        rc = L.lwm_w6_quantise(pick(wp, w), pick(qp, q), pick(sp, s), pick(rp, r), K, N, None)
        B.sync()
        return rc, bool((q.read() == 0xa5).all() and RC.is_poison(r.read()) and (s.read() == 0xa5).all())

    for kw, code in ((dict(K=48), RC.EUNSUP), (dict(K=12320), RC.EUNSUP), (dict(N=20), RC.EUNSUP), (dict(N=4), RC.EUNSUP),
                     (dict(K=0), RC.EINVAL), (dict(N=-16), RC.EINVAL), (dict(wp=0), RC.EINVAL), (dict(qp=0), RC.EINVAL),
                     (dict(sp=0), RC.EINVAL), (dict(rp=0), RC.EINVAL), (dict(wp=w.ptr + 2), RC.EINVAL), (dict(qp=q.ptr + 8), RC.EINVAL),
                     (dict(sp=s.ptr + 8), RC.EINVAL), (dict(rp=r.ptr + 8), RC.EINVAL)):
        assert call(**kw) == (code, True), kw
        assert L.lwm_last_error().startswith(b"w6_quantise: ")
    assert call() == (_capi.LWM_OK, False)
    assert all(b.intact() for b in (w, r, q, s))
