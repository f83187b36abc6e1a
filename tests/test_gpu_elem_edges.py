"""The kernels either side of attention at edge shapes and values, on the device through the Python surface
(lwm_amd.llama_ops, lwm_amd.ops): the cases, the float64 references with their magnitudes and the per-element verdict are
tests/_elem_cases.py's (the host emulator runs the same ones in tests/test_emu_elem_edges.py).  Every figure a run
measures is printed (pytest -s)."""
import numpy as np
import pytest

from oracle import llama_ops_ref as R
from oracle.attention_ref import round_bf16
from tests import _elem_cases as E

pytestmark = pytest.mark.gpu

FLAVOURS = [pytest.param(False, id="bf16"), pytest.param(True, id="f32")]
PAD = 8


def _sfx(f32):
    return "f32" if f32 else "bf16"


def _ids(names):
    return [pytest.param(n, f32, id=f"{n if isinstance(n, str) else 'x'.join(map(str, n[:2]))}-{_sfx(f32)}")
            for f32 in (False, True) for n in names(f32, device=True)]


def _dev(a, f32=True):
    """numpy -> device tensor; float arrays become bf16 unless f32 (their values are bf16 values already)"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if f32 or t.dtype != torch.float32 else t.to(torch.bfloat16)


def _np(t):
    return t.detach().float().cpu().numpy()


def _nan_buffer(shape, dtype):
    import torch
    buf = torch.empty(shape, dtype=dtype, device="cuda")
    buf.view(torch.uint8).fill_(0xFF)
    return buf


def _gaps_intact(buf, used):
    import torch
    return bool((buf[..., used:].contiguous().view(torch.uint8) == 0xFF).all())


# ---------------------------------------------------------------- RoPE
@pytest.mark.parametrize("f32", FLAVOURS)
@pytest.mark.parametrize("case", E.rope_cases(), ids=repr)
def test_rope(case, f32):
    """apply_rotary_emb forward and (autograd) conjugate against fp64, per element, xq with H heads and xk a two-head view;
    then the operands as views into a wider buffer whose gaps hold NaN: the contiguous call's bits, the gaps untouched"""
    import torch
    from lwm_amd import llama_ops as LO
    v = E.Verdict("gpu", f32)
    x = case.x(f32)
    xd = _dev(x, f32).requires_grad_(True)
    tab = _dev(case.table)
    pos = _dev(case.pos_arg)
    yq, yk = LO.apply_rotary_emb(xd, xd[:, :, :2], tab, pos)
    E.verify_rope(case, _np(yq), False, v)
    assert torch.equal(yk, yq[:, :, :2])
    (gx,) = torch.autograd.grad(yq, xd, xd.detach())                   # the backward of x -> rope(x) at g = x: the conjugate rotation of x
    E.verify_rope(case, _np(gx), True, v)
    B, S, H, D = x.shape
    buf = _nan_buffer((B, S, H, D + PAD), xd.dtype)
    buf[..., :D] = xd.detach()
    sq, sk = LO.apply_rotary_emb(buf[..., :D], buf[:, :, 1:, :D], tab, pos)
    assert torch.equal(sq, yq) and torch.equal(sk, yq[:, :, 1:])
    assert _gaps_intact(buf, D) and torch.equal(buf[..., :D], xd.detach())


@pytest.mark.parametrize("case", E.rope_cases()[:3], ids=repr)
def test_qkv_rope_rotates_in_place_what_apply_rotary_emb_rotates(case):
    """qkv_rope with wq = I, wk = 2 I, wv = -I (exact in any GEMM): xq, xk must be the bits of apply_rotary_emb on x and
    2 x, xv = -x; the backward's dx = conj(gq) + 2 conj(gk) - gv against fp64, per element"""
    import torch
    from lwm_amd import llama_ops as LO
    v = E.Verdict("gpu", False)
    x = case.x(False)
    B, S, H, D = x.shape
    d = H * D
    xd = _dev(x, False).reshape(B, S, d).requires_grad_(True)
    eye = torch.eye(d, dtype=torch.bfloat16, device="cuda")
    tab, pos = _dev(case.table), _dev(case.pos_arg)
    q, k, xv = LO.qkv_rope(xd, eye, 2 * eye, -eye, tab, pos, H)
    x4 = xd.detach().reshape(B, S, H, D)
    rq, rk = LO.apply_rotary_emb(x4, 2 * x4, tab, pos)
    assert torch.equal(q, rq) and torch.equal(k, rk) and torch.equal(xv, -x4)
    E.verify_rope(case, _np(q), False, v)
    g = np.random.default_rng(5)
    gq, gk, gv = (round_bf16(g.standard_normal(x.shape).astype(np.float32)) for _ in range(3))
    (dx,) = torch.autograd.grad([q, k, xv], xd, [_dev(t, False) for t in (gq, gk, gv)])
    cq, mq = E.rope_ref(gq, case.table, case.pos, conj=True)
    ck, mk = E.rope_ref(gk, case.table, case.pos, conj=True)
    E.check(f"gpu bf16 {case.name}.qkv_rope_dx", _np(dx).reshape(x.shape), cq + 2 * ck - gv, mq + 2 * mk + np.abs(gv), E.BF16_TOL)


# ---------------------------------------------------------------- RMSNorm
@pytest.mark.parametrize("shape,f32", _ids(E.rms_shapes))
def test_rmsnorm(shape, f32):
    """RMSNorm forward, its backward through autograd (dx and the weight's gradient), and -- bf16 -- the same through
    rmsnorm_residual with the residual branch's gradient folded into the kernel"""
    import torch
    from lwm_amd import llama_ops as LO
    case = E.rms_case(*shape)
    x, w, g, res = case.ops(f32)
    dt = torch.float32 if f32 else torch.bfloat16
    norm = LO.RMSNorm(case.C, E.EPS, dtype=dt).cuda()
    with torch.no_grad():
        norm.kernel.copy_(_dev(w))
    xd = _dev(x, f32).requires_grad_(True)
    y = norm(xd)
    got = dict(y=_np(y), rstd=_np(y.grad_fn.saved_tensors[2]))      # (x, weight, rstd) as the forward saved them
    if case.fwd_only:
        E.verify_rms(case, got, E.Verdict("gpu", f32))
        return
    dx, dw = torch.autograd.grad(y, [xd, norm.kernel], _dev(g, f32))
    assert dw.dtype == norm.kernel.dtype
    got.update(dx=_np(dx), dw=_np(dw))
    if not f32:
        y2, xp = LO.rmsnorm_residual(norm, xd)
        assert torch.equal(y2, y)
        dx2, dw2 = torch.autograd.grad([y2, xp], [xd, norm.kernel], [_dev(g, f32), _dev(res, f32)])
        got.update(dx_res=_np(dx2), dw_res=_np(dw2))
    E.verify_rms(case, got, E.Verdict("gpu", f32))


# ---------------------------------------------------------------- SwiGLU
def _swiglu(case, f32):
    import torch
    from lwm_amd import llama_ops as LO
    a, b, g = (_dev(t, f32) for t in case.ops(f32))
    a.requires_grad_(True)
    b.requires_grad_(True)
    y = LO.swiglu(a, b)
    da, db = torch.autograd.grad(y, [a, b], g)
    return dict(y=y.detach(), da=da, db=db)


@pytest.mark.parametrize("f32", FLAVOURS)
@pytest.mark.parametrize("case", E.swiglu_cases(), ids=repr)
def test_swiglu(case, f32):
    E.verify_swiglu(case, {n: _np(t) for n, t in _swiglu(case, f32).items()}, E.Verdict("gpu", f32))


@pytest.mark.parametrize("case", E.swiglu_halves_cases(), ids=repr)
def test_swiglu_halves(case):
    """gate | up as the halves of a (rows, 2F) view into a wider buffer with NaN in the gaps: bit for bit the flat form"""
    import torch
    from lwm_amd import llama_ops as LO
    a, b, g = (_dev(t, False) for t in case.ops(False))
    rows, F = a.shape
    flat = _swiglu(case, False)
    buf = _nan_buffer((rows, 2 * F + PAD), torch.bfloat16)
    buf[:, :F], buf[:, F:2 * F] = a, b
    y13 = buf[:, :2 * F].requires_grad_(True)
    y = LO.swiglu_halves(y13)
    (d13,) = torch.autograd.grad(y, y13, g)
    assert torch.equal(y, flat["y"]) and torch.equal(d13[:, :F], flat["da"]) and torch.equal(d13[:, F:], flat["db"])
    assert _gaps_intact(buf, 2 * F)
    E.verify_swiglu(case, dict(y=_np(y), da=_np(d13[:, :F]), db=_np(d13[:, F:])), E.Verdict("gpu", False))


# ---------------------------------------------------------------- cross entropy
@pytest.mark.parametrize("name,f32", _ids(E.ce_names))
def test_cross_entropy_kernel(name, f32):
    """the fused kernel with explicit row weights (what the public entry points hand it): nll, correct, dlogits"""
    from lwm_amd import llama_ops as LO
    case = E.ce_case(name, f32)
    nll, cor, dl = LO._softmax_ce(_dev(case.logits(f32), f32), _dev(case.target), _dev(case.weight), True)
    E.verify_ce(case, (_np(nll), _np(cor), _np(dl)), E.Verdict("gpu", f32))


def _public_ref(x, tok, valid):
    """the oracle's loss and accuracy; dlogits with its magnitude from the reference of the kernel cases"""
    with np.errstate(all="ignore"):
        loss, acc, _ = R.cross_entropy_loss_and_accuracy(x, tok, valid)
    B, S, V = x.shape
    w = (np.where(valid > 0, 1.0, 0.0) / (np.maximum(valid.sum(-1, keepdims=True), 1e-10) * B)).reshape(-1)
    return loss, acc, w


def _check_public(name, v, loss, acc, ref_loss, ref_acc):
    assert np.isfinite(ref_loss) and np.isfinite(ref_acc)
    E.check_rel(f"{v.tag} {name}.loss", np.array([float(loss)]), np.array([ref_loss]), 1e-6, floor=1.0)
    assert abs(float(acc) - ref_acc) <= 1e-6, f"{name}: accuracy {float(acc)} against {ref_acc}"


@pytest.mark.parametrize("f32", FLAVOURS)
@pytest.mark.parametrize("V", [8, 520, 8448, 32768])
def test_cross_entropy_loss_and_accuracy(V, f32):
    """the public entry point: loss, accuracy, and the gradient per element; then the one valid == 0 row filled with NaN /
    +Inf / -Inf: loss and accuracy stay the oracle's finite values, that row's gradient is 0, no other row's changes a bit"""
    import torch
    from lwm_amd import llama_ops as LO
    v = E.Verdict("gpu", f32)
    x, tok, valid = E.ce_public_case(V, 5)
    x = E._prep(f32, x)[0]
    ref_loss, ref_acc, w = _public_ref(x, tok, valid)

    def run(xx):
        ld = _dev(xx, f32).requires_grad_(True)
        loss, acc = LO.cross_entropy_loss_and_accuracy(ld, _dev(tok), _dev(valid), sp_sharded=False)
        (dl,) = torch.autograd.grad(loss, ld)
        return loss, acc, dl

    loss, acc, dl = run(x)
    name = f"ce_public_V{V}"
    _check_public(name, v, loss, acc, ref_loss, ref_acc)
    ref = E.ce_ref(x.reshape(-1, V), tok.reshape(-1), w)
    v(f"{name}.dlogits", _np(dl).reshape(-1, V), *ref["dl"], np32=E.ce_np32(x.reshape(-1, V), tok.reshape(-1), w) if f32 else None)
    for poison in E.POISONS:
        xp = E._prep(f32, E.ce_public_case(V, 5, poison)[0])[0]
        assert not np.isfinite(xp[0, 2]).all() and np.array_equal(xp[valid > 0], x[valid > 0])
        assert _public_ref(xp, tok, valid)[:2] == (ref_loss, ref_acc)
        loss_p, acc_p, dl_p = run(xp)
        _check_public(f"{name}_poison{poison}", v, loss_p, acc_p, ref_loss, ref_acc)
        assert torch.equal(loss_p, loss) and torch.equal(acc_p, acc)
        assert torch.equal(dl_p, dl) and not dl_p[0, 2].any()


@pytest.mark.parametrize("f32", FLAVOURS)
def test_chunked_lm_head_loss(f32):
    """loss and accuracy against the oracle on the logits the head GEMM produced, dh per element; then the hidden state of
    the valid == 0 row filled with NaN / Inf: finite, equal loss and accuracy, that row's dh 0, every other row's dh
    unchanged to the bit.  (The head's weight gradient is the wgrad GEMM's, tested elsewhere; with a non-finite hidden row
    h^T dlogits is NaN * 0 inside the GEMM and is not pinned here.)"""
    import torch
    from lwm_amd import llama_ops as LO
    v = E.Verdict("gpu", f32)
    V, Dm = 520, 64
    g = np.random.default_rng(8)
    # small integers and eighths: every product and every partial sum of the head GEMM is exact in f32, so the logits do not
    # depend on the order in which a library kernel adds them
    h = g.integers(-3, 4, (2, 3, Dm)).astype(np.float32)
    k = (g.integers(-4, 5, (Dm, V)) / 8).astype(np.float32)
    _, tok, valid = E.ce_public_case(V, 5)
    kd = _dev(k, f32)

    def run(hh):
        hd = _dev(hh, f32).requires_grad_(True)
        loss, acc = LO.chunked_lm_head_loss(hd, kd, _dev(tok), _dev(valid), chunk=2, sp_sharded=False)
        (dh,) = torch.autograd.grad(loss, hd)
        return loss, acc, dh

    loss, acc, dh = run(h)
    logits = E._prep(f32, (h.reshape(-1, Dm).astype(np.float64) @ k.astype(np.float64)).astype(np.float32))[0].reshape(2, 3, V)
    assert np.array_equal(_np(_dev(h, f32).reshape(-1, Dm) @ kd).reshape(2, 3, V), logits)
    ref_loss, ref_acc, w = _public_ref(logits, tok, valid)
    _check_public("chunked_head", v, loss, acc, ref_loss, ref_acc)
    dl, dl_mag = E.ce_ref(logits.reshape(-1, V), tok.reshape(-1), w)["dl"]
    k64 = k.astype(np.float64)
    np32 = (E.ce_np32(logits.reshape(-1, V), tok.reshape(-1), w) @ k.T).astype(np.float32) if f32 else None
    v("chunked_head.dh", _np(dh).reshape(-1, Dm), dl @ k64.T, dl_mag @ np.abs(k64).T, np32=np32)
    for poison in E.POISONS:
        hp = h.copy()
        hp[0, 2, ::3] = poison
        loss_p, acc_p, dh_p = run(hp)
        assert torch.equal(loss_p, loss) and torch.equal(acc_p, acc)
        assert torch.equal(dh_p, dh) and not dh_p[0, 2].any()


@pytest.mark.parametrize("f32", FLAVOURS)
def test_vision_text_loss_gradients_and_accuracies(f32):
    """V = 8448 as tests/test_gpu_llama_ops.py, but both accuracies and the gradients of both logit tensors, per element;
    and a row masked out of both losses holding NaN / Inf in both tensors"""
    import torch
    from lwm_amd import llama_ops as LO
    v = E.Verdict("gpu", f32)
    V = 8448
    xv, tok, lm = E.ce_public_case(V, 21)
    xt = E.ce_public_case(V, 22)[0]
    xv, xt = E._prep(f32, xv, xt)
    tvm = np.array([[1, 0, 1], [0, 1, 0]], np.float32)
    tok[0, 1] = int(xt[0, 1].argmax())                        # one correct text prediction (vision has one at [0, 0])
    tv, tt = np.where(tvm > 0, tok, 0), np.where(tvm > 0, 0, tok)
    mv, mt = lm * tvm, lm * (1 - tvm)
    (lv, av, wv), (lt, at, wt) = _public_ref(xv, tv, mv), _public_ref(xt, tt, mt)
    assert av > 0 and at > 0

    def run(a, b):
        a, b = _dev(a, f32).requires_grad_(True), _dev(b, f32).requires_grad_(True)
        loss, aux = LO.vision_text_loss(a, b, _dev(tok), _dev(lm), _dev(tvm))
        return (loss, aux) + torch.autograd.grad(loss, [a, b])

    loss, aux, gv, gt = run(xv, xt)
    _check_public("vision_text.vision", v, aux["vision_loss"], aux["vision_acc"], lv, av)
    _check_public("vision_text.text", v, aux["text_loss"], aux["text_acc"], lt, at)
    E.check_rel(f"{v.tag} vision_text.loss", np.array([float(loss)]), np.array([0.5 * (lv + lt)]), 1e-6, floor=1.0)
    for n, got, x, t, w in (("vision", gv, xv, tv, wv), ("text", gt, xt, tt, wt)):
        x2, w2 = x.reshape(-1, V), 0.5 * w
        v(f"vision_text.d{n}_logits", _np(got).reshape(-1, V), *E.ce_ref(x2, t.reshape(-1), w2)["dl"],
          np32=E.ce_np32(x2, t.reshape(-1), w2) if f32 else None)
    for poison in E.POISONS:
        pv, pt = xv.copy(), xt.copy()
        pv[0, 2, ::3] = poison
        pt[0, 2, 1::3] = poison
        loss_p, aux_p, gv_p, gt_p = run(pv, pt)
        assert torch.equal(loss_p, loss) and all(torch.equal(aux_p[n], aux[n]) for n in aux)
        assert torch.equal(gv_p, gv) and torch.equal(gt_p, gt) and not gv_p[0, 2].any() and not gt_p[0, 2].any()


# ---------------------------------------------------------------- GEMV family
@pytest.mark.parametrize("rows,K,N", E.GEMV_SHAPES)
def test_gemv_and_dense_routing(rows, K, N):
    import torch
    from lwm_amd import llama_ops as LO
    x, w = E.gemv_ops(rows, K, N)
    xd, wd = _dev(x, False), _dev(w, False)
    yb, yf = LO.gemv(xd, wd), LO.gemv(xd, wd, torch.float32)
    E.verify_gemv(f"gemv_{rows}x{K}x{N}", _np(yb), _np(yf), x, w, E.Verdict("gpu", False))
    # `dense` streams these through the GEMV as before (at most four rows, no autograd)
    with torch.no_grad():
        assert LO._decode_rows(xd, (wd,)) == rows
        assert torch.equal(LO.dense(xd, wd), yb) and torch.equal(LO.dense(xd.reshape(rows, 1, K), wd).reshape(rows, N), yb)
        assert torch.equal(LO.dense(xd, wd, torch.float32), yf)


def test_gemv_multi_unequal_widths():
    import torch
    from lwm_amd import llama_ops as LO
    x = _dev(E.gemv_ops(2, 160, 256)[0], False)
    ws = [_dev(E.gemv_ops(2, 160, n, seed=i)[1], False) for i, n in enumerate((256, 64, 64))]
    for dt in (torch.bfloat16, torch.float32):
        for w, y in zip(ws, LO.gemv_multi(x, ws, dt)):
            assert torch.equal(y, LO.gemv(x, w, dt))


@pytest.mark.parametrize("d,N", [(160, 384), (4096, 11008)])
def test_gemv_fused(d, N):
    """norm on load against RMSNorm -> gemv; residual against gemv + bf16 add (bit-equal); ss_out sums; x and the
    residual rows of wider buffers with NaN in the gaps (the Python surface keeps ldy = N)"""
    import torch
    from lwm_amd import llama_ops as LO
    rows = 2
    v = E.Verdict("gpu", False)
    g = np.random.default_rng(d + N)
    x, w = E.gemv_ops(rows, d, N)
    gam = round_bf16((g.standard_normal(d) * 3 + 0.5).astype(np.float32))
    res = round_bf16(g.standard_normal((rows, N)).astype(np.float32))
    xbuf, rbuf = _nan_buffer((rows, d + PAD), torch.bfloat16), _nan_buffer((rows, N + PAD), torch.bfloat16)
    xbuf[:, :d], rbuf[:, :N] = _dev(x, False), _dev(res, False)
    xd, rd, wd = xbuf[:, :d], rbuf[:, :N], _dev(w, False)
    plain = LO.gemv(xd.contiguous(), wd)
    assert torch.equal(LO.gemv_fused(xd, [wd])[0], plain) and torch.equal(LO.gemv(xd, wd), plain)
    (z,), sso = LO.gemv_fused(xd, [wd], residual=rd, want_ss=True)
    assert torch.equal(z, plain + rd)
    assert tuple(sso.shape) == (rows, N // 128)
    assert np.allclose(_np(sso).astype(np.float64).sum(1), (_np(z).astype(np.float64) ** 2).sum(1), rtol=1e-5)
    norm = LO.RMSNorm(d, E.EPS).cuda()
    with torch.no_grad():
        norm.kernel.copy_(_dev(gam))
        xn = norm(xd.contiguous())
    ref, mag = E.gemv_ref(_np(xn), w)
    for n_ss in (1, 5, 32):
        parts = np.zeros((rows, n_ss), np.float32)
        for i, ch in enumerate(np.array_split(np.arange(d), n_ss)):
            parts[:, i] = (x[:, ch].astype(np.float64) ** 2).sum(1)
        (y1,) = LO.gemv_fused(xd, [wd], norm=(_dev(parts), _dev(gam, False), E.EPS))
        v(f"gemv_fused_{d}x{N}.norm_on_load_ss{n_ss}", _np(y1), ref, mag)
    assert _gaps_intact(xbuf, d) and _gaps_intact(rbuf, N)


# ---------------------------------------------------------------- grid caps: one large call = the same work in calls below the cap
CAP_VECTORS = 65536 * 256


@pytest.mark.parametrize("f32", FLAVOURS)
def test_swiglu_past_the_grid_cap(f32):
    import torch
    from lwm_amd import llama_ops as LO
    vw = 4 if f32 else 8
    n = vw * (CAP_VECTORS + 773)
    dt = torch.float32 if f32 else torch.bfloat16
    gen = torch.Generator(device="cuda").manual_seed(1)
    a, b, g = (torch.randn(n, device="cuda", generator=gen, dtype=torch.float32).mul_(2).to(dt) for _ in range(3))
    half = vw * (CAP_VECTORS // 2)

    def run(a_, b_, g_):
        a_, b_ = a_.clone().requires_grad_(True), b_.clone().requires_grad_(True)
        y = LO.swiglu(a_, b_)
        return (y.detach(),) + torch.autograd.grad(y, [a_, b_], g_)

    whole = run(a, b, g)
    lo, hi = run(a[:half], b[:half], g[:half]), run(a[half:], b[half:], g[half:])
    for t, l, h in zip(whole, lo, hi):
        assert torch.equal(t[:half], l) and torch.equal(t[half:], h)


@pytest.mark.parametrize("f32", FLAVOURS)
def test_rope_past_the_grid_cap(f32):
    import torch
    from lwm_amd import llama_ops as LO
    D, H, B = 128, 128, 1
    vec = D // (4 if f32 else 8)
    S = (CAP_VECTORS + 4096) // (H * vec) + 1
    assert B * S * H * vec > CAP_VECTORS
    dt = torch.float32 if f32 else torch.bfloat16
    gen = torch.Generator(device="cuda").manual_seed(2)
    x = torch.randn(B, S, H, D, device="cuda", generator=gen, dtype=torch.float32).to(dt)
    tab = _dev(E.rope_table(D, 4096, 1e4))
    pos = torch.randint(0, 4096, (B, S), device="cuda", generator=gen, dtype=torch.int32)
    whole, _ = LO.apply_rotary_emb(x, x[:, :, :1], tab, pos)
    cut = S // 2
    lo, _ = LO.apply_rotary_emb(x[:, :cut], x[:, :cut, :1], tab, pos[:, :cut])
    hi, _ = LO.apply_rotary_emb(x[:, cut:], x[:, cut:, :1], tab, pos[:, cut:])
    assert torch.equal(whole[:, :cut], lo) and torch.equal(whole[:, cut:], hi)


def test_cast_and_sum_past_the_grid_cap_and_with_a_tail():
    """4096 blocks x 256 threads x 8 elements, three more vectors, and a tail of 5 that one thread walks (misc_kernels.h);
    lwm_sum_f32 has no tail loop and refuses an n that is no multiple of 4"""
    import torch
    from lwm_amd import ops
    n = 8 * (4096 * 256 + 3) + 5
    gen = torch.Generator(device="cuda").manual_seed(3)
    srcs = [torch.randn(n, device="cuda", generator=gen) * 10.0 ** s for s in (0, -2, 1)]
    assert torch.equal(ops.cast_f32_to_bf16(srcs[0]), srcs[0].to(torch.bfloat16))
    ordered = (srcs[0] + srcs[1]) + srcs[2]
    assert torch.equal(ops.sum_f32_to_bf16(srcs), ordered.to(torch.bfloat16))
    from lwm_amd import _capi
    with pytest.raises(_capi.LwmError):
        ops.sum_f32_to_bf16(srcs, dst=torch.empty(n, device="cuda"))
    n4 = 4 * (4096 * 256 + 3)
    s4 = [s[:n4].contiguous() for s in srcs]
    assert torch.equal(ops.sum_f32_to_bf16(s4, dst=torch.empty(n4, device="cuda")), ordered[:n4])
