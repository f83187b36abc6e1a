"""The 4-bit (MXFP4) decode weights on the device: the quantiser bitwise against the numpy restatement (tests/_w4_ref.py), the
GEMV bitwise -- outputs and workspace partials -- against the device's bf16 GEMV on the dequantised weights, guard bands
around everything the kernels read and write, determinism, and the model: after quantize_decode_weights("fp4") every
generate route gives the tokens and logits of the same (rounded) model streaming bf16.  Every check is exact."""
import ctypes as C

import numpy as np
import pytest

from tests import _w4_ref as W4, _w8_ref as W8

pytestmark = pytest.mark.gpu

GUARD = 256              # bytes either side of a guarded buffer
FILL = 0xA5


class Guarded:
    """a device buffer between two guard bands of FILL bytes; `.t` is the tensor inside"""

    def __init__(self, shape, dtype, init=None):
        import torch
        n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        self.raw = torch.full((n + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda")
        self.t = self.raw[GUARD:GUARD + n].view(dtype).view(*shape)
        if init is not None:
            self.t.copy_(init)
        assert self.t.data_ptr() % 16 == 0

    def intact(self):
        return bool((self.raw[:GUARD] == FILL).all() and (self.raw[-GUARD:] == FILL).all())

    @property
    def ptr(self):
        return self.t.data_ptr()


def _bf16(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16)


def _bits(t):
    import torch
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32 if t.element_size() == 4 else torch.uint8)


def dev_quantise(w, in_place=False):
    """w (K, N) f32 of bf16 values -> Guarded codes, scale bytes, rounded through lwm_w4_quantise on the device"""
    import torch
    from lwm_amd import _capi
    from lwm_amd._lib import lib
    K, N = w.shape
    src = Guarded((K, N), torch.bfloat16, _bf16(w))
    q, s = Guarded((K // 4, N // 8, 16), torch.uint8), Guarded((K // 32, N), torch.uint8)
    r = src if in_place else Guarded((K, N), torch.bfloat16)
    L = lib()
    _capi.check(L, L.lwm_w4_quantise(src.ptr, q.ptr, s.ptr, r.ptr, K, N, None), "lwm_w4_quantise")
    torch.cuda.synchronize()
    assert src.intact() and q.intact() and s.intact() and r.intact()
    return q, s, r


def dev_gemv(x, mats, *, w4, norm=None, residual=None, want_ss=False, want_f32=False):
    """emu_gemv of tests/test_emu_w4.py on the device, every buffer guarded -> ([y], ss_out or None, workspace) tensors"""
    import torch
    from lwm_amd import _capi
    from lwm_amd._lib import lib
    L = lib()
    rows, K = x.shape
    Ns = [(m[1] if w4 else m).shape[1] for m in mats]
    xb = Guarded((rows, K), torch.bfloat16, _bf16(x))
    work = Guarded((sum(max(L.lwm_gemv_workspace_bytes(rows, K, N), 16) for N in Ns) // 4,), torch.float32)
    a = (_capi.LwmGemvW4Args if w4 else _capi.LwmGemvArgs)()
    a.x, a.ldx, a.nmat, a.rows, a.K, a.workspace = xb.ptr, K, len(mats), rows, K, work.ptr
    guarded, ys = [xb, work], []
    for i, m in enumerate(mats):
        if w4:
            q = Guarded(m[0].shape, torch.uint8, torch.from_numpy(m[0]))
            s = Guarded(m[1].shape, torch.uint8, torch.from_numpy(m[1]))
            a.w[i], a.w_scale[i] = q.ptr, s.ptr
            guarded += [q, s]
        else:
            wb = Guarded(m.shape, torch.bfloat16, _bf16(m))
            a.w[i] = wb.ptr
            guarded.append(wb)
        a.N[i] = Ns[i]
        y = Guarded((rows, Ns[i]), torch.float32 if want_f32 else torch.bfloat16)
        if want_f32:
            a.y_f32[i] = y.ptr
        else:
            a.y[i], a.ldy[i] = y.ptr, Ns[i]
        ys.append(y)
    if norm is not None:
        ss, gam, eps = norm
        ssa, gb = Guarded(ss.shape, torch.float32, torch.from_numpy(ss)), Guarded(gam.shape, torch.bfloat16, _bf16(gam))
        a.norm_weight, a.ss_in, a.ss_n, a.eps = gb.ptr, ssa.ptr, ss.shape[1], eps
        guarded += [ssa, gb]
    if residual is not None:
        rb = Guarded(residual.shape, torch.bfloat16, _bf16(residual))
        a.residual[0], a.ldres[0] = rb.ptr, Ns[0]
        guarded.append(rb)
    sso = None
    if want_ss:
        sso = Guarded((rows, Ns[0] // 128), torch.float32)
        a.ss_out = sso.ptr
        guarded.append(sso)
    fn, name = (L.lwm_gemv_fused_w4, "lwm_gemv_fused_w4") if w4 else (L.lwm_gemv_fused_bf16, "lwm_gemv_fused_bf16")
    _capi.check(L, fn(C.byref(a), None), name)
    torch.cuda.synchronize()
    assert all(g.intact() for g in guarded + ys), "a guard band was written"
    if w4:      # the inputs the kernel reads are what they were: codes and scale bytes
        for i, m in enumerate(mats):
            assert np.array_equal(guarded[2 + 2 * i].t.cpu().numpy(), m[0]) and np.array_equal(guarded[3 + 2 * i].t.cpu().numpy(), m[1])
    used = sum(L.lwm_gemv_workspace_bytes(rows, K, N) for N in Ns) // 4
    return [_bits(y.t).clone() for y in ys], None if sso is None else _bits(sso.t).clone(), _bits(work.t)[:used].clone()


@pytest.fixture(scope="module")
def packs_of():
    """(K, Ns, rows) -> x, numpy packs, dequantised weights: computed once, shared, never modified"""
    memo = {}

    def get(rows, K, Ns):
        key = (rows, K, tuple(Ns))
        if key not in memo:
            x, ws = W4.gemv_case(rows, K, Ns)
            packs = [W4.quantise(w) for w in ws]
            memo[key] = (x, packs, [W4.dequant(q, e, w.shape).astype(np.float32) for (q, e), w in zip(packs, ws)])
        return memo[key]
    return get


# ---------------------------------------------------------------- quantiser
@pytest.mark.parametrize("case", W4.quantiser_cases(), ids=lambda c: c[0])
def test_quantiser_equals_the_restatement(case):
    import torch
    from oracle import attention_ref as R
    name, w = case
    q_ref, e_ref = W4.quantise(w)
    r_ref = R.to_bf16_bits(W4.rounded(q_ref, e_ref, w.shape)).astype(np.int16)
    for in_place in (False, True):
        q, s, r = dev_quantise(w, in_place)
        assert np.array_equal(s.t.cpu().numpy(), e_ref)
        assert np.array_equal(q.t.cpu().numpy(), q_ref)
        assert np.array_equal(r.t.view(torch.int16).cpu().numpy(), r_ref)
    q2, s2, r2 = dev_quantise(w)                                   # determinism: two launches, equal bits
    assert torch.equal(q2.t, q.t) and torch.equal(s2.t, s.t) and torch.equal(_bits(r2.t), _bits(r.t))
    _, _, r3 = dev_quantise(W4.rounded(q_ref, e_ref, w.shape))     # idempotent: the rounded weights are a fixed point
    assert torch.equal(_bits(r3.t), _bits(r.t))


# ---------------------------------------------------------------- GEMV
@pytest.mark.parametrize("K,Ns", W8.GEMV_SHAPES, ids=lambda v: str(v).replace(" ", ""))
def test_gemv_equals_the_bf16_gemv_on_the_rounded_weights(K, Ns, packs_of):
    import torch
    for rows in (1, 2, 3, 4):
        x, packs, deq = packs_of(rows, K, Ns)
        for f32 in (False, True):
            got, _, work = dev_gemv(x, packs, w4=True, want_f32=f32)
            ref, _, rwork = dev_gemv(x, deq, w4=False, want_f32=f32)
            assert torch.equal(work, rwork), rows                      # every partial, bit for bit
            assert all(torch.equal(g, r) for g, r in zip(got, ref)), rows
            assert all(bool(g.any()) for g in got)
        again, _, work2 = dev_gemv(x, packs, w4=True, want_f32=True)   # determinism
        assert torch.equal(work2, work) and all(torch.equal(a, g) for a, g in zip(again, got))


@pytest.mark.parametrize("rows", [1, 4])
@pytest.mark.parametrize("K,N", [(160, 48), (416, 2064)])
def test_gemv_norm_on_load(rows, K, N, packs_of):
    import torch
    from oracle import attention_ref as R
    x, packs, deq = packs_of(rows, K, (N, 16))
    rng = np.random.default_rng(5)
    gam = R.round_bf16((1.0 + 0.2 * rng.standard_normal(K)).astype(np.float32))
    for n_ss in (1, 5, 64):
        ss = (rng.dirichlet(np.ones(n_ss), size=rows) * (x.astype(np.float64) ** 2).sum(-1, keepdims=True)).astype(np.float32)
        for f32 in (False, True):
            got, _, work = dev_gemv(x, packs, w4=True, norm=(ss, gam, 1e-6), want_f32=f32)
            ref, _, rwork = dev_gemv(x, deq, w4=False, norm=(ss, gam, 1e-6), want_f32=f32)
            assert torch.equal(work, rwork) and all(torch.equal(g, r) for g, r in zip(got, ref))


@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("K,N", [(160, 128), (416, 1152)])
def test_gemv_residual_and_ss_out(rows, K, N, packs_of):
    import torch
    from oracle import attention_ref as R
    x, packs, deq = packs_of(rows, K, (N,))
    res = R.round_bf16(np.random.default_rng(6).standard_normal((rows, N)).astype(np.float32) * 4.0)
    (g,), gss, work = dev_gemv(x, packs, w4=True, residual=res, want_ss=True)
    (r,), rss, rwork = dev_gemv(x, deq, w4=False, residual=res, want_ss=True)
    assert torch.equal(work, rwork) and torch.equal(g, r) and torch.equal(gss, rss)


def test_python_wrappers_round_in_place_and_agree():
    """lwm_amd.w4: quantise_weight rounds the tensor in place, bumps its version, w4_dequant of the pack IS the tensor, and
    gemv_fused_w4 on the pack equals llama_ops.gemv_fused on the rounded tensor"""
    import torch
    from lwm_amd import llama_ops as LO, w4
    x, (w,) = W4.gemv_case(3, 416, (1152,))
    q_ref, e_ref = W4.quantise(w)
    k = _bf16(w).cuda()
    v0 = k._version
    p = w4.quantise_weight(k)
    assert k._version > v0 and p.stamp == (k._version, k.data_ptr()) and p.shape == (416, 1152)
    assert np.array_equal(p.q.cpu().numpy(), q_ref) and np.array_equal(p.scale.cpu().numpy(), e_ref)
    assert np.array_equal(k.float().cpu().numpy(), W4.rounded(q_ref, e_ref, w.shape))
    assert torch.equal(w4.w4_dequant(p.q, p.scale, p.shape), k)
    xd = _bf16(x).cuda()
    res = torch.randn(3, 1152, device="cuda").to(torch.bfloat16)
    (a,), sa = w4.gemv_fused_w4(xd, [p], residual=res, want_ss=True)
    (b,), sb = LO.gemv_fused(xd, [k], residual=res, want_ss=True)
    assert torch.equal(a, b) and torch.equal(sa, sb)
    (a,) = w4.gemv_fused_w4(xd, [p], out_dtype=torch.float32)
    assert torch.equal(a, LO.gemv_fused(xd, [k], out_dtype=torch.float32)[0])


# ---------------------------------------------------------------- model
CFG = dict(vocab_size=272, hidden_size=256, intermediate_size=352, num_hidden_layers=2, num_attention_heads=2,
           max_sequence_length=128)


def _spread(model):
    """weights of ordinary size instead of the 0.02 initialisation: logits that tell tokens apart"""
    import torch
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if p.dim() == 2:
                p.copy_((torch.randn(p.shape, generator=g) * (1.5 / p.shape[0] ** 0.5 if "wte" not in n and "vte" not in n else 1.0))
                        .to(p.dtype))
    return model


def _count_calls(monkeypatch, module, name):
    calls, real = [], getattr(module, name)

    def counted(x, mats, **kw):
        calls.append(len(mats))
        return real(x, mats, **kw)
    monkeypatch.setattr(module, name, counted)
    return calls


def test_generate_streams_the_packs_and_equals_the_rounded_bf16_model(monkeypatch):
    import torch
    from lwm_amd import w4
    from lwm_amd.llama import LLaMAConfig, LLaMAForCausalLM
    torch.manual_seed(0)
    model = _spread(LLaMAForCausalLM(LLaMAConfig(**CFG)).cuda())
    ids1 = torch.randint(3, 272, (1, 9), device="cuda")
    ids3 = torch.randint(3, 272, (3, 11), device="cuda")
    mask3 = torch.ones(3, 11, dtype=torch.int32, device="cuda")
    mask3[0, :4] = 0
    mask3[2, :1] = 0                                               # left padding
    before = {n: p.detach().clone() for n, p in model._decode_weight_params()}
    assert model.quantize_decode_weights("fp4") is model and model.decode_packs("fp8") is None
    # the model IS the rounded model: every parameter equals what its pack stands for, and moved by at most a third of
    # its block's amax (codes at most 2 apart at the top of a scale that holds amax / s > 3)
    for n, p in model._decode_weight_params():
        pk = model.decode_packs("fp4")[n]
        assert torch.equal(p, w4.w4_dequant(pk.q, pk.scale, pk.shape)), n
        amax = before[n].float().abs().reshape(-1, 32, p.shape[1]).amax(1).repeat_interleave(32, 0)
        assert ((p.float() - before[n].float()).abs() <= amax / 3).all(), n
        assert not torch.equal(p, before[n]), n
    calls = _count_calls(monkeypatch, w4, "gemv_fused_w4")
    kw = dict(max_new_tokens=6, return_logits=True)
    routes = [dict(input_ids=ids1), dict(input_ids=ids1, graph=True),
              dict(input_ids=ids3, attention_mask=mask3), dict(input_ids=ids3, attention_mask=mask3, graph=True),
              dict(input_ids=ids1, kv_dtype="fp8"), dict(input_ids=ids3, attention_mask=mask3, kv_dtype="fp8", graph=True),
              dict(input_ids=ids1, kv_dtype="fp4"), dict(input_ids=ids3, attention_mask=mask3, kv_dtype="fp4", graph=True),
              dict(input_ids=ids3, attention_mask=mask3, prefill_chunk=4)]
    got = [model.generate(**r, **kw) for r in routes]
    n_calls = len(calls)
    assert n_calls >= len(routes) * (6 + 2 * 4) and set(calls) == {1, 2, 3}       # heads and the four launch pairs per layer
    assert model.drop_decode_weights() is model and model.decode_packs("fp4") is None and model.decode_packs("fp8") is None
    ref = [model.generate(**r, **kw) for r in routes]
    assert len(calls) == n_calls                                   # bf16 streaming again
    for r, (tg, lg), (tr, lr) in zip(routes, got, ref):
        assert torch.equal(tg, tr) and torch.equal(lg, lr), {k: v for k, v in r.items() if k != "input_ids" and k != "attention_mask"}
        assert lg.shape[:2] == (r["input_ids"].shape[0], 6) and torch.isfinite(lg).all()
    assert len({tuple(t.flatten().tolist()) for t, _ in got[:1] + got[2:3]}) == 2
    # quantising the rounded model again changes no value
    snap = {n: p.detach().clone() for n, p in model._decode_weight_params()}
    model.quantize_decode_weights("fp4")
    assert all(torch.equal(p, snap[n]) for n, p in model._decode_weight_params())


def test_generate_vision_with_cfg(monkeypatch):
    import torch
    from lwm_amd import w4
    from lwm_amd.vision_llama import VideoLLaMAConfig, VideoLLaMAForCausalLM
    torch.manual_seed(0)
    cfg = VideoLLaMAConfig(**CFG, vision_vocab_size=272, sample_mode="vision")
    model = _spread(VideoLLaMAForCausalLM(cfg).cuda())
    model.quantize_decode_weights("fp4")
    assert "vision_head" in model.decode_packs("fp4") and "lm_head" in model.decode_packs("fp4")
    ids = torch.randint(3, 272, (1, 7), device="cuda")
    ids = torch.cat([ids, torch.full_like(ids, 1)], 0)            # conditional + unconditional
    calls = _count_calls(monkeypatch, w4, "gemv_fused_w4")
    kw = dict(cfg_scales=[3.0], max_new_tokens=6, temperature=0.8, top_k=40, seed=11, return_logits=True)
    got = [model.generate_vision(ids, **kw), model.generate_vision(ids, graph=True, **kw)]
    assert len(calls) >= 2 * 2
    n_calls = len(calls)
    model.drop_decode_weights()
    ref = [model.generate_vision(ids, **kw), model.generate_vision(ids, graph=True, **kw)]
    assert len(calls) == n_calls
    for (tg, lg), (tr, lr) in zip(got, ref):
        assert torch.equal(tg, tr) and torch.equal(lg, lr) and lg.shape[:2] == (2, 6)


def test_a_stale_pack_is_refused():
    import torch
    from lwm_amd.llama import LLaMAConfig, LLaMAForCausalLM
    torch.manual_seed(0)
    model = LLaMAForCausalLM(LLaMAConfig(**CFG)).cuda().quantize_decode_weights("fp4")
    ids = torch.randint(3, 272, (1, 5), device="cuda")
    model.generate(ids, max_new_tokens=3)
    with torch.no_grad():
        model.h[1].attention.wq.mul_(2)
    with pytest.raises(RuntimeError, match=r"h\.1\.attention\.wq.*quantize_decode_weights\('fp4'\)"):
        model.generate(ids, max_new_tokens=3)
    model.quantize_decode_weights("fp4")                           # quantise again: accepted
    model.generate(ids, max_new_tokens=3)
    with torch.no_grad():
        model.lm_head.add_(1)
    with pytest.raises(RuntimeError, match="lm_head"):
        model.generate(ids, max_new_tokens=1)
    model.drop_decode_weights()
    model.generate(ids, max_new_tokens=2)


def test_switching_between_the_formats(monkeypatch):
    """fp8 -> fp4 -> bf16: one kind of pack at a time, each route streams its own, and the refusals name the mode"""
    import torch
    from lwm_amd import w4, w8
    from lwm_amd.cli import _common
    from lwm_amd.llama import LLaMAConfig, LLaMAForCausalLM
    torch.manual_seed(0)
    model = _spread(LLaMAForCausalLM(LLaMAConfig(**CFG)).cuda())
    ids = torch.randint(3, 272, (2, 5), device="cuda")
    c8, c4 = _count_calls(monkeypatch, w8, "gemv_fused_w8"), _count_calls(monkeypatch, w4, "gemv_fused_w4")
    kw = dict(max_new_tokens=3, return_logits=True)
    model.quantize_decode_weights("fp8")
    assert model.decode_packs("fp4") is None and len(model.decode_packs("fp8")) == 2 * 7 + 1
    model.generate(ids, **kw)
    n8 = len(c8)
    assert n8 > 0 and not c4
    model.quantize_decode_weights("fp4")
    assert model.decode_packs("fp8") is None and len(model.decode_packs("fp4")) == 2 * 7 + 1
    t4, l4 = model.generate(ids, **kw)
    n4 = len(c4)
    assert n4 > 0 and len(c8) == n8
    model.quantize_decode_weights("bf16")
    assert model.decode_packs("fp8") is None and model.decode_packs("fp4") is None
    tb, lb = model.generate(ids, **kw)
    assert len(c4) == n4 and len(c8) == n8 and torch.equal(t4, tb) and torch.equal(l4, lb)
    model.quantize_decode_weights("fp4").quantize_decode_weights("fp8")           # and back: the 8-bit packs replace the 4-bit ones
    assert model.decode_packs("fp4") is None and model.decode_packs("fp8") is not None
    t8, l8 = model.generate(ids, **kw)
    assert len(c8) > n8 and len(c4) == n4
    with pytest.raises(ValueError, match="int4"):
        model.quantize_decode_weights("int4")
    model.drop_decode_weights()
    monkeypatch.setenv("LWM_DECODE_WEIGHTS", "FP4")
    assert _common.apply_decode_weights(model) is model and len(model.decode_packs("fp4")) == 2 * 7 + 1 and model.decode_packs("fp8") is None
    f32 = LLaMAForCausalLM(LLaMAConfig(**CFG), torch.float32).cuda()
    with pytest.raises(NotImplementedError, match="float32 model"):
        f32.quantize_decode_weights("fp4")
    assert f32.decode_packs("fp4") is None


def test_a_five_row_step_takes_the_bf16_rows_kernel(monkeypatch):
    """decode_rows = 8, five rows: no 4-bit body above 4 rows -- the step runs gemm_rows_fused over the rounded bf16 parameters,
    with and without the packs, to the same bits"""
    import torch
    from lwm_amd import llama_ops, w4
    from lwm_amd.llama import LLaMAConfig, LLaMAForCausalLM
    torch.manual_seed(0)
    model = _spread(LLaMAForCausalLM(LLaMAConfig(**CFG)).cuda())
    model.decode_rows = 8
    ids = torch.randint(3, 272, (5, 6), device="cuda")
    model.quantize_decode_weights("fp4")
    c4, crows = _count_calls(monkeypatch, w4, "gemv_fused_w4"), _count_calls(monkeypatch, llama_ops, "gemm_rows_fused")
    kw = dict(max_new_tokens=4, return_logits=True)
    tg, lg = model.generate(ids, **kw)
    assert not c4 and len(crows) >= 3 * 2 * 4
    n_rows = len(crows)
    model.drop_decode_weights()
    tr, lr = model.generate(ids, **kw)
    assert len(crows) == 2 * n_rows and torch.equal(tg, tr) and torch.equal(lg, lr) and torch.isfinite(lg).all()
