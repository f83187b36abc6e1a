"""The 6-bit (MXFP6) decode weights on the device: the checks of tests/_w6_cases.py (shared with the host emulation) over
guarded device buffers -- the quantiser bitwise against the numpy restatement, the GEMV and the 5-32-row entry bitwise, outputs
and workspace partials, against the device's bf16 entries on the dequantised weights -- and the model: after
quantize_decode_weights("fp6") every generate route gives the tokens and logits of the same (rounded) model streaming bf16,
through lwm_gemv_fused_w6 at up to four rows and lwm_gemm_rows_fused_w6 above.  Every check is exact."""
import numpy as np
import pytest

from tests import _rows_cases as RC, _w6_cases as WC, _w6_ref as W6, _w8_ref as W8

pytestmark = pytest.mark.gpu
ids = lambda v: str(v).replace(" ", "")


class Guarded:
    """a device buffer between two guard bands of FILL bytes (the backend buffer of tests/_rows_cases.py): reading or
    writing next to a tensor shows"""

    def __init__(self, arr):
        import torch
        arr = np.ascontiguousarray(arr)
        self.dtype, self.shape, self.n = arr.dtype, arr.shape, arr.nbytes
        self.raw = torch.full((self.n + 2 * RC.GUARD,), RC.FILL, dtype=torch.uint8, device="cuda")
        self.raw[RC.GUARD:RC.GUARD + self.n].copy_(torch.from_numpy(arr.reshape(-1).view(np.uint8)))
        self.ptr = self.raw.data_ptr() + RC.GUARD
        assert self.ptr % 16 == 0

    def read(self):
        return self.raw[RC.GUARD:RC.GUARD + self.n].cpu().numpy().view(self.dtype).reshape(self.shape).copy()

    def intact(self):
        return bool((self.raw[:RC.GUARD] == RC.FILL).all() and (self.raw[RC.GUARD + self.n:] == RC.FILL).all())


class DevBackend:
    def lib(self):
        from lwm_amd._lib import lib
        return lib()

    def buf(self, arr):
        return Guarded(arr)

    def sync(self):
        import torch
        torch.cuda.synchronize()


B = DevBackend()


# ---------------------------------------------------------------- kernels
@pytest.mark.parametrize("case", W6.quantiser_cases(), ids=lambda c: c[0])
def test_quantiser_equals_the_restatement(case):
    WC.check_quantiser(B, case[1])
    a, b = WC.quantise(B, case[1]), WC.quantise(B, case[1])            # determinism: two launches, equal bits
    assert all(np.array_equal(u, v) for u, v in zip(a, b))


def test_quantiser_refusals_touch_nothing():
    WC.check_quantiser_refusals(B)


@pytest.mark.parametrize("K,Ns", W8.GEMV_SHAPES, ids=ids)
def test_gemv_equals_the_bf16_gemv_on_the_rounded_weights(K, Ns):
    for rows in (1, 2, 3, 4):
        WC.check_gemv(B, rows, K, Ns)


@pytest.mark.parametrize("rows", [1, 4])
@pytest.mark.parametrize("K,N", [(160, 48), (416, 2064)])
def test_gemv_norm_on_load(rows, K, N):
    WC.check_gemv_norm(B, rows, K, N)


@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("K,N", [(160, 128), (416, 1152)])
def test_gemv_residual_and_ss_out(rows, K, N):
    WC.check_gemv_residual_ss(B, rows, K, N)


def test_both_entries_through_the_quantiser_kernel():
    WC.check_through_the_quantiser(B)


@pytest.mark.parametrize("rows", [5, 17, 32])
@pytest.mark.parametrize("K,Ns", WC.ROWS_SHAPES, ids=ids)
def test_rows_entry_equals_the_bf16_rows_entry_on_the_rounded_weights(rows, K, Ns):
    WC.check_rows(B, rows, K, Ns)


@pytest.mark.parametrize("rows", [5, 32])
def test_rows_entry_norm_residual_and_ss_out(rows):
    WC.check_rows_residual_ss(B, rows)


def test_a_row_has_the_same_bits_in_a_batch_of_5_and_of_32():
    WC.check_row_independence(B)


@pytest.mark.parametrize("entry", ["gemv", "rows"])
def test_refusals_touch_nothing(entry):
    for name in WC.refusal_names(entry):
        WC.check_refusal(B, entry, name)
    WC.check_accepted(B, entry)


def _bf16(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16)


def test_python_wrappers_round_in_place_and_agree():
    """lwm_amd.w6: quantise_weight rounds the tensor in place, bumps its version, w6_dequant of the pack IS the tensor, and
    the two wrappers on the pack equal llama_ops.gemv_fused / gemm_rows_fused on the rounded tensor"""
    import torch
    from lwm_amd import llama_ops as LO, w6
    x, (w,) = W6.gemv_case(9, 416, (1152,))
    q_ref, e_ref = W6.quantise(w)
    k = _bf16(w).cuda()
    v0 = k._version
    p = w6.quantise_weight(k)
    assert k._version > v0 and p.stamp == (k._version, k.data_ptr()) and p.shape == (416, 1152)
    assert np.array_equal(p.q.cpu().numpy(), q_ref) and np.array_equal(p.scale.cpu().numpy(), e_ref)
    assert np.array_equal(k.float().cpu().numpy(), W6.rounded(q_ref, e_ref, w.shape))
    assert torch.equal(w6.w6_dequant(p.q, p.scale, p.shape), k)
    xd = _bf16(x).cuda()
    res = torch.randn(9, 1152, device="cuda").to(torch.bfloat16)
    for rows, mine, theirs in ((3, w6.gemv_fused_w6, LO.gemv_fused), (9, w6.gemm_rows_fused_w6, LO.gemm_rows_fused)):
        (a,), sa = mine(xd[:rows], [p], residual=res[:rows], want_ss=True)
        (b,), sb = theirs(xd[:rows], [k], residual=res[:rows], want_ss=True)
        assert torch.equal(a, b) and torch.equal(sa, sb)
        (a,) = mine(xd[:rows], [p], out_dtype=torch.float32)
        assert torch.equal(a, theirs(xd[:rows], [k], out_dtype=torch.float32)[0])


# ---------------------------------------------------------------- model (the tiny model of tests/test_gpu_w4.py)
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


def _others(monkeypatch):
    """call counters of the 8-bit and 4-bit wrappers: they must stay empty while the 6-bit packs are held"""
    from lwm_amd import w4, w8
    return [_count_calls(monkeypatch, m, n) for m, n in ((w8, "gemv_fused_w8"), (w8, "gemm_rows_fused_w8"), (w4, "gemv_fused_w4"))]


def test_generate_streams_the_packs_and_equals_the_rounded_bf16_model(monkeypatch):
    import torch
    from lwm_amd import w6
    from lwm_amd.llama import LLaMAConfig, LLaMAForCausalLM
    torch.manual_seed(0)
    model = _spread(LLaMAForCausalLM(LLaMAConfig(**CFG)).cuda())
    ids1 = torch.randint(3, 272, (1, 9), device="cuda")
    ids3 = torch.randint(3, 272, (3, 11), device="cuda")
    mask3 = torch.ones(3, 11, dtype=torch.int32, device="cuda")
    mask3[0, :4] = 0
    mask3[2, :1] = 0                                               # left padding
    before = {n: p.detach().clone() for n, p in model._decode_weight_params()}
    assert model.quantize_decode_weights("fp6") is model and model.decode_packs("fp8") is None and model.decode_packs("fp4") is None
    # the model IS the rounded model: every parameter equals what its pack stands for, and moved by less than a fifteenth
    # of its block's amax (codes at most 0.5 apart at the top of a scale that holds amax / s > 3.75)
    for n, p in model._decode_weight_params():
        pk = model.decode_packs("fp6")[n]
        assert torch.equal(p, w6.w6_dequant(pk.q, pk.scale, pk.shape)), n
        amax = before[n].float().abs().reshape(-1, 32, p.shape[1]).amax(1).repeat_interleave(32, 0)
        assert ((p.float() - before[n].float()).abs() < amax / 15).all(), n
        assert not torch.equal(p, before[n]), n
    calls, rows_calls, others = _count_calls(monkeypatch, w6, "gemv_fused_w6"), _count_calls(monkeypatch, w6, "gemm_rows_fused_w6"), _others(monkeypatch)
    kw = dict(max_new_tokens=6, return_logits=True)
    routes = [dict(input_ids=ids1), dict(input_ids=ids1, graph=True),
              dict(input_ids=ids3, attention_mask=mask3), dict(input_ids=ids3, attention_mask=mask3, graph=True),
              dict(input_ids=ids1, kv_dtype="fp8"), dict(input_ids=ids3, attention_mask=mask3, kv_dtype="fp6", graph=True),
              dict(input_ids=ids1, kv_dtype="fp4"), dict(input_ids=ids3, attention_mask=mask3, prefill_chunk=4)]
    got = [model.generate(**r, **kw) for r in routes]
    n_calls = len(calls)
    assert n_calls >= len(routes) * (6 + 2 * 4) and set(calls) == {1, 2, 3}       # heads and the four launch pairs per layer
    assert not rows_calls and not any(others)
    assert model.drop_decode_weights() is model and model.decode_packs("fp6") is None and model.decode_packs("fp8") is None and model.decode_packs("fp4") is None
    ref = [model.generate(**r, **kw) for r in routes]
    assert len(calls) == n_calls                                   # bf16 streaming again
    for r, (tg, lg), (tr, lr) in zip(routes, got, ref):
        assert torch.equal(tg, tr) and torch.equal(lg, lr), {k: v for k, v in r.items() if k != "input_ids" and k != "attention_mask"}
        assert lg.shape[:2] == (r["input_ids"].shape[0], 6) and torch.isfinite(lg).all()
    assert len({tuple(t.flatten().tolist()) for t, _ in got[:1] + got[2:3]}) == 2
    # quantising the rounded model again changes no value
    snap = {n: p.detach().clone() for n, p in model._decode_weight_params()}
    model.quantize_decode_weights("fp6")
    assert all(torch.equal(p, snap[n]) for n, p in model._decode_weight_params())


def test_generate_vision_heads_stream_the_packs(monkeypatch):
    import torch
    from lwm_amd import w6
    from lwm_amd.vision_llama import VideoLLaMAConfig, VideoLLaMAForCausalLM
    torch.manual_seed(0)
    cfg = VideoLLaMAConfig(**CFG, vision_vocab_size=272, sample_mode="vision")
    model = _spread(VideoLLaMAForCausalLM(cfg).cuda())
    model.quantize_decode_weights("fp6")
    assert "vision_head" in model.decode_packs("fp6") and "lm_head" in model.decode_packs("fp6")
    ids = torch.randint(3, 272, (1, 7), device="cuda")
    ids = torch.cat([ids, torch.full_like(ids, 1)], 0)            # conditional + unconditional
    calls, others = _count_calls(monkeypatch, w6, "gemv_fused_w6"), _others(monkeypatch)
    kw = dict(cfg_scales=[3.0], max_new_tokens=6, temperature=0.8, top_k=40, seed=11, return_logits=True)
    got = [model.generate_vision(ids, **kw), model.generate_vision(ids, graph=True, **kw)]
    assert len(calls) >= 2 * 2 and 1 in calls and not any(others)      # (one pack per call: the heads among them)
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
    model = LLaMAForCausalLM(LLaMAConfig(**CFG)).cuda().quantize_decode_weights("fp6")
    ids = torch.randint(3, 272, (1, 5), device="cuda")
    model.generate(ids, max_new_tokens=3)
    with torch.no_grad():
        model.h[1].attention.wq.mul_(2)
    with pytest.raises(RuntimeError, match=r"h\.1\.attention\.wq.*quantize_decode_weights\('fp6'\)"):
        model.generate(ids, max_new_tokens=3)
    model.quantize_decode_weights("fp6")                           # quantise again: accepted
    model.generate(ids, max_new_tokens=3)
    with torch.no_grad():
        model.lm_head.add_(1)
    with pytest.raises(RuntimeError, match="lm_head"):
        model.generate(ids, max_new_tokens=1)
    model.drop_decode_weights()
    model.generate(ids, max_new_tokens=2)


def test_switching_between_the_formats(monkeypatch):
    """fp6 -> fp8 -> fp6 -> fp4 -> bf16: one kind of pack at a time, each route streams its own, and the refusals name the mode"""
    import torch
    from lwm_amd import w4, w6, w8
    from lwm_amd.cli import _common
    from lwm_amd.llama import LLaMAConfig, LLaMAForCausalLM
    torch.manual_seed(0)
    model = _spread(LLaMAForCausalLM(LLaMAConfig(**CFG)).cuda())
    ids = torch.randint(3, 272, (2, 5), device="cuda")
    c8, c6, c4 = (_count_calls(monkeypatch, m, n) for m, n in ((w8, "gemv_fused_w8"), (w6, "gemv_fused_w6"), (w4, "gemv_fused_w4")))
    kw = dict(max_new_tokens=3, return_logits=True)
    model.quantize_decode_weights("fp6")
    assert model.decode_packs("fp8") is None and model.decode_packs("fp4") is None and len(model.decode_packs("fp6")) == 2 * 7 + 1
    t6, l6 = model.generate(ids, **kw)
    n6 = len(c6)
    assert n6 > 0 and not c8 and not c4
    model.quantize_decode_weights("fp8")
    assert model.decode_packs("fp6") is None and model.decode_packs("fp4") is None and len(model.decode_packs("fp8")) == 2 * 7 + 1
    model.generate(ids, **kw)
    n8 = len(c8)
    assert n8 > 0 and len(c6) == n6
    model.quantize_decode_weights("fp6")
    assert model.decode_packs("fp8") is None and len(model.decode_packs("fp6")) == 2 * 7 + 1
    model.generate(ids, **kw)
    assert len(c6) > n6 and len(c8) == n8
    n6 = len(c6)
    model.quantize_decode_weights("fp4")
    assert model.decode_packs("fp6") is None and model.decode_packs("fp8") is None and len(model.decode_packs("fp4")) == 2 * 7 + 1
    model.generate(ids, **kw)
    assert len(c4) > 0 and len(c6) == n6
    model.quantize_decode_weights("fp6").quantize_decode_weights("bf16")
    assert model.decode_packs("fp8") is None and model.decode_packs("fp6") is None and model.decode_packs("fp4") is None
    n4 = len(c4)
    model.generate(ids, **kw)
    assert len(c6) == n6 and len(c8) == n8 and len(c4) == n4
    with pytest.raises(ValueError, match="int6"):
        model.quantize_decode_weights("int6")
    monkeypatch.setenv("LWM_DECODE_WEIGHTS", "FP6")
    assert _common.apply_decode_weights(model) is model and len(model.decode_packs("fp6")) == 2 * 7 + 1 and model.decode_packs("fp8") is None and model.decode_packs("fp4") is None
    f32 = LLaMAForCausalLM(LLaMAConfig(**CFG), torch.float32).cuda()
    with pytest.raises(NotImplementedError, match=r"'fp6'.*float32 model.*6-bit"):
        f32.quantize_decode_weights("fp6")
    assert f32.decode_packs("fp6") is None


def test_a_five_row_step_takes_the_6_bit_rows_kernel(monkeypatch):
    """decode_rows = 8, five rows: the step and the head run lwm_gemm_rows_fused_w6 over the packs, to the bits of
    gemm_rows_fused over the rounded bf16 parameters; under a graph too"""
    import torch
    from lwm_amd import llama_ops, w6
    from lwm_amd.llama import LLaMAConfig, LLaMAForCausalLM
    torch.manual_seed(0)
    model = _spread(LLaMAForCausalLM(LLaMAConfig(**CFG)).cuda())
    model.decode_rows = 8
    ids = torch.randint(3, 272, (5, 6), device="cuda")
    model.quantize_decode_weights("fp6")
    c6, c6rows = _count_calls(monkeypatch, w6, "gemv_fused_w6"), _count_calls(monkeypatch, w6, "gemm_rows_fused_w6")
    crows, others = _count_calls(monkeypatch, llama_ops, "gemm_rows_fused"), _others(monkeypatch)
    kw = dict(max_new_tokens=4, return_logits=True)
    got = [model.generate(ids, **kw), model.generate(ids, graph=True, **kw)]
    assert not c6 and not crows and not any(others) and len(c6rows) >= 3 * (2 * 4 + 1) and set(c6rows) == {1, 2, 3}
    n_rows = len(c6rows)
    model.drop_decode_weights()
    ref = [model.generate(ids, **kw), model.generate(ids, graph=True, **kw)]
    assert len(c6rows) == n_rows and len(crows) >= 3 * 2 * 4
    for (tg, lg), (tr, lr) in zip(got, ref):
        assert torch.equal(tg, tr) and torch.equal(lg, lr) and torch.isfinite(lg).all()
