"""lwm_gemm_rows_fused_bf16 / lwm_gemm_rows_fused_w8 (csrc/gemm_rows.h) on the device -- the checks of tests/_rows_cases.py
(shared with the host emulation) over guarded device buffers -- and the routing: with decode_rows set, one-token steps of
5..N rows run through the fused step and the new entries (text and vision model, graphs, 8-bit packs, the 8-bit KV cache);
unset, nothing moves."""
import numpy as np
import pytest

from tests import _rows_cases as RC

pytestmark = pytest.mark.gpu
ids = lambda v: str(v).replace(" ", "")


class DevBuf:
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
        return DevBuf(arr)

    def sync(self):
        import torch
        torch.cuda.synchronize()


B = DevBackend()


# ---------------------------------------------------------------- kernels
@pytest.mark.parametrize("rows", RC.ROWS)
@pytest.mark.parametrize("Ns", RC.NSETS, ids=ids)
@pytest.mark.parametrize("K", RC.KS_)
def test_exact_cases(K, Ns, rows):
    RC.check_exact(B, rows, K, Ns)


@pytest.mark.parametrize("rows", RC.ROWS)
@pytest.mark.parametrize("Ns", RC.SS_NS, ids=ids)
@pytest.mark.parametrize("K", RC.KS_)
def test_exact_residual_and_ss_out(K, Ns, rows):
    RC.check_exact_residual_ss(B, rows, K, Ns)


@pytest.mark.parametrize("rows", RC.ROWS)
@pytest.mark.parametrize("Ns", RC.NSETS, ids=ids)
@pytest.mark.parametrize("K", RC.KS_)
def test_random_data_against_fp64(K, Ns, rows):
    RC.check_random(B, rows, K, Ns)


@pytest.mark.parametrize("n_ss", [1, 32, 64])
@pytest.mark.parametrize("rows", [5, 17, 32])
@pytest.mark.parametrize("K,Ns", [(160, (520,)), (384, (64, 1032))], ids=ids)
def test_norm_on_load(K, Ns, rows, n_ss):
    RC.check_norm(B, rows, K, Ns, n_ss)


@pytest.mark.parametrize("rows", RC.ROWS)
@pytest.mark.parametrize("Ns", RC.NSETS + RC.SS_NS, ids=ids)
@pytest.mark.parametrize("K", RC.KS_)
def test_packs_equal_the_bf16_entry_on_the_rounded_weights(K, Ns, rows):
    RC.check_packs(B, rows, K, Ns)


@pytest.mark.parametrize("K,Ns,fused", [(160, (520,), False), (384, (64, 1032), False), (384, (384,), True)], ids=ids)
def test_row_independence(K, Ns, fused):
    RC.check_row_independence(B, K, Ns, fused)


@pytest.mark.parametrize("w8", [False, True], ids=["bf16", "w8"])
@pytest.mark.parametrize("name", list(RC.REFUSALS))
def test_refusals_touch_nothing(name, w8):
    RC.check_refusal(B, w8, name)


@pytest.mark.parametrize("name", list(RC.W8_REFUSALS))
def test_w8_refusals_touch_nothing(name):
    RC.check_refusal(B, True, name)


@pytest.mark.parametrize("w8", [False, True], ids=["bf16", "w8"])
def test_the_unedited_arguments_are_accepted(w8):
    RC.check_accepted(B, w8)


# ---------------------------------------------------------------- the same table against lwm_gemv_fused_bf16 / _w8
@pytest.mark.parametrize("w8", [False, True], ids=["bf16", "w8"])
@pytest.mark.parametrize("name", list(RC.GEMV_REFUSALS))
def test_gemv_refusals_touch_nothing(name, w8):
    RC.check_refusal(B, w8, name, entry="gemv")


@pytest.mark.parametrize("name", list(RC.W8_REFUSALS))
def test_gemv_w8_refusals_touch_nothing(name):
    RC.check_refusal(B, True, name, entry="gemv")


@pytest.mark.parametrize("w8", [False, True], ids=["bf16", "w8"])
@pytest.mark.parametrize("name", ("rows 0",) + RC.GEMV_ACCEPTS)
def test_gemv_accepts_what_the_rows_entries_refuse(name, w8):
    RC.check_gemv_accepts(B, w8, name)


@pytest.mark.parametrize("w8", [False, True], ids=["bf16", "w8"])
def test_gemv_unedited_arguments_are_accepted(w8):
    RC.check_accepted(B, w8, entry="gemv")


def test_two_launches_give_the_same_bits():
    x, ws = RC.random_case(17, 384, (520, 64, 1032))
    a, b = RC.run(B, x, ws, want_f32=True), RC.run(B, x, ws, want_f32=True)
    assert RC.same(a, b) and np.array_equal(RC.bits(a["work"]), RC.bits(b["work"]))


def test_python_wrappers_agree_with_each_other():
    """llama_ops.gemm_rows_fused on a rounded kernel == w8.gemm_rows_fused_w8 on its pack; refusals by name"""
    import torch
    from lwm_amd import llama_ops as LO, w8
    torch.manual_seed(3)
    k = (torch.randn(384, 1152, device="cuda") * 0.1).to(torch.bfloat16)
    p = w8.quantise_weight(k)
    x = torch.randn(9, 384, device="cuda").to(torch.bfloat16)
    res = torch.randn(9, 1152, device="cuda").to(torch.bfloat16)
    (a,), sa = w8.gemm_rows_fused_w8(x, [p], residual=res, want_ss=True)
    (b,), sb = LO.gemm_rows_fused(x, [k], residual=res, want_ss=True)
    assert torch.equal(a, b) and torch.equal(sa, sb)
    (a,) = w8.gemm_rows_fused_w8(x, [p], out_dtype=torch.float32)
    (b,) = LO.gemm_rows_fused(x, [k], out_dtype=torch.float32)
    assert torch.equal(a, b)
    ref = x.double() @ k.double()
    assert ((b.double() - ref).abs() <= 384 * 2.0 ** -23 * (x.double().abs() @ k.double().abs())).all()
    with pytest.raises(ValueError, match="rows"):
        LO.gemm_rows_fused(torch.zeros(33, 384, device="cuda", dtype=torch.bfloat16), [k])
    with pytest.raises(ValueError, match="aligned"):
        LO.gemm_rows_fused(torch.zeros(9, 392, device="cuda", dtype=torch.bfloat16)[:, 4:388], [k])


# ---------------------------------------------------------------- models
CFG = dict(vocab_size=512, hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2,
           max_sequence_length=128)
NEW = 5


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


def _count(monkeypatch, obj, name):
    calls, real = [], getattr(obj, name)

    def counted(*a, **kw):
        calls.append(name)
        return real(*a, **kw)
    monkeypatch.setattr(obj, name, counted)
    return calls


@pytest.fixture(scope="module")
def text_model():
    import torch
    from lwm_amd.llama import LLaMAConfig, LLaMAForCausalLM
    torch.manual_seed(0)
    return _spread(LLaMAForCausalLM(LLaMAConfig(**CFG)).cuda())


@pytest.fixture(scope="module")
def prompts8():
    import torch
    g = torch.Generator().manual_seed(5)
    return torch.randint(3, 512, (8, 9), generator=g).cuda()


def _close(a, b):
    return bool(((a - b).abs() <= 2e-2 * b.abs().max()).all())


@pytest.mark.parametrize("kv_dtype", [None, "fp8"])
def test_generate_with_eight_rows(text_model, prompts8, kv_dtype, monkeypatch):
    import torch
    from lwm_amd import llama_ops as LO, w8
    model = text_model
    monkeypatch.delenv("LWM_DECODE_ROWS", raising=False)
    kw = dict(max_new_tokens=NEW, return_logits=True, kv_dtype=kv_dtype)
    model.decode_rows = None
    snap = {n: p.detach().clone() for n, p in model.named_parameters()}
    try:
        t_off, l_off = model.generate(prompts8, **kw)
        model.decode_rows = 8
        fused = _count(monkeypatch, type(model), "_decode_layers_fused")
        rows_calls = _count(monkeypatch, LO, "gemm_rows_fused")
        t_on, l_on = model.generate(prompts8, **kw)
        assert len(fused) == NEW - 1 and len(rows_calls) >= (NEW - 1) * (4 * 2 + 1)      # four launch pairs per layer and the head
        print("max |logits on - off| / max |logits off| =", float((l_on - l_off).abs().max() / l_off.abs().max()))
        assert _close(l_on, l_off)
        t_g, l_g = model.generate(prompts8, graph=True, **kw)
        assert torch.equal(t_g, t_on) and torch.equal(l_g, l_on)
        # the 8-bit packs: the rounded model through the packs == the rounded model streaming bf16
        model.quantize_decode_weights("fp8")
        n_rows = len(rows_calls)
        w8_calls = _count(monkeypatch, w8, "gemm_rows_fused_w8")
        got = [model.generate(prompts8, **kw), model.generate(prompts8, graph=True, **kw)]
        assert len(w8_calls) >= (NEW - 1) * (4 * 2 + 1) + (4 * 2 + 1) and len(rows_calls) == n_rows
        n_w8 = len(w8_calls)
        model.drop_decode_weights()
        ref = [model.generate(prompts8, **kw), model.generate(prompts8, graph=True, **kw)]
        assert len(w8_calls) == n_w8 and len(rows_calls) > n_rows
        for (tg, lg), (tr, lr) in zip(got, ref):
            assert torch.equal(tg, tr) and torch.equal(lg, lr) and torch.isfinite(lg).all()
        assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])
    finally:
        model.drop_decode_weights()
        model.decode_rows = None
        with torch.no_grad():
            for n, p in model.named_parameters():
                p.copy_(snap[n])


def test_batch_invariance(text_model, monkeypatch):
    """8 rows = 4 prompts, each twice: the duplicates get equal logits at every step"""
    import torch
    monkeypatch.delenv("LWM_DECODE_ROWS", raising=False)
    g = torch.Generator().manual_seed(9)
    four = torch.randint(3, 512, (4, 7), generator=g).cuda()
    ids8 = torch.cat([four, four.flip(0)], 0)
    text_model.decode_rows = 8
    try:
        for kw in (dict(), dict(graph=True), dict(kv_dtype="fp8")):
            t, l = text_model.generate(ids8, max_new_tokens=NEW, return_logits=True, **kw)
            assert torch.equal(l[:4], l[4:].flip(0)) and torch.equal(t[:4], t[4:].flip(0)), kw
    finally:
        text_model.decode_rows = None


def test_a_prompt_decodes_alike_in_a_batch_of_5_and_of_32(text_model, monkeypatch):
    import torch
    monkeypatch.delenv("LWM_DECODE_ROWS", raising=False)
    g = torch.Generator().manual_seed(10)
    ids32 = torch.randint(3, 512, (32, 7), generator=g).cuda()
    text_model.decode_rows = 32
    try:
        _, l32 = text_model.generate(ids32, max_new_tokens=3, return_logits=True)
        _, l5 = text_model.generate(ids32[20:25], max_new_tokens=3, return_logits=True)
        assert torch.equal(l5[:, 1:], l32[20:25, 1:])           # (step 0 is the prefill: library GEMMs over all tokens)
    finally:
        text_model.decode_rows = None


@pytest.fixture(scope="module")
def vision_model():
    import torch
    from lwm_amd.vision_llama import VideoLLaMAConfig, VideoLLaMAForCausalLM
    torch.manual_seed(0)
    return _spread(VideoLLaMAForCausalLM(VideoLLaMAConfig(**CFG, sample_mode="vision")).cuda())


def test_vision_model(vision_model, monkeypatch):
    import torch
    from lwm_amd import llama_ops as LO
    model = vision_model
    monkeypatch.delenv("LWM_DECODE_ROWS", raising=False)
    g = torch.Generator().manual_seed(6)
    cond = torch.randint(3, 512, (3, 7), generator=g).cuda()
    ids = torch.cat([cond, torch.full_like(cond, 1)], 0)           # three prompts: conditional + unconditional = 6 rows
    kw = dict(cfg_scales=[3.0, 2.0, 1.5], max_new_tokens=NEW, temperature=0.8, top_k=40, seed=11, return_logits=True)
    fused = _count(monkeypatch, type(model), "_decode_layers_fused")
    try:
        model.cfg.sample_mode = "vision"
        model.decode_rows = None
        t_off, l_off = model.generate_vision(ids, **kw)
        assert not fused                                           # option unset: block by block, as before
        model.decode_rows = 8
        rows_calls = _count(monkeypatch, LO, "gemm_rows_fused")
        t_on, l_on = model.generate_vision(ids, **kw)
        assert len(fused) == NEW - 1 and len(rows_calls) >= (NEW - 1) * (4 * 2 + 1) and l_on.shape[:2] == (6, NEW)
        n_fused = len(fused)
        t_g, l_g = model.generate_vision(ids, graph=True, **kw)
        assert len(fused) > n_fused
        assert torch.equal(t_g, t_on) and torch.equal(l_g, l_on)
        print("vision max |logits on - off| / max |logits off| =", float((l_on - l_off).abs().max() / l_off.abs().max()))
        assert _close(l_on, l_off)
        # text continuation at two rows: the fused step too (the GEMV: <= 4 rows)
        model.cfg.sample_mode = "text"
        n_fused, n_rows = len(fused), len(rows_calls)
        out = model.generate(ids[:2], max_new_tokens=3)
        assert len(fused) == n_fused + 2 and len(rows_calls) == n_rows and out.shape == (2, 3)
    finally:
        model.cfg.sample_mode = "vision"
        model.decode_rows = None


def test_option_unset_changes_nothing(text_model, vision_model, monkeypatch):
    import torch
    from lwm_amd import llama_ops as LO
    monkeypatch.delenv("LWM_DECODE_ROWS", raising=False)
    assert text_model.decode_rows is None and LO.decode_rows_limit() is None
    x5 = torch.zeros(5, 1, 256, dtype=torch.bfloat16, device="cuda")
    with torch.no_grad():
        assert text_model._fused_decode_ok(x5[:4], 1) and not text_model._fused_decode_ok(x5, 1)
        rows_calls = _count(monkeypatch, LO, "gemm_rows_fused")
        k = torch.zeros(256, 64, dtype=torch.bfloat16, device="cuda")
        LO.dense(x5, k)
        assert not rows_calls
        monkeypatch.setenv("LWM_DECODE_ROWS", "6")
        assert text_model.decode_rows == 6 and vision_model.decode_rows == 6
        assert text_model._fused_decode_ok(x5, 1) and not text_model._fused_decode_ok(torch.cat([x5, x5[:2]]), 1)
        LO.dense(x5, k)
        assert len(rows_calls) == 1
        text_model.decode_rows = 9                                  # the attribute wins over the environment
        assert text_model.decode_rows == 9
        text_model.decode_rows = None
    for bad in ("4", "33", "0", "-7", "many", "5.5"):
        monkeypatch.setenv("LWM_DECODE_ROWS", bad)
        with pytest.raises(ValueError, match="LWM_DECODE_ROWS"):
            text_model.decode_rows
        with pytest.raises(ValueError, match="LWM_DECODE_ROWS"):
            LO.dense(x5, k)
    monkeypatch.delenv("LWM_DECODE_ROWS")
    for bad in (4, 33, "x", 6.5):
        with pytest.raises(ValueError, match="decode_rows"):
            text_model.decode_rows = bad
    assert text_model.decode_rows is None


def test_refused_by_name(monkeypatch):
    """a float32 model never takes the fused step, whatever decode_rows says"""
    import torch
    from lwm_amd.llama import LLaMAConfig, LLaMAForCausalLM
    monkeypatch.delenv("LWM_DECODE_ROWS", raising=False)
    f32 = LLaMAForCausalLM(LLaMAConfig(**CFG), torch.float32).cuda()
    f32.decode_rows = 8
    with torch.no_grad():
        assert not f32._fused_decode_ok(torch.zeros(8, 1, 256, device="cuda"), 1)
        assert not f32._fused_decode_ok(torch.zeros(8, 1, 256, device="cuda", dtype=torch.bfloat16), 2)      # sp > 1
    with pytest.raises(NotImplementedError, match="float32 model"):
        f32.quantize_decode_weights("fp8")
