"""The operator boundary of lwm_amd.w8 on the CPU (the contract of tests/test_op_boundary.py for the wrappers of the new
module): under a tripwire library nothing a check should have stopped reaches the C ABI; the parsing of LWM_DECODE_WEIGHTS;
and the refusals of quantize_decode_weights that need no device."""
import contextlib

import pytest
import torch

from tests import _boundary as BD, _emu

R, K, N = 2, 160, 48
u8, f32, bf16 = torch.uint8, torch.float32, torch.bfloat16


@contextlib.contextmanager
def tripwire():
    """lwm_amd.w8.lib replaced by the Tripwire of tests/_boundary.py, the way tripwire() there does it for ops"""
    from lwm_amd import w8
    with BD.tripwire(_emu.lib()) as wire:
        saved = w8.lib
        w8.lib = lambda: wire
        try:
            yield wire
        finally:
            w8.lib = saved


class Dev:
    """A stand-in that says it lives on a device: the wrappers' checks read attributes only, so every defect below is
    exercised with the device check out of the way -- and still nothing may reach the library"""

    def __init__(self, t):
        self._t = t

    is_cuda = True

    def __getattr__(self, n):
        return getattr(self._t, n)


def _dev(v):
    from lwm_amd.w8 import W8Kernel
    if torch.is_tensor(v):
        return Dev(v)
    if isinstance(v, W8Kernel):
        return W8Kernel(_dev(v.q), _dev(v.scale), v.shape, v.stamp)
    if isinstance(v, (list, tuple)):
        return type(v)(_dev(e) for e in v)
    return v


def pack(k=K, n=N):
    from lwm_amd.w8 import W8Kernel
    return W8Kernel(torch.full((k, n), 0x38, dtype=u8), torch.ones((k + 127) // 128, n), (k, n), (0, 0))


def make():
    g = torch.Generator().manual_seed(0)
    return dict(x=torch.randn(R, K, generator=g).to(bf16), packs=[pack()])


def make_full():
    kw = make()
    kw["packs"] = [pack(K, 128)]
    kw.update(norm=(torch.ones(R, 4), torch.ones(K, dtype=bf16), 1e-6), residual=torch.zeros(R, 128, dtype=bf16), want_ss=True)
    return kw


def _pack_edit(**fields):
    def edit(kw, dev):
        p = kw["packs"][0]
        for k, f in fields.items():
            setattr(p, k, f(getattr(p, k)))
    return edit


def _norm_edit(i, f):
    def edit(kw, dev):
        n = list(kw["norm"])
        n[i] = f(n[i])
        kw["norm"] = tuple(n)
    return edit


GEMV_DEFECTS = {
    "x f32": BD.cast("x", f32),
    "x of three dimensions": BD.reshaped("x", (1, R, K)),
    "x with a strided inner dimension": lambda kw, dev: kw.update(x=torch.zeros(R, 2 * K, dtype=bf16)[:, ::2]),
    "x of another K": BD.reshaped("x", (R, K + 32)),
    "no packs": lambda kw, dev: kw.update(packs=[]),
    "four packs": lambda kw, dev: kw.update(packs=[pack() for _ in range(4)]),
    "a bf16 tensor instead of a pack": lambda kw, dev: kw.update(packs=[torch.zeros(K, N, dtype=bf16)]),
    "bytes int8": _pack_edit(q=lambda t: t.to(torch.int8)),
    "bytes bf16": _pack_edit(q=lambda t: t.to(bf16)),
    "bytes of another shape": _pack_edit(q=lambda t: torch.zeros(K, N + 16, dtype=u8)),
    "bytes transposed": _pack_edit(q=lambda t: torch.zeros(N, K, dtype=u8).t()),
    "scales f64": _pack_edit(scale=lambda t: t.double()),
    "scales of one group too few": _pack_edit(scale=lambda t: t[:1]),
    "scales strided": _pack_edit(scale=lambda t: torch.ones(2, 2 * N)[:, ::2]),
    "out_dtype f16": lambda kw, dev: kw.update(out_dtype=torch.float16),
}
FULL_DEFECTS = {
    "norm ss f64": _norm_edit(0, lambda t: t.double()),
    "norm ss of another row count": _norm_edit(0, lambda t: torch.ones(R + 1, 4)),
    "norm ss with 65 partials": _norm_edit(0, lambda t: torch.ones(R, 65)),
    "norm ss strided": _norm_edit(0, lambda t: torch.ones(R, 8)[:, ::2]),
    "norm weight f32": _norm_edit(1, lambda t: t.float()),
    "norm weight of another length": _norm_edit(1, lambda t: torch.ones(K + 1, dtype=bf16)),
    "residual f32": BD.cast("residual", f32),
    "residual of another shape": BD.reshaped("residual", (R, 64)),
    "residual with a strided inner dimension": lambda kw, dev: kw.update(residual=torch.zeros(R, 256, dtype=bf16)[:, ::2]),
    "residual with two packs": lambda kw, dev: kw.update(packs=[pack(K, 128), pack(K, 128)], want_ss=False),
    "want_ss with an f32 output": lambda kw, dev: kw.update(out_dtype=f32, residual=None),
    "want_ss with N % 128": lambda kw, dev: kw.update(packs=[pack(K, 48)], residual=None),
}
QUANT_DEFECTS = {
    "an f32 kernel": lambda t: t.float(),
    "a uint8 kernel": lambda t: t.to(u8),
    "a kernel of three dimensions": lambda t: t[None],
    "a transposed kernel": lambda t: torch.zeros(N, K, dtype=bf16).t(),
    "K % 32": lambda t: torch.zeros(K + 16, N, dtype=bf16),
    "K > 12288": lambda t: torch.zeros(12320, 16, dtype=bf16),
    "N % 8": lambda t: torch.zeros(K, N + 4, dtype=bf16),
    "an empty kernel": lambda t: torch.zeros(0, N, dtype=bf16),
}


@contextlib.contextmanager
def standin_devices():
    with tripwire() as wire, pytest.MonkeyPatch.context() as mp:
        mp.setattr(torch, "is_tensor", lambda t: isinstance(t, (torch.Tensor, Dev)))
        mp.setattr(torch, "empty", lambda *a, device=None, **k: torch.zeros(*a, **k))
        yield wire


def test_host_tensors_are_refused_before_the_library():
    from lwm_amd import w8
    with tripwire() as wire:
        for kw in (make(), make_full()):
            with pytest.raises(ValueError):
                w8.gemv_fused_w8(**kw)
        with pytest.raises(ValueError):
            w8.quantise_weight(torch.zeros(K, N, dtype=bf16))
        assert wire.reached == []


@pytest.mark.parametrize("name", list(GEMV_DEFECTS) + list(FULL_DEFECTS))
def test_each_gemv_defect_is_refused_on_its_own(name):
    """every tensor claims to be on a device, so the one edit is the only defect of the call"""
    from lwm_amd import w8
    kw, edit = (make(), GEMV_DEFECTS[name]) if name in GEMV_DEFECTS else (make_full(), FULL_DEFECTS[name])
    edit(kw, "cpu")
    kw = {k: _dev(v) for k, v in kw.items()}
    with standin_devices() as wire:
        with pytest.raises(ValueError):
            w8.gemv_fused_w8(**kw)
        assert wire.reached == []


@pytest.mark.parametrize("name", list(QUANT_DEFECTS))
def test_each_quantiser_defect_is_refused_on_its_own(name):
    from lwm_amd import w8
    k = Dev(QUANT_DEFECTS[name](torch.zeros(K, N, dtype=bf16)))
    with standin_devices() as wire:
        with pytest.raises(ValueError):
            w8.quantise_weight(k)
        assert wire.reached == []


def test_the_well_formed_calls_pass_every_check():
    """... and the tables above are not vacuous: with the stand-in devices the unedited calls get as far as the library"""
    from lwm_amd import w8
    for kw in (make(), make_full()):
        kw = {k: _dev(v) for k, v in kw.items()}
        with standin_devices() as wire:
            with pytest.raises(AssertionError, match="reached the C library: lwm_gemv_fused_w8"):
                w8.gemv_fused_w8(**kw)
            assert wire.reached == ["lwm_gemv_fused_w8"]
    with standin_devices() as wire:
        with pytest.raises(AssertionError, match="reached the C library: lwm_w8_quantise"):
            w8.quantise_weight(Dev(torch.zeros(K, N, dtype=bf16)))
        assert wire.reached == ["lwm_w8_quantise"]


def test_a_stale_pack_names_its_parameter():
    from lwm_amd.w8 import W8Kernel
    w = torch.zeros(32, 16, dtype=bf16)
    p = W8Kernel(None, None, (32, 16), (w._version, w.data_ptr()))
    assert p.check(w, "h.0.attention.wq") is p
    w.add_(1)
    with pytest.raises(RuntimeError, match=r"h\.0\.attention\.wq.*quantize_decode_weights"):
        p.check(w, "h.0.attention.wq")
    with pytest.raises(RuntimeError, match="lm_head"):
        p.check(w.clone(), "lm_head")                 # another tensor at another address


# ---------------------------------------------------------------- the model's refusals that need no device
def _tiny(dtype):
    from lwm_amd.llama import LLaMAConfig, LLaMAForCausalLM
    cfg = LLaMAConfig(vocab_size=272, hidden_size=256, intermediate_size=352, num_hidden_layers=1, num_attention_heads=2,
                      max_sequence_length=64)
    return LLaMAForCausalLM(cfg, dtype)


def test_model_refusals_by_name():
    m = _tiny(f32)
    with pytest.raises(NotImplementedError, match="float32 model"):
        m.quantize_decode_weights("fp8")
    m = _tiny(bf16)
    with pytest.raises(ValueError, match="int4"):
        m.quantize_decode_weights("int4")
    with tripwire() as wire:
        with pytest.raises(ValueError, match=r"h\.0\.attention\.wq"):       # host parameters: no CPU path, named
            m.quantize_decode_weights("fp8")
        assert wire.reached == []
    assert m.decode_packs("fp8") is None and m.quantize_decode_weights("bf16") is m and m.drop_decode_weights() is m


def test_sp_ring_is_refused_by_name(monkeypatch):
    from lwm_amd import llama
    m = _tiny(bf16)
    monkeypatch.setattr(llama, "sp_size_rank", lambda axis: (2, 0))
    with pytest.raises(NotImplementedError, match="sp > 1"):
        m.quantize_decode_weights("fp8")


# ---------------------------------------------------------------- the entry points' environment switch
class _Model:
    def __init__(self):
        self.calls = []

    def quantize_decode_weights(self, mode):
        self.calls.append(mode)


def test_apply_decode_weights(monkeypatch):
    from lwm_amd.cli import _common
    monkeypatch.delenv("LWM_DECODE_WEIGHTS", raising=False)
    m = _Model()
    assert _common.apply_decode_weights(m) is m and m.calls == []
    for v in ("", "bf16", "BF16"):
        monkeypatch.setenv("LWM_DECODE_WEIGHTS", v)
        _common.apply_decode_weights(m)
    assert m.calls == []
    for v in ("fp8", "FP8"):
        monkeypatch.setenv("LWM_DECODE_WEIGHTS", v)
        _common.apply_decode_weights(m)
    assert m.calls == ["fp8", "fp8"]
    for bad in ("bogus", "int8", "1"):
        monkeypatch.setenv("LWM_DECODE_WEIGHTS", bad)
        with pytest.raises(SystemExit, match="LWM_DECODE_WEIGHTS"):
            _common.apply_decode_weights(m)
    assert m.calls == ["fp8", "fp8"]
