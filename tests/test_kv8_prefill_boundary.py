"""The operator boundary of lwm_amd.kv8.attn_prefill_kv8 on the CPU (the contract of tests/test_op_boundary.py for the
wrapper of the new module): under a tripwire library nothing a check should have stopped reaches the C ABI; and the
parsing of LWM_PREFILL_CHUNK in the entry points' sampler_kwargs."""
import contextlib

import pytest
import torch

from tests import _boundary as BD, _emu

B, Sq, Sk, H, D = 2, 3, 19, 2, 128
u8, f32, bf16 = torch.uint8, torch.float32, torch.bfloat16


@contextlib.contextmanager
def tripwire():
    """lwm_amd.kv8.lib replaced by the Tripwire of tests/_boundary.py, the way tripwire() there does it for ops"""
    from lwm_amd import kv8
    with BD.tripwire(_emu.lib()) as wire:
        saved = kv8.lib
        kv8.lib = lambda: wire
        try:
            yield wire
        finally:
            kv8.lib = saved


def make(dev="cpu"):
    g = torch.Generator().manual_seed(0)
    kv = torch.ones(B, Sk, dtype=u8)
    kv[0, :4] = 0
    return dict(q=torch.randn(B, Sq, H, D, generator=g).to(bf16).to(dev),
                cached_key=torch.full((B, Sk, H, D), 0x38, dtype=u8).to(dev), key_scale=torch.ones(B, Sk, H).to(dev),
                cached_value=torch.full((B, Sk, H, D), 0x38, dtype=u8).to(dev), value_scale=torch.ones(B, Sk, H).to(dev),
                key_valid=kv.to(dev), q_start=Sk - Sq, k_splits=2)


class Dev:
    """A stand-in that says it lives on a device: the wrapper's checks read attributes only, so every defect below is
    exercised with the device check out of the way -- and still nothing may reach the library"""

    def __init__(self, t):
        self._t = t

    is_cuda = True

    def __getattr__(self, n):
        return getattr(self._t, n)


def test_host_tensors_are_refused_before_the_library():
    from lwm_amd import kv8
    with tripwire() as wire:
        with pytest.raises(ValueError):
            kv8.attn_prefill_kv8(**make())
        assert wire.reached == []


DEFECTS = {
    "cached_key of another dtype": BD.cast("cached_key", torch.int8),
    "cached_value bf16": BD.cast("cached_value", bf16),
    "key_scale float64": BD.cast("key_scale", torch.float64),
    "value_scale bf16": BD.cast("value_scale", bf16),
    "cached_key of another length": BD.reshaped("cached_key", (B, Sk + 1, H, D)),
    "cached_value of another head count": BD.reshaped("cached_value", (B, Sk, H + 1, D)),
    "cached_value of another batch": BD.reshaped("cached_value", (B + 1, Sk, H, D)),
    "key_scale of another head count": BD.reshaped("key_scale", (B, Sk, H + 1)),
    "value_scale of another length": BD.reshaped("value_scale", (B, Sk - 1, H)),
    "cached_key with a strided inner dimension": lambda kw, dev: kw.update(cached_key=torch.zeros(B, Sk, H, 2 * D, dtype=u8)[..., ::2]),
    "value_scale with strided heads": lambda kw, dev: kw.update(value_scale=torch.ones(B, Sk, 2 * H)[..., ::2]),
    "q with a strided inner dimension": lambda kw, dev: kw.update(q=torch.zeros(B, Sq, H, 2 * D, dtype=bf16)[..., ::2]),
    "key_valid of another length": BD.reshaped("key_valid", (B, Sk + 8)),
    "key_valid (B, 1, Sk)": BD.reshaped("key_valid", (B, 1, Sk)),
    "key_valid int32": BD.cast("key_valid", torch.int32),
    "key_valid with strided keys": lambda kw, dev: kw.update(key_valid=torch.ones(B, 2 * Sk, dtype=u8)[:, ::2]),
    "an f32 query": BD.cast("q", f32),
    "head_dim 64": lambda kw, dev: kw.update(q=kw["q"][..., :64].contiguous()),
    "q_start < 0": lambda kw, dev: kw.update(q_start=-1),
    "k_splits beyond 4096": lambda kw, dev: kw.update(k_splits=5000),
}


@pytest.mark.parametrize("name", list(DEFECTS))
def test_each_defect_is_refused_on_its_own(name):
    """every tensor claims to be on a device, so the one edit is the only defect of the call"""
    from lwm_amd import kv8
    kw = make()
    DEFECTS[name](kw, "cpu")
    kw = {k: Dev(v) if torch.is_tensor(v) else v for k, v in kw.items()}
    with tripwire() as wire, pytest.MonkeyPatch.context() as mp:
        mp.setattr(torch, "is_tensor", lambda t: isinstance(t, (torch.Tensor, Dev)))
        with pytest.raises(ValueError):
            kv8.attn_prefill_kv8(**kw)
        assert wire.reached == []


def test_the_well_formed_call_passes_every_check():
    """... and the table above is not vacuous: with the stand-in devices the unedited call gets as far as the library"""
    from lwm_amd import kv8
    kw = {k: Dev(v) if torch.is_tensor(v) else v for k, v in make().items()}
    with tripwire() as wire, pytest.MonkeyPatch.context() as mp:
        mp.setattr(torch, "is_tensor", lambda t: isinstance(t, (torch.Tensor, Dev)))
        mp.setattr(torch, "empty", lambda *a, device=None, **k: torch.zeros(*a, **k))
        with pytest.raises(AssertionError, match="reached the C library: lwm_attn_prefill_kv8"):
            kv8.attn_prefill_kv8(**kw)
        assert wire.reached == ["lwm_attn_prefill_kv8"]


# ---------------------------------------------------------------- the entry points' environment switch
class _Model:
    dtype = bf16


def test_sampler_kwargs_prefill_chunk(monkeypatch):
    from lwm_amd.cli import _common
    for v in ("LWM_PREFILL_CHUNK", "LWM_KV_CACHE", "LWM_DECODE_GRAPH"):
        monkeypatch.delenv(v, raising=False)
    gen = object()
    assert _common.sampler_kwargs(_Model(), 7, gen) == dict(generator=gen)          # unset: the dict as it was
    monkeypatch.setenv("LWM_PREFILL_CHUNK", "")
    assert _common.sampler_kwargs(_Model(), 7, gen) == dict(generator=gen)
    monkeypatch.setenv("LWM_PREFILL_CHUNK", "8192")
    assert _common.sampler_kwargs(_Model(), 7, gen) == dict(generator=gen, prefill_chunk=8192)
    monkeypatch.setenv("LWM_KV_CACHE", "fp8")
    monkeypatch.setenv("LWM_DECODE_GRAPH", "1")
    assert _common.sampler_kwargs(_Model(), 7, gen) == dict(seed=7, graph=True, kv_dtype="fp8", prefill_chunk=8192)
    for bad in ("0", "-4", "4k", "1.5"):
        monkeypatch.setenv("LWM_PREFILL_CHUNK", bad)
        with pytest.raises(SystemExit, match="LWM_PREFILL_CHUNK"):
            _common.sampler_kwargs(_Model(), 7, gen)
