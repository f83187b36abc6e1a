"""The operator boundary of lwm_amd.kv6 on the CPU (the contract of tests/test_kv8_prefill_boundary.py for the four
front-end functions of the 6-bit cache): under a tripwire library a bad dtype, shape, device or stride raises ValueError
before the C ABI is reached, and a well-formed call reaches exactly the named entry point; and the parsing of
LWM_KV_CACHE=fp6 in the entry points' sampler_kwargs, with and without LWM_PREFILL_CHUNK."""
import contextlib

import pytest
import torch

from tests import _boundary as BD, _emu

B, Sq, Sk, H, D = 2, 3, 19, 2, 128
u8, f32, bf16 = torch.uint8, torch.float32, torch.bfloat16


@contextlib.contextmanager
def tripwire():
    """lwm_amd.ops.lib (the writes and the decode go through it) and lwm_amd.kv6.lib replaced by the Tripwire of
    tests/_boundary.py"""
    from lwm_amd import kv6
    with BD.tripwire(_emu.lib()) as wire:
        saved = kv6.lib
        kv6.lib = lambda: wire
        try:
            yield wire
        finally:
            kv6.lib = saved


def _cache(rows):
    return dict(c=torch.full((B, rows, H, 96), 0x38, dtype=u8), s=torch.full((B, rows, H, 4), 127, dtype=u8))


def make_prefill():
    g = torch.Generator().manual_seed(0)
    kv = torch.ones(B, Sk, dtype=u8)
    kv[0, :4] = 0
    k, v = _cache(Sk), _cache(Sk)
    return dict(q=torch.randn(B, Sq, H, D, generator=g).to(bf16), cached_key=k["c"], key_scale=k["s"], cached_value=v["c"],
                value_scale=v["s"], key_valid=kv, q_start=Sk - Sq, k_splits=2)


def make_decode():
    g = torch.Generator().manual_seed(0)
    k, v = _cache(Sk), _cache(Sk)
    return dict(q=torch.randn(B, 1, H, D, generator=g).to(bf16), cached_key=k["c"], key_scale=k["s"], cached_value=v["c"],
                value_scale=v["s"], dense_mask=torch.ones(B, 1, Sk, dtype=u8), k_splits=2)


def make_write():
    g = torch.Generator().manual_seed(0)
    k = _cache(Sk)
    return dict(cache=k["c"], scale=k["s"], src=torch.randn(B, 5, H, D, generator=g).to(bf16), dst_row0=3)


def make_write_at():
    kw = make_write()
    del kw["dst_row0"]
    return dict(kw, index_dev=torch.tensor([3], dtype=torch.int32))


class Dev:
    """A stand-in that says it lives on a device: the wrappers' checks read attributes (and rows) only, so every defect
    below is exercised with the device check out of the way -- and still nothing may reach the library"""

    def __init__(self, t):
        self._t = t

    is_cuda = True

    def __getattr__(self, n):
        return getattr(self._t, n)

    def __getitem__(self, i):
        return Dev(self._t[i])


def _fn(name):
    from lwm_amd import kv6
    return getattr(kv6, name)


strided = lambda name, shape, dtype: (lambda kw, dev: kw.update({name: torch.zeros(*shape[:-1], 2 * shape[-1], dtype=dtype)[..., ::2]}))

CACHE_DEFECTS = {
    "cached_key of another dtype": BD.cast("cached_key", torch.int8),
    "cached_value bf16": BD.cast("cached_value", bf16),
    "key_scale f32": BD.cast("key_scale", f32),
    "value_scale int8": BD.cast("value_scale", torch.int8),
    "cached_key with the 4-bit cache's 64-byte heads": BD.reshaped("cached_key", (B, Sk, H, 64)),
    "cached_key with the 8-bit cache's 128-byte heads": BD.reshaped("cached_key", (B, Sk, H, 128)),
    "cached_value of another head count": BD.reshaped("cached_value", (B, Sk, H + 1, 96)),
    "cached_value of another batch": BD.reshaped("cached_value", (B + 1, Sk, H, 96)),
    "cached_value of another length": BD.reshaped("cached_value", (B, Sk + 1, H, 96)),
    "key_scale of the 8-bit cache's shape": BD.reshaped("key_scale", (B, Sk, H)),
    "value_scale of another length": BD.reshaped("value_scale", (B, Sk - 1, H, 4)),
    "cached_key with a strided inner dimension": strided("cached_key", (B, Sk, H, 96), u8),
    "value_scale with strided bytes": strided("value_scale", (B, Sk, H, 4), u8),
    "an f32 query": BD.cast("q", f32),
    "head_dim 64": lambda kw, dev: kw.update(q=kw["q"][..., :64].contiguous()),
    "k_splits beyond 4096": lambda kw, dev: kw.update(k_splits=5000),
}
WRITE_DEFECTS = {
    "cache of another dtype": BD.cast("cache", torch.int8),
    "cache with 64-byte heads": BD.reshaped("cache", (B, Sk, H, 64)),
    "cache with strided rows": lambda kw, dev: kw.update(cache=torch.zeros(B, 2 * Sk, H, 96, dtype=u8)[:, ::2]),
    "scale f32": BD.cast("scale", f32),
    "scale of the 8-bit cache's shape": BD.reshaped("scale", (B, Sk, H)),
    "an f32 source": BD.cast("src", f32),
    "a source of another head count": BD.reshaped("src", (B, 5, H + 1, D)),
    "a source of head_dim 64": BD.reshaped("src", (B, 5, H, 64)),
    "a source of another batch": BD.reshaped("src", (B + 1, 5, H, D)),
    "more source rows than there are": lambda kw, dev: kw.update(src_row0=2, nrows=4),
}
TABLE = {
    "attn_prefill_kv6": (make_prefill, "lwm_attn_prefill_kv6", {
        **CACHE_DEFECTS,
        "q with a strided inner dimension": strided("q", (B, Sq, H, D), bf16),
        "key_valid of another length": BD.reshaped("key_valid", (B, Sk + 8)),
        "key_valid (B, 1, Sk)": BD.reshaped("key_valid", (B, 1, Sk)),
        "key_valid int32": BD.cast("key_valid", torch.int32),
        "key_valid with strided keys": lambda kw, dev: kw.update(key_valid=torch.ones(B, 2 * Sk, dtype=u8)[:, ::2]),
        "q_start < 0": lambda kw, dev: kw.update(q_start=-1),
    }),
    "attn_decode_kv6": (make_decode, "lwm_attn_decode_kv6", {
        **CACHE_DEFECTS,
        "a block of queries": lambda kw, dev: kw.update(q=torch.zeros(B, 2, H, D, dtype=bf16)),
        "dense_mask (B, Sk)": BD.reshaped("dense_mask", (B, Sk)),
        "dense_mask int32": BD.cast("dense_mask", torch.int32),
        "dense_mask with strided keys": lambda kw, dev: kw.update(dense_mask=torch.ones(B, 1, 2 * Sk, dtype=u8)[..., ::2]),
    }),
    "kv6_cache_write": (make_write, "lwm_kv6_cache_write", {
        **WRITE_DEFECTS,
        "a destination past the cache": lambda kw, dev: kw.update(dst_row0=Sk - 2),
        "a negative destination": lambda kw, dev: kw.update(dst_row0=-1),
    }),
    "kv6_cache_write_at": (make_write_at, "lwm_kv6_cache_write_at", {
        **WRITE_DEFECTS,
        "an int64 index": BD.cast("index_dev", torch.int64),
        "an index of two elements": BD.reshaped("index_dev", (2,)),
    }),
}
ROWS = [(fn, name) for fn, (_, _, defects) in TABLE.items() for name in defects]


@pytest.mark.parametrize("fn", list(TABLE))
def test_host_tensors_are_refused_before_the_library(fn):
    make, _, _ = TABLE[fn]
    with tripwire() as wire:
        with pytest.raises(ValueError):
            _fn(fn)(**make())
        assert wire.reached == []


@pytest.mark.parametrize("fn,name", ROWS, ids=[f"{fn}-{name}" for fn, name in ROWS])
def test_each_defect_is_refused_on_its_own(fn, name):
    """every tensor claims to be on a device, so the one edit is the only defect of the call"""
    make, _, defects = TABLE[fn]
    kw = make()
    defects[name](kw, "cpu")
    kw = {k: Dev(v) if torch.is_tensor(v) else v for k, v in kw.items()}
    with tripwire() as wire, pytest.MonkeyPatch.context() as mp:
        mp.setattr(torch, "is_tensor", lambda t: isinstance(t, (torch.Tensor, Dev)))
        with pytest.raises(ValueError):
            _fn(fn)(**kw)
        assert wire.reached == []


@pytest.mark.parametrize("fn", list(TABLE))
def test_the_well_formed_call_reaches_exactly_its_entry_point(fn):
    """... and the tables above are not vacuous: with the stand-in devices the unedited call gets as far as the library"""
    make, entry, _ = TABLE[fn]
    kw = {k: Dev(v) if torch.is_tensor(v) else v for k, v in make().items()}
    with tripwire() as wire, pytest.MonkeyPatch.context() as mp:
        mp.setattr(torch, "is_tensor", lambda t: isinstance(t, (torch.Tensor, Dev)))
        mp.setattr(torch, "empty", lambda *a, device=None, **k: torch.zeros(*a, **k))
        with pytest.raises(AssertionError, match=f"reached the C library: {entry}$"):
            _fn(fn)(**kw)
        assert wire.reached == [entry]


def test_the_format_names_its_block_function():
    from lwm_amd import kv4, kv6, kv8, ops
    assert ops._kvq_block_fn(kv6.KV6) is kv6.attn_prefill_kv6
    assert ops._kvq_block_fn(ops.KV8) is kv8.attn_prefill_kv8            # the default of the trailing field
    with pytest.raises(NotImplementedError, match="block kernel over the 4-bit cache is not built"):
        ops._kvq_block_fn(kv4.KV4)
    assert (kv6.KV6.head_bytes, kv6.KV6.kv_dtype, kv6.KV6.scale_keys) == (96, "fp6", kv4.KV4.scale_keys)


# ---------------------------------------------------------------- the entry points' environment switch
class _Model:
    dtype = bf16


def test_sampler_kwargs_fp6(monkeypatch):
    from lwm_amd.cli import _common
    from lwm_amd.llama import cache_kwargs
    for v in ("LWM_PREFILL_CHUNK", "LWM_KV_CACHE", "LWM_DECODE_GRAPH", "LWM_TOP_P"):
        monkeypatch.delenv(v, raising=False)
    gen = object()
    monkeypatch.setenv("LWM_KV_CACHE", "fp6")
    assert _common.sampler_kwargs(_Model(), 7, gen) == dict(generator=gen, kv_dtype="fp6")
    monkeypatch.setenv("LWM_KV_CACHE", "FP6")
    assert _common.sampler_kwargs(_Model(), 7, gen) == dict(generator=gen, kv_dtype="fp6")
    monkeypatch.setenv("LWM_PREFILL_CHUNK", "8192")
    assert _common.sampler_kwargs(_Model(), 7, gen) == dict(generator=gen, kv_dtype="fp6", prefill_chunk=8192)
    monkeypatch.setenv("LWM_DECODE_GRAPH", "1")
    assert _common.sampler_kwargs(_Model(), 7, gen) == dict(seed=7, graph=True, kv_dtype="fp6", prefill_chunk=8192)
    monkeypatch.delenv("LWM_PREFILL_CHUNK")
    assert _common.sampler_kwargs(_Model(), 7, gen) == dict(seed=7, graph=True, kv_dtype="fp6")
    monkeypatch.setenv("LWM_KV_CACHE", "fp5")
    with pytest.raises(SystemExit, match="'fp6', 'fp4', 'fp8', 'bf16'"):
        _common.sampler_kwargs(_Model(), 7, gen)
    # what generate() hands init_cache
    assert cache_kwargs("fp6") == dict(kv_dtype="fp6")
    assert cache_kwargs("fp6", 8192) == dict(kv_dtype="fp6", chunked_prefill=True)
    assert cache_kwargs(None, 8192) == {}
