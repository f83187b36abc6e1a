"""The operator boundary of lwm_amd.w6 on the CPU (the contract of tests/test_w8_boundary.py for the 6-bit wrappers, the GEMV's
and the rows entry's): under a tripwire library nothing a check should have stopped reaches the C ABI; w6_dequant as the
written-down layout; the parsing of LWM_DECODE_WEIGHTS=fp6; and the refusals of quantize_decode_weights("fp6") that need no
device."""
import contextlib

import pytest
import torch

from tests import _boundary as BD, _emu, _w6_ref as W6
from tests.test_w8_boundary import Dev, _Model, _tiny

R, K, N = 2, 160, 48
u8, f32, bf16 = torch.uint8, torch.float32, torch.bfloat16


@contextlib.contextmanager
def tripwire():
    """lwm_amd.w6.lib replaced by the Tripwire of tests/_boundary.py"""
    from lwm_amd import w6
    with BD.tripwire(_emu.lib()) as wire:
        saved = w6.lib
        w6.lib = lambda: wire
        try:
            yield wire
        finally:
            w6.lib = saved


def _dev(v):
    from lwm_amd.w6 import W6Kernel
    if torch.is_tensor(v):
        return Dev(v)
    if isinstance(v, W6Kernel):
        return W6Kernel(_dev(v.q), _dev(v.scale), v.shape, v.stamp)
    if isinstance(v, (list, tuple)):
        return type(v)(_dev(e) for e in v)
    return v


def pack(k=K, n=N):
    from lwm_amd.w6 import W6Kernel
    return W6Kernel(torch.full((k // 4, n // 8, 24), 0x22, dtype=u8), torch.full((k // 32, n), 127, dtype=u8), (k, n), (0, 0))


def pack8():
    from lwm_amd.w8 import W8Kernel
    return W8Kernel(torch.zeros(K, N, dtype=u8), torch.ones(2, N), (K, N), (0, 0))


def make():
    g = torch.Generator().manual_seed(0)
    return dict(x=torch.randn(R, K, generator=g).to(bf16), packs=[pack()])


def make_full():
    kw = make()
    kw["packs"] = [pack(K, 128)]
    kw.update(norm=(torch.ones(R, 4), torch.ones(K, dtype=bf16), 1e-6), residual=torch.zeros(R, 128, dtype=bf16), want_ss=True)
    return kw


def _pack_edit(**fields):
    def edit(kw):
        p = kw["packs"][0]
        for k, f in fields.items():
            setattr(p, k, f(getattr(p, k)))
    return edit


GEMV_DEFECTS = {
    "x f32": lambda kw: kw.update(x=kw["x"].float()),
    "x of three dimensions": lambda kw: kw.update(x=kw["x"].reshape(1, R, K)),
    "x with a strided inner dimension": lambda kw: kw.update(x=torch.zeros(R, 2 * K, dtype=bf16)[:, ::2]),
    "x of another K": lambda kw: kw.update(x=torch.zeros(R, K + 32, dtype=bf16)),
    "no packs": lambda kw: kw.update(packs=[]),
    "four packs": lambda kw: kw.update(packs=[pack() for _ in range(4)]),
    "a bf16 tensor instead of a pack": lambda kw: kw.update(packs=[torch.zeros(K, N, dtype=bf16)]),
    "an 8-bit pack": lambda kw: kw.update(packs=[pack8()]),
    "codes int8": _pack_edit(q=lambda t: t.to(torch.int8)),
    "codes row-major (K, 3 N / 4)": _pack_edit(q=lambda t: t.reshape(K, 3 * N // 4)),
    "codes of another shape": _pack_edit(q=lambda t: torch.zeros(K // 4, N // 8 + 1, 24, dtype=u8)),
    "codes in 16-byte slots": _pack_edit(q=lambda t: torch.zeros(K // 4, N // 8, 16, dtype=u8)),
    "codes strided": _pack_edit(q=lambda t: torch.zeros(K // 4, N // 8, 48, dtype=u8)[:, :, ::2]),
    "scales f32": _pack_edit(scale=lambda t: t.float()),
    "scales per 128 rows": _pack_edit(scale=lambda t: t[:2]),
    "scales strided": _pack_edit(scale=lambda t: torch.zeros(K // 32, 2 * N, dtype=u8)[:, ::2]),
    "out_dtype f16": lambda kw: kw.update(out_dtype=torch.float16),
}
FULL_DEFECTS = {
    "norm ss f64": lambda kw: kw.update(norm=(kw["norm"][0].double(),) + kw["norm"][1:]),
    "norm ss with 65 partials": lambda kw: kw.update(norm=(torch.ones(R, 65),) + kw["norm"][1:]),
    "norm weight f32": lambda kw: kw.update(norm=(kw["norm"][0], kw["norm"][1].float(), 1e-6)),
    "residual f32": lambda kw: kw.update(residual=kw["residual"].float()),
    "residual of another shape": lambda kw: kw.update(residual=torch.zeros(R, 64, dtype=bf16)),
    "residual with two packs": lambda kw: kw.update(packs=[pack(K, 128), pack(K, 128)], want_ss=False),
    "want_ss with an f32 output": lambda kw: kw.update(out_dtype=f32, residual=None),
    "want_ss with N % 128": lambda kw: kw.update(packs=[pack(K, 48)], residual=None),
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


WRAPPERS = ("gemv_fused_w6", "gemm_rows_fused_w6")
ROWS_DEFECTS = {
    "no rows": lambda kw: kw.update(x=torch.zeros(0, K, dtype=bf16)),
    "33 rows": lambda kw: kw.update(x=torch.zeros(33, K, dtype=bf16)),
    "x misaligned": lambda kw: kw.update(x=torch.zeros(R, K + 8, dtype=bf16)[:, 4:K + 4]),
    "a row stride that is no multiple of 8": lambda kw: kw.update(x=torch.zeros(R, K + 4, dtype=bf16)[:, :K]),
}


def test_host_tensors_are_refused_before_the_library():
    from lwm_amd import w6
    with tripwire() as wire:
        for kw in (make(), make_full()):
            for fn in WRAPPERS:
                with pytest.raises(ValueError):
                    getattr(w6, fn)(**kw)
        with pytest.raises(ValueError):
            w6.quantise_weight(torch.zeros(K, N, dtype=bf16))
        assert wire.reached == []


@pytest.mark.parametrize("name", list(GEMV_DEFECTS) + list(FULL_DEFECTS))
def test_each_gemv_defect_is_refused_on_its_own(name):
    """every tensor claims to be on a device, so the one edit is the only defect of the call"""
    from lwm_amd import w6
    kw, edit = (make(), GEMV_DEFECTS[name]) if name in GEMV_DEFECTS else (make_full(), FULL_DEFECTS[name])
    edit(kw)
    kw = {k: _dev(v) for k, v in kw.items()}
    with standin_devices() as wire:
        for fn in WRAPPERS:
            with pytest.raises(ValueError):
                getattr(w6, fn)(**kw)
        assert wire.reached == []


@pytest.mark.parametrize("name", list(ROWS_DEFECTS))
def test_each_rows_defect_is_refused_on_its_own(name):
    """what the rows entry asks of x beyond the GEMV: 1..32 rows, 16-byte alignment, a row stride of whole 16-byte words"""
    from lwm_amd import w6
    kw = make()
    ROWS_DEFECTS[name](kw)
    kw = {k: _dev(v) for k, v in kw.items()}
    with standin_devices() as wire:
        with pytest.raises(ValueError, match="gemm_rows_fused_w6"):
            w6.gemm_rows_fused_w6(**kw)
        assert wire.reached == []


@pytest.mark.parametrize("name", list(QUANT_DEFECTS))
def test_each_quantiser_defect_is_refused_on_its_own(name):
    from lwm_amd import w6
    k = Dev(QUANT_DEFECTS[name](torch.zeros(K, N, dtype=bf16)))
    with standin_devices() as wire:
        with pytest.raises(ValueError):
            w6.quantise_weight(k)
        assert wire.reached == []


def test_the_well_formed_calls_pass_every_check():
    """... and the tables above are not vacuous: with the stand-in devices the unedited calls get as far as the library"""
    from lwm_amd import w6
    for kw in (make(), make_full()):
        kw = {k: _dev(v) for k, v in kw.items()}
        for fn in WRAPPERS:
            entry = "lwm_" + fn
            with standin_devices() as wire:
                with pytest.raises(AssertionError, match="reached the C library: " + entry):
                    getattr(w6, fn)(**kw)
                assert wire.reached == [entry]
    with standin_devices() as wire:
        with pytest.raises(AssertionError, match="reached the C library: lwm_w6_quantise"):
            w6.quantise_weight(Dev(torch.zeros(K, N, dtype=bf16)))
        assert wire.reached == ["lwm_w6_quantise"]


def test_a_stale_pack_names_its_parameter():
    from lwm_amd.w6 import W6Kernel
    w = torch.zeros(32, 16, dtype=bf16)
    p = W6Kernel(None, None, (32, 16), (w._version, w.data_ptr()))
    assert p.check(w, "h.0.attention.wq") is p
    w.add_(1)
    with pytest.raises(RuntimeError, match=r"h\.0\.attention\.wq.*fp6.*quantize_decode_weights\('fp6'\)"):
        p.check(w, "h.0.attention.wq")
    with pytest.raises(RuntimeError, match="lm_head"):
        p.check(w.clone(), "lm_head")                 # another tensor at another address


def test_w6_dequant_is_the_layout_of_the_restatement():
    """the torch statement of the byte layout against the numpy one (tests/_w6_ref.py), on host tensors"""
    from lwm_amd.w6 import w6_dequant
    for name, w in W6.quantiser_cases():
        q, e = W6.quantise(w)
        got = w6_dequant(torch.from_numpy(q), torch.from_numpy(e), w.shape)
        ref = torch.from_numpy(W6.rounded(q, e, w.shape)).to(bf16)
        assert got.dtype == bf16 and torch.equal(got.view(torch.int16), ref.view(torch.int16)), name
    with pytest.raises(ValueError, match="w6_dequant"):
        w6_dequant(torch.from_numpy(q).reshape(-1, 16), torch.from_numpy(e), w.shape)
    with pytest.raises(ValueError, match="w6_dequant"):
        w6_dequant(torch.from_numpy(q), torch.from_numpy(e).float(), w.shape)


# ---------------------------------------------------------------- the model's refusals that need no device
def test_model_refusals_by_name():
    m = _tiny(f32)
    with pytest.raises(NotImplementedError, match=r"'fp6'.*float32 model.*6-bit"):
        m.quantize_decode_weights("fp6")
    m = _tiny(bf16)
    with pytest.raises(ValueError, match="int4"):
        m.quantize_decode_weights("int4")
    with tripwire() as wire:
        with pytest.raises(ValueError, match=r"'fp6'.*h\.0\.attention\.wq"):       # host parameters: no CPU path, named
            m.quantize_decode_weights("fp6")
        assert wire.reached == []
    assert m.decode_packs("fp6") is None and m.decode_packs("fp8") is None and m.quantize_decode_weights("bf16") is m and m.drop_decode_weights() is m


def test_sp_ring_is_refused_by_name(monkeypatch):
    from lwm_amd import llama
    m = _tiny(bf16)
    monkeypatch.setattr(llama, "sp_size_rank", lambda axis: (2, 0))
    with pytest.raises(NotImplementedError, match=r"'fp6'.*sp > 1"):
        m.quantize_decode_weights("fp6")
    assert m.decode_packs("fp6") is None


# ---------------------------------------------------------------- the entry points' environment switch
def test_apply_decode_weights(monkeypatch):
    from lwm_amd.cli import _common
    m = _Model()
    for v in ("fp6", "FP6", "Fp6"):
        monkeypatch.setenv("LWM_DECODE_WEIGHTS", v)
        assert _common.apply_decode_weights(m) is m
    assert m.calls == ["fp6", "fp6", "fp6"]
    monkeypatch.setenv("LWM_DECODE_WEIGHTS", "fp8")
    _common.apply_decode_weights(m)
    assert m.calls[-1] == "fp8"
    for bad in ("bogus", "int4", "4", "fp4 ", "int6", "6", "fp6 ", "mxfp6"):       # the existing boundary tests' values among them
        monkeypatch.setenv("LWM_DECODE_WEIGHTS", bad)
        with pytest.raises(SystemExit, match=f"LWM_DECODE_WEIGHTS='{bad}': 'fp8', 'bf16'"):
            _common.apply_decode_weights(m)
    assert len(m.calls) == 4
