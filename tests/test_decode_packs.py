"""The model's one decode-pack state (LLaMAForCausalLM._decode_packs behind decode_packs()) and the one table of weight formats
(lwm_amd.wpack.FORMATS) on the host: a tiny bf16 model whose quantisers are stubs, so no device and no library call."""
import itertools

import pytest
import torch

from tests.test_w8_boundary import _Model, _tiny

MODES = ("fp8", "fp6", "fp4")
# what a caller might pass: every fpN, the integer formats nobody built, the wrong case
CANDIDATES = [f"fp{n}" for n in range(1, 33)] + ["bf16", "int8", "int4", "w8", "e4m3", "mxfp4", "FP8", "none"]


@pytest.fixture
def model(monkeypatch):
    """the tiny model, with each format's quantise_weight replaced by a stub that returns an (empty) pack of its class"""
    from lwm_amd.wpack import FORMATS
    for fmt in FORMATS.values():
        cls = getattr(fmt.module, fmt.pack)
        monkeypatch.setattr(fmt.module, "quantise_weight",
                            lambda p, cls=cls: cls(None, None, p.shape, (p._version, p.data_ptr())))
    return _tiny(torch.bfloat16)


def _holds(m, mode):
    """m holds the packs of `mode` (None: none) and says so through every reading of decode_packs"""
    from lwm_amd.wpack import FORMATS
    for other in MODES:
        if other != mode:
            assert m.decode_packs(other) is None
    if mode is None:
        assert m.decode_packs() is None
        return
    packs = m.decode_packs(mode)
    fmt, held = m.decode_packs()
    assert fmt is FORMATS[mode] and held is packs
    assert len(packs) == 7 * len(m.h) + 1 and set(packs) == {n for n, _ in m._decode_weight_params()}
    cls = getattr(fmt.module, fmt.pack)
    assert all(type(p) is cls and p.fmt is fmt for p in packs.values())


def test_formats_table():
    from lwm_amd import wpack
    assert tuple(wpack.FORMATS) == MODES
    for mode, fmt in wpack.FORMATS.items():
        assert fmt.mode == mode and fmt.module.FORMAT is fmt
        cls = getattr(fmt.module, fmt.pack)
        assert issubclass(cls, wpack.WeightPack) and cls.fmt is fmt
        assert fmt.proj.fused[0] is not None
        for name, entry in zip(fmt.proj.fused, fmt.proj.entries):
            assert (name is None) == (entry is None)
            if name is not None:
                assert callable(getattr(fmt.module, name))
    assert [f.proj.fused[1] is None for f in wpack.FORMATS.values()] == [False, False, True]     # (no 4-bit rows entry)


@pytest.mark.parametrize("first,second", list(itertools.permutations(MODES, 2)))
def test_one_kind_of_pack_is_held(model, first, second):
    _holds(model, None)
    assert model.quantize_decode_weights(first) is model
    _holds(model, first)
    assert model.quantize_decode_weights(second) is model
    _holds(model, second)
    assert model.quantize_decode_weights(first) is model
    _holds(model, first)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("drop", ["bf16", None, "drop"])
def test_dropping_leaves_none(model, mode, drop):
    model.quantize_decode_weights(mode)
    _holds(model, mode)
    assert (model.drop_decode_weights() if drop == "drop" else model.quantize_decode_weights(drop)) is model
    _holds(model, None)


def test_a_stand_in_without_the_attribute_holds_nothing(model):
    del model._decode_packs
    _holds(model, None)


def test_every_front_end_takes_the_same_modes(model, monkeypatch):
    from lwm_amd.cli import _common
    from lwm_amd.wpack import FORMATS
    want = set(FORMATS) | {"bf16"}

    def quantize_takes(mode):
        try:
            model.quantize_decode_weights(mode)
        except ValueError:
            return False
        return True

    def apply_takes(mode):
        monkeypatch.setenv("LWM_DECODE_WEIGHTS", mode)
        m = _Model()
        try:
            _common.apply_decode_weights(m)
        except SystemExit:
            return False
        assert m.calls == ([mode] if mode in FORMATS else [])
        return True

    lower = [c for c in CANDIDATES if c == c.lower()]
    assert {c for c in CANDIDATES if quantize_takes(c)} == want
    assert {c for c in lower if apply_takes(c)} == want          # (the environment switch folds case: FP8 is fp8 there)
    assert set(_common._DECODE_WEIGHTS_NOTES) == set(FORMATS)
