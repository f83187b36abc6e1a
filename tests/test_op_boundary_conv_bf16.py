"""The operator boundary of the bf16 convolution wrappers, the CPU half (tests/test_op_boundary.py has the table of the
older wrappers): under the tripwire library, well-formed and malformed calls with host tensors are refused with
ValueError before anything reaches the C library.  Also what needs no device of the precision switch: the VQGAN keyword
and LWM_VQGAN_PRECISION."""
import pytest
import torch

from tests import _boundary as Bd, _emu


@pytest.fixture()
def wire():
    with Bd.tripwire(_emu.lib()) as w:
        yield w


def _call(**over):
    from lwm_amd import ops
    kw = dict(x=torch.zeros(1, 8, 8, 64), pack=ops.ConvPackBF16(torch.zeros(9, 8, 64, 8, dtype=torch.bfloat16), (3, 3, 64, 64)),
              bias=torch.zeros(64), residual=torch.zeros(1, 8, 8, 64))
    kw.update(over)
    return ops.conv2d_nhwc_bf16(**kw)


def test_host_tensors_never_reach_the_library(wire):
    from lwm_amd import ops
    assert ops.lib() is wire
    with pytest.raises(ValueError, match="ROCm device tensor"):
        ops.conv_pack_bf16(torch.zeros(3, 3, 64, 64))
    with pytest.raises(ValueError, match="ROCm device tensor"):
        _call()
    assert wire.reached == []


@pytest.mark.parametrize("over", [dict(x=torch.zeros(1, 8, 8, 32)), dict(x=torch.zeros(8, 8, 64)), dict(pack=torch.zeros(9, 8, 64, 8)),
                                  dict(bias=torch.zeros(32)), dict(residual=torch.zeros(1, 8, 8, 32)), dict(x=torch.zeros(1, 8, 8, 64).double())],
                         ids=["channels", "rank", "pack type", "bias shape", "residual shape", "dtype"])
def test_bad_calls_stay_off_the_library(over, wire):
    with pytest.raises(ValueError):
        _call(**over)
    assert wire.reached == []


def test_pack_refuses_ineligible_kernels_by_name(wire):
    from lwm_amd import ops
    for shape in ((3, 3, 40, 64), (3, 3, 64, 3), (3, 64, 64)):
        with pytest.raises(ValueError):
            ops.conv_pack_bf16(torch.zeros(shape))
    assert wire.reached == []


def test_precision_switch_values():
    from lwm_amd.cli._common import parse_vqgan_precision
    from lwm_amd.vqgan import VQGAN
    assert [parse_vqgan_precision(t) for t in ("", None, "f32", "F32", "bf16", "BF16")] == ["f32", "f32", "f32", "f32", "bf16", "bf16"]
    for bad in ("int8", "fp16", "bfloat16"):
        with pytest.raises(SystemExit, match=f"LWM_VQGAN_PRECISION='{bad}'"):
            parse_vqgan_precision(bad)
    with pytest.raises(ValueError, match="'f32'.*'bf16'"):
        VQGAN(params={}, precision="fp16")
