"""The bf16 convolution route of the VQGAN on MI355X: the contract of lwm_conv2d_nhwc_bf16 (include/lwm_hip.h; cases and
references in tests/_conv16_ref.py) through ops.conv_pack_bf16 / ops.conv2d_nhwc_bf16, then the model: which layers take
which kernel under VQGAN(precision=...), every layer held to the contract in place, and the wiring measured against the
rounded-operand oracle.  The f32 route is the parity anchor and its own tests (tests/test_gpu_vqgan.py) stay as they are."""
import numpy as np
import pytest

from lwm_amd.vqgan import VQGAN, VQGANConfig, random_params
from oracle import vqgan_ref as R
from oracle.attention_ref import round_bf16
from tests import _conv16_ref as K

pytestmark = pytest.mark.gpu


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _conv(x, w, b=None, r=None, **kw):
    from lwm_amd import ops
    return ops.conv2d_nhwc_bf16(_dev(x), ops.conv_pack_bf16(_dev(w)), _dev(b), _dev(r), **kw).cpu().numpy()


def test_pack_is_the_documented_layout():
    import torch
    from lwm_amd import ops
    w = K.random_case(0, 1, 1, 1, 64, 96, 3, {}, False)[1]
    p = ops.conv_pack_bf16(_dev(w))
    assert p.shape == (3, 3, 64, 96) and p.data.dtype == torch.bfloat16 and p.data.is_contiguous()
    assert np.array_equal(p.data.view(torch.int16).cpu().numpy().view(np.uint16), K.pack(w))


@pytest.mark.parametrize("case", K.CASES, ids=K.IDS)
def test_exact_on_integer_data(case):
    """contract point 1"""
    *shape, kw, res = case
    x, w, b, r = K.int_case(1, *shape, kw, res)
    got, ref = _conv(x, w, b, r, **kw), R.conv2d(x, w, b, r, **kw)
    assert got.shape == ref.shape and np.array_equal(got, ref), np.abs(got - ref).max()


@pytest.mark.parametrize("case", K.CASES, ids=K.IDS)
def test_random_data_within_the_bound(case):
    """contract point 2"""
    *shape, kw, res = case
    x, w, b, r = K.random_case(2, *shape, kw, res)
    print("worst error / bound:", K.check_contract2(_conv(x, w, b, r, **kw), x, w, b, r, **kw))


def test_full_resolution_layer_exact():
    """one layer at the size the tokeniser runs it, 512 tiles of 128 x 128 with the residual: integer data, exact"""
    x, w, b, r = K.int_case(3, 1, 256, 256, 128, 128, 3, {}, True)
    assert np.array_equal(_conv(x, w, b, r), R.conv2d(x, w, b, r))


def test_clip_without_bias():
    x, w, _, _ = K.random_case(8, 1, 12, 12, 32, 128, 3, {}, False)
    x *= 4.0
    got = _conv(x, w, clip=True)
    y64, mag = K.ref64(x, w)
    assert np.abs(got).max() == 1.0 and (np.abs(y64) > 1).mean() > 0.2
    assert (np.abs(got - np.clip(y64, -1, 1)) <= K.bound(w, mag)).all()


def test_rounding_is_nearest_even_at_the_staging():
    """contract point 3"""
    x, w = K.rne_case()
    got = _conv(x, w)
    assert np.array_equal(got.view(np.uint32), round_bf16(x).view(np.uint32))


def test_hidden_memory_reaches_nothing():
    """contract point 4: x, the residual and the output between guard bands of NaN patterns, x with no room behind its
    last image: the same bits as from plain tensors, finite, the guards intact"""
    import torch
    from lwm_amd import ops
    Guarded = K.DevGuarded
    for case in (K.CASES[0], K.CASES[5], K.CASES[7]):
        *shape, kw, res = case
        x, w, b, r = K.random_case(10, *shape, kw, res)
        plain = _conv(x, w, b, r, **kw)
        gx, gy = Guarded(x.shape, torch.float32, _dev(x)), Guarded(plain.shape, torch.float32)
        gr = Guarded(plain.shape, torch.float32, _dev(r)) if res else None
        ops.conv2d_nhwc_bf16(gx.t, ops.conv_pack_bf16(_dev(w)), _dev(b), gr.t if res else None, out=gy.t, **kw)
        assert gx.intact() and gy.intact() and (gr is None or gr.intact())
        assert np.array_equal(gy.t.cpu().numpy(), plain) and np.isfinite(plain).all()


def test_same_launch_same_bits_and_batch_independence():
    """contract point 5"""
    x, w, b, r = K.random_case(11, 3, 8, 24, 64, 128, 3, {}, True)
    a = _conv(x, w, b, r)
    assert np.array_equal(a, _conv(x, w, b, r))
    assert np.array_equal(_conv(x[1:2], w, b, r[1:2])[0], a[1])


def test_refusals_by_name():
    """contract point 6 at the operator boundary and at the C entry"""
    import ctypes as C
    import torch
    from lwm_amd import _capi, ops
    with pytest.raises(ValueError, match="Cin=40"):
        ops.conv_pack_bf16(torch.zeros(3, 3, 40, 64).cuda())
    with pytest.raises(ValueError, match="Cout=3"):
        ops.conv_pack_bf16(torch.zeros(3, 3, 64, 3).cuda())
    pack = ops.conv_pack_bf16(torch.zeros(3, 3, 64, 64).cuda())
    x = torch.zeros(1, 8, 8, 64).cuda()
    for bad in (dict(x=x.cpu()), dict(x=torch.zeros(1, 8, 8, 32).cuda()), dict(x=x.double()), dict(bias=torch.zeros(32).cuda()),
                dict(residual=torch.zeros(1, 8, 8, 32).cuda()), dict(pack=torch.zeros(9, 8, 64, 8).cuda())):
        kw = dict(x=x, pack=pack)
        kw.update(bad)
        with pytest.raises(ValueError):
            ops.conv2d_nhwc_bf16(**kw)
    L = ops.lib()
    y = torch.zeros(1, 8, 8, 64).cuda()
    args = lambda Cin, Cout: _capi.LwmConvArgs(x.data_ptr(), pack.data.data_ptr(), None, None, y.data_ptr(), 1, 8, 8, Cin, Cout, 3, 3,
                                               1, 1, 0, 8, 8, 0)
    assert L.lwm_conv2d_nhwc_bf16(C.byref(args(40, 64)), None) == _capi.LWM_EUNSUPPORTED and b"Cin=40" in L.lwm_last_error()
    assert L.lwm_conv2d_nhwc_bf16(C.byref(args(64, 3)), None) == _capi.LWM_EUNSUPPORTED and b"Cout=3" in L.lwm_last_error()
    assert L.lwm_conv2d_nhwc_bf16(None, None) == _capi.LWM_EINVAL


# ---------------------------------------------------------------- the model: default widths, resolution 32, one frame
@pytest.fixture(scope="module")
def model():
    """params, config, one frame, and the f32 oracle's latents, codes and decoded pixels of it (computed once)"""
    cfg = VQGANConfig.get_default_config(dict(resolution=32))
    params = random_params(cfg, seed=0)
    x = np.random.default_rng(5).uniform(-1, 1, (1, 32, 32, 3)).astype(np.float32)
    d = cfg.as_dict()
    lat = R.conv2d(R.encoder(params["encoder"], x, d), params["quant_conv"]["kernel"], params["quant_conv"]["bias"])
    codes = R.vq_argmin(lat, params["quantize"]["embeddings"])
    return dict(cfg=cfg, d=d, params=params, x=x, lat=lat, codes=codes, pix=R.decode(params, codes, d))


def _latents(vq, x):
    import torch
    with torch.no_grad():
        return vq._conv(vq.params["quant_conv"], vq._encoder(vq.params["encoder"], _dev(x))).cpu().numpy()


def _record(monkeypatch):
    from lwm_amd import ops
    calls = []
    f32, b16 = ops.conv2d_nhwc, ops.conv2d_nhwc_bf16

    def rec_f32(x, w, bias=None, residual=None, **kw):
        calls.append(("f32", tuple(w.shape)))
        return f32(x, w, bias, residual, **kw)

    def rec_b16(x, pack, bias=None, residual=None, **kw):
        y = b16(x, pack, bias, residual, **kw)
        calls.append(("bf16", pack.shape, x, pack, bias, residual, kw, y))
        return y
    monkeypatch.setattr(ops, "conv2d_nhwc", rec_f32)
    monkeypatch.setattr(ops, "conv2d_nhwc_bf16", rec_b16)
    return calls


def test_routing_and_the_default_is_untouched(model, monkeypatch):
    import torch
    m = model
    calls = _record(monkeypatch)
    out = {}
    for name, kw in (("none", {}), ("f32", dict(precision="f32")), ("bf16", dict(precision="bf16"))):
        vq = VQGAN(params=m["params"], config=m["cfg"], **kw)
        del calls[:]
        out[name] = (vq.encode(_dev(m["x"]))[1], torch.from_numpy(_latents(vq, m["x"])), vq.decode(_dev(m["codes"])))
        taken = [(c[0], c[1]) for c in calls]
        if name == "bf16":
            assert {s for k, s in taken if k == "f32"} == {(3, 3, 3, 128), (3, 3, 128, 3)}
            assert all((s[2] == 3 or s[3] == 3) == (k == "f32") for k, s in taken) and sum(k == "bf16" for k, _ in taken) > 60
        else:
            assert taken and all(k == "f32" for k, _ in taken)
    for a, b in zip(out["none"], out["f32"]):
        assert torch.equal(a.cpu(), b.cpu())


def test_every_layer_in_place(model, monkeypatch):
    """each convolution the bf16 route runs inside encode and decode, held to contract point 2 on the operands it was
    given (fp64 reference on the CPU)"""
    import torch
    m = model
    calls = _record(monkeypatch)
    vq = VQGAN(params=m["params"], config=m["cfg"], precision="bf16")
    vq.encode(_dev(m["x"]))
    vq.decode(_dev(m["codes"]))
    layers = [c for c in calls if c[0] == "bf16"]
    assert len(layers) > 60
    worst = 0.0
    for _, shape, x, pack, bias, residual, kw, y in layers:
        KH, KW, Cin, Cout = shape
        w = pack.data.float().permute(0, 1, 3, 2).reshape(KH, KW, Cin, Cout).cpu().numpy()      # (bf16 values: rounding them again changes nothing)
        n = lambda t: None if t is None else t.cpu().numpy()
        opts = {k: v for k, v in kw.items() if k != "clip"}
        assert not kw.get("clip")
        worst = max(worst, K.check_contract2(n(y), n(x), w, n(bias), n(residual), **opts))
    print(f"{len(layers)} layers, worst error / bound: {worst:.3f}")


def test_wiring_against_the_rounded_operand_oracle(model):
    """The movement of the bf16 route against the f32 route on the device, beside the movement of the rounded-operand
    oracle against the plain oracle on the CPU (m_ref), in two measures: rms of the latent difference over rms of the
    latents, and mean absolute pixel difference of decode on the f32 oracle's codes.  At most 2 m_ref: the margin stands
    for another order of summation and the occasional flipped rounding; a wiring mistake moves the output by order 1."""
    m = model
    with K.rounded_operand_oracle() as Q:
        lat16 = Q.conv2d(Q.encoder(m["params"]["encoder"], m["x"], m["d"]), m["params"]["quant_conv"]["kernel"],
                         m["params"]["quant_conv"]["bias"])
        pix16 = Q.decode(m["params"], m["codes"], m["d"])
    rms = lambda a: float(np.sqrt(np.mean(np.square(a.astype(np.float64)))))
    ref_lat, ref_pix = rms(lat16 - m["lat"]) / rms(m["lat"]), float(np.abs(pix16 - m["pix"]).mean())
    f32 = VQGAN(params=m["params"], config=m["cfg"])
    b16 = VQGAN(params=m["params"], config=m["cfg"], precision="bf16")
    lat_f, lat_b = _latents(f32, m["x"]), _latents(b16, m["x"])
    dev_lat = rms(lat_b - lat_f) / rms(lat_f)
    dev_pix = float(np.abs(b16.decode(_dev(m["codes"])).cpu().numpy() - f32.decode(_dev(m["codes"])).cpu().numpy()).mean())
    print(f"latents: device {dev_lat:.5f}, rounded-operand oracle {ref_lat:.5f}; pixels: device {dev_pix:.5f}, oracle {ref_pix:.5f}")
    assert 0 < ref_lat < 0.05 and 0 < ref_pix < 0.05          # (the oracle did round, and a format's worth)
    assert 0 < dev_lat <= 2 * ref_lat and 0 < dev_pix <= 2 * ref_pix


def test_agreement_with_the_f32_route_is_reported():
    """resolution 64, 8 frames: how many codes stay and how far the pixels move.  Printed, not asserted: a property of
    the format and the weights, and random weights say little about a trained codebook."""
    cfg = VQGANConfig.get_default_config(dict(resolution=64))
    params = random_params(cfg, seed=0)
    x = _dev(np.random.default_rng(6).uniform(-1, 1, (8, 64, 64, 3)).astype(np.float32))
    f32, b16 = VQGAN(params=params, config=cfg), VQGAN(params=params, config=cfg, precision="bf16")
    idx_f, idx_b = f32.encode(x)[1], b16.encode(x)[1]
    d = (b16.decode(idx_f) - f32.decode(idx_f)).abs()
    print(f"codes equal: {int((idx_f == idx_b).sum())} of {idx_f.numel()}; pixels on the f32 codes: mean {float(d.mean()):.4f}, "
          f"max {float(d.max()):.4f}")
    assert idx_b.shape == idx_f.shape and bool(((idx_b >= 0) & (idx_b < cfg.num_embeddings)).all())


def test_construction_and_cli(model, monkeypatch):
    from lwm_amd.cli import _common
    with pytest.raises(ValueError, match="'f32'.*'bf16'"):
        VQGAN(params=model["params"], config=model["cfg"], precision="fp16")
    monkeypatch.setenv("LWM_VQGAN_PRECISION", "BF16")
    vq = _common.load_vqgan("", 0)
    assert vq.precision == "bf16" and len(vq._packs) > 60
    monkeypatch.delenv("LWM_VQGAN_PRECISION")
    assert _common.load_vqgan("", 0).precision == "f32"
    monkeypatch.setenv("LWM_VQGAN_PRECISION", "int8")
    with pytest.raises(SystemExit, match="LWM_VQGAN_PRECISION='int8'"):
        _common.load_vqgan("", 0)
