"""Attention at the inputs nobody feeds it, on the host emulator (tests/emu): a softmax scale that is not 1/sqrt(D),
strided operands between poisoned gaps, masks that empty whole tiles and hundreds of rows, large logits through the
backward, an 8-bit cache with scales all over the place.  The cases are tests/_attn_cases.py's; the device runs the same
ones in tests/test_gpu_attn_edges.py.  Bounds: the 1e-2 / 1e-4 of tests/test_emu_kernels.py for the bf16 kernels, the
1e-5 of tests/test_emu_attn_f32.py for the f32 flavour, the 2e-2 / 2e-3 of test_decode_kv8_vs_oracle for the 8-bit cache."""
import numpy as np
import pytest

from oracle import attention_ref as R
from tests import _attn_cases as A, _emu
from tests.test_emu_kv8 import emu_cache, emu_decode

FLAVOURS = [pytest.param(False, id="bf16"), pytest.param(True, id="f32")]


def _run(case, f32):
    q, k, v, do = case.operands(f32)
    kw = case.kw
    if f32:
        out, lse = _emu.attn_fwd_f32(q, k, v, **kw)
        dq, dk, dv = _emu.attn_bwd_f32(q, k, v, out, lse, do, **kw)
    else:
        out, lse = _emu.attn_fwd(q, k, v, **kw)
        dq, dk, dv = _emu.attn_bwd(q, k, v, out, lse, do, **kw)
    return dict(out=out, lse=lse, dq=dq, dk=dk, dv=dv)


def _run_and_verify(case, f32):
    got = _run(case, f32)
    A.verify(case, got, A.EMU_F32 if f32 else A.EMU_BF16, f32)
    if case.has_segments and not f32:
        # the segment-block hints skip work, they never change a bit
        _emu.SEGMENT_SKIP = False
        try:
            plain = _run(case, f32)
        finally:
            _emu.SEGMENT_SKIP = True
        for n in got:
            assert np.array_equal(got[n], plain[n]), f"{case.name}: {n} differs with the segment-block hints"


# ---------------------------------------------------------------- B1
@pytest.mark.parametrize("f32", FLAVOURS)
@pytest.mark.parametrize("case", A.scale_cases(), ids=repr)
def test_scale_fwd_bwd(case, f32):
    _run_and_verify(case, f32)


@pytest.mark.parametrize("scale", A.SCALES)
@pytest.mark.parametrize("Sq,splits", [(40, 3), (1, 1), (1, 3)], ids=["splitk", "decode", "decode_splitk"])
def test_scale_dense_mask_inference(Sq, splits, scale):
    """the dense-mask split-K forward + lwm_attn_combine, and (Sq = 1) the decode kernel"""
    q, k, v, mask, scale = A.infer_case(scale, Sq)
    out, lse = _emu.attn_infer(q, k, v, mask, k_splits=splits, scale=scale)
    ro, rl = R.dense_attention(q, k, v, causal=False, dense_mask=mask, scale=scale)
    o0, _ = R.dense_attention(q, k, v, causal=False, dense_mask=mask)
    assert A.Bounds.rel(ro, o0) > 10 * A.EMU_BF16.tol
    A.EMU_BF16.check(f"infer_scale{scale}.out", out, ro)
    A.EMU_BF16.check_lse(f"infer_scale{scale}.lse", lse, rl)


def _kv8_emu(kq, ks, vq, vs):
    B, Sk, H, _ = kq.shape
    (ka, sa), (va, ta) = emu_cache(B, Sk, H), emu_cache(B, Sk, H)        # (16-byte aligned copies)
    ka[...], sa[...], va[...], ta[...] = kq, ks, vq, vs
    return ka, sa, va, ta


@pytest.mark.parametrize("scale", A.SCALES)
def test_scale_decode_kv8(scale):
    q, kq, ks, vq, vs, mask, splits = A.kv8_case(seed=520)
    out, lse, _, _ = emu_decode(q, *_kv8_emu(kq, ks, vq, vs), mask, splits, scale=scale)
    ro, rl = A.kv8_reference(q, kq, ks, vq, vs, mask, scale)
    o0, _ = R.dense_attention(q, A.K8.dequant(kq, ks), A.K8.dequant(vq, vs), causal=False, dense_mask=mask)
    assert A.Bounds.rel(ro, o0) > 10 * 2e-2
    assert np.abs(out - ro).max() / np.abs(ro).max() <= 2e-2
    assert np.abs(lse - rl).max() <= 2e-3


# ---------------------------------------------------------------- B2
@pytest.mark.parametrize("f32", FLAVOURS)
@pytest.mark.parametrize("case", A.strided_cases(), ids=repr)
def test_strided_operands_between_poisoned_gaps(case, f32):
    """q, k, v, out, dout, dq, dk, dv all slots of larger buffers whose every other byte is NaN bits: the bits of the
    dense call, and not one gap byte touched"""
    q, k, v, do = case.operands(f32)
    B, Sq, H, _ = q.shape
    Sk = k.shape[1]
    dt = np.float32 if f32 else np.uint16
    enc = (lambda x: x) if f32 else R.to_bf16_bits

    def run(strided):
        if strided:
            qbuf, (qa, oa, doa, dqa) = A.slots_np(B, Sq, 4, H, dt)
            kbuf, (ka, va, dka, dva) = A.slots_np(B, Sk, 4, H, dt)
        else:
            qbuf = kbuf = None
            qa, oa, doa, dqa = (_emu.aligned((B, Sq, H, A.D), dt) for _ in range(4))
            ka, va, dka, dva = (_emu.aligned((B, Sk, H, A.D), dt) for _ in range(4))
        qa[...], ka[...], va[...], doa[...] = enc(q), enc(k), enc(v), enc(do)
        lse = _emu.attn_train_raw(qa, ka, va, oa, doa, dqa, dka, dva, **case.kw)
        return (oa, dqa, dka, dva, lse), (qbuf, kbuf)

    dense, _ = run(False)
    strided, bufs = run(True)
    assert strided[0].strides != dense[0].strides
    for n, a, b in zip(("out", "dq", "dk", "dv", "lse"), strided, dense):
        assert np.array_equal(a.view(np.uint8) if a.flags.c_contiguous else np.ascontiguousarray(a).view(np.uint8),
                              np.ascontiguousarray(b).view(np.uint8)), f"{case.name}: {n} differs from the dense call"
    assert all(A.gaps_intact_np(b) for b in bufs), "a byte outside the operands was written"
    dec = (lambda x: x) if f32 else R.from_bf16_bits
    got = dict(out=dec(strided[0]), dq=dec(strided[1]), dk=dec(strided[2]), dv=dec(strided[3]), lse=strided[4])
    A.verify(case, got, A.EMU_F32 if f32 else A.EMU_BF16, f32)


# ---------------------------------------------------------------- B3
@pytest.mark.parametrize("f32", FLAVOURS)
@pytest.mark.parametrize("case", A.mask_cases(), ids=repr)
def test_mask_structure(case, f32):
    _run_and_verify(case, f32)


# ---------------------------------------------------------------- B4
@pytest.mark.parametrize("case", A.large_logit_cases(), ids=repr)
def test_large_logits_through_the_backward(case):
    _run_and_verify(case, False)


# ---------------------------------------------------------------- B5
def test_decode_kv8_heterogeneous_scales():
    q, kq, ks, vq, vs, mask, splits = A.kv8_case()
    assert len(np.unique(ks)) >= 5 and len(np.unique(vs)) >= 20
    out, lse, _, _ = emu_decode(q, *_kv8_emu(kq, ks, vq, vs), mask, splits)
    ro, rl = A.kv8_reference(q, kq, ks, vq, vs, mask)
    print("kv8 heterogeneous scales: out", np.abs(out - ro).max() / np.abs(ro).max(), "lse", np.abs(lse - rl).max())
    assert np.abs(out - ro).max() / np.abs(ro).max() <= 2e-2
    assert np.abs(lse - rl).max() <= 2e-3
