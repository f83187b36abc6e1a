"""The dQ kernel (attn_bwd_dq4_kernel / _meta, 16x16x32 bf16 MFMAs) on the device at the shapes of
tests/_dq16_cases.py: every element of dq against the fp64 oracle with the bound of
tests/test_gpu_attention.py::test_fwd_bwd_vs_oracle (tests/_parity.py::check_dq), bit-identical repeats, the f32 carry
both ways.  The kernel takes the saved output and the LSE of the case's reference (the oracle's, the output rounded to
bf16), so the verdict is about this kernel alone."""
import numpy as np
import pytest

from tests import _dq16_cases as Q

pytestmark = pytest.mark.gpu


def _dev(a, dt=None):
    import torch
    t = torch.from_numpy(np.array(a)).cuda()      # (a copy: the shared references are read-only)
    return t if dt is None else t.to(dt)


def _dq(case, **kw):
    import torch
    from lwm_amd import ops
    q, k, v, do = (_dev(t, torch.bfloat16) for t in case.operands(False))
    out, lse, *_ = Q.reference(case.name)
    ckw = dict(case.kw)
    for n, dt in (("seg_q", torch.int32), ("seg_k", torch.int32), ("key_valid", torch.uint8)):
        if ckw.get(n) is not None:
            ckw[n] = _dev(ckw[n], dt)
    lse_d = _dev(lse)
    delta = ops.attn_bwd_delta(_dev(out, torch.bfloat16), do, lse_d)
    dq = ops.attn_bwd_dq_block(q, k, v, do, lse_d, delta, **ckw, **kw)
    torch.cuda.synchronize()
    return dq


@pytest.mark.parametrize("case", Q.CASES, ids=repr)
def test_dq_vs_oracle(case):
    import torch
    dq = _dq(case)
    Q.verify_dq(case, dq.float().cpu().numpy())
    assert torch.equal(dq, _dq(case)), f"{case.name}: dq differs between two runs"


@pytest.mark.parametrize("carry_in", [False, True], ids=["fresh", "carry_in"])
@pytest.mark.parametrize("final", [False, True], ids=["to_acc", "final"])
def test_dq_carry(carry_in, final):
    import torch
    case = Q.CARRY_CASE
    B, Sq, H, D = case.operands(False)[0].shape
    offset = (np.random.default_rng(7).standard_normal((B, Sq, H, D)) * 0.05).astype(np.float32) if carry_in else None
    run = lambda: _dq(case, carry_in=carry_in, final=final, dq_acc=_dev(offset) if carry_in else None)
    got = run()
    assert got.dtype == (torch.bfloat16 if final else torch.float32)
    Q.verify_dq(case, got.float().cpu().numpy(), offset=None if offset is None else offset.astype(np.float64))
    assert torch.equal(got, run())
