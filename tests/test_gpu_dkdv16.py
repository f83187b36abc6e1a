"""The dK/dV kernel (attn_bwd_dkdv4_kernel / _meta, 16x16x32 bf16 MFMAs) on the device at the shapes of
tests/_dkdv16_cases.py: every element of dk and dv against the fp64 oracle with the bound of
tests/test_gpu_attention.py::test_fwd_bwd_vs_oracle (tests/_parity.py::check), exact zeros for keys that no query sees,
bit-identical repeats, the f32 carries both ways.  The kernel takes the saved output and the LSE of the case's reference
(the oracle's, the output rounded to bf16), so the verdict is about this kernel alone."""
import numpy as np
import pytest

from tests import _dkdv16_cases as K

pytestmark = pytest.mark.gpu


def _dev(a, dt=None):
    import torch
    t = torch.from_numpy(np.array(a)).cuda()      # (a copy: the shared references are read-only)
    return t if dt is None else t.to(dt)


def _dkdv(case, **kw):
    import torch
    from lwm_amd import ops
    q, k, v, do = (_dev(t, torch.bfloat16) for t in case.operands(False))
    out, lse, *_ = K.reference(case.name)
    ckw = dict(case.kw)
    for n, dt in (("seg_q", torch.int32), ("seg_k", torch.int32), ("key_valid", torch.uint8)):
        if ckw.get(n) is not None:
            ckw[n] = _dev(ckw[n], dt)
    lse_d = _dev(lse)
    delta = ops.attn_bwd_delta(_dev(out, torch.bfloat16), do, lse_d)
    dk, dv = ops.attn_bwd_dkdv_block(q, k, v, do, lse_d, delta, **ckw, **kw)
    torch.cuda.synchronize()
    return dk, dv


@pytest.mark.parametrize("case", K.CASES, ids=repr)
def test_dkdv_vs_oracle(case):
    import torch
    dk, dv = _dkdv(case)
    K.verify_dkdv(case, dk.float().cpu().numpy(), dv.float().cpu().numpy())
    dk2, dv2 = _dkdv(case)
    assert torch.equal(dk, dk2) and torch.equal(dv, dv2), f"{case.name}: dk / dv differ between two runs"


@pytest.mark.parametrize("carry_in", [False, True], ids=["fresh", "carry_in"])
@pytest.mark.parametrize("final", [False, True], ids=["to_acc", "final"])
def test_dkdv_carry(carry_in, final):
    import torch
    case = K.CARRY_CASE
    B, Sk, H, D = case.operands(False)[1].shape
    offset = None
    if carry_in:
        rng = np.random.default_rng(7)
        offset = [(rng.standard_normal((B, Sk, H, D)) * 0.05).astype(np.float32) for _ in range(2)]
    run = lambda: _dkdv(case, carry_in=carry_in, final=final,
                        dk_acc=_dev(offset[0]) if carry_in else None, dv_acc=_dev(offset[1]) if carry_in else None)
    dk, dv = run()
    assert dk.dtype == dv.dtype == (torch.bfloat16 if final else torch.float32)
    K.verify_dkdv(case, dk.float().cpu().numpy(), dv.float().cpu().numpy(),
                  offset=None if offset is None else [o.astype(np.float64) for o in offset])
    dk2, dv2 = run()
    assert torch.equal(dk, dk2) and torch.equal(dv, dv2)
