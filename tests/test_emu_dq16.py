"""The dQ kernel (attn_bwd_dq4_kernel / _meta, 16x16x32 bf16 MFMAs) on the host emulator at the shapes of
tests/_dq16_cases.py: every element of dq against the fp64 oracle with the bound of
tests/test_gpu_attention.py::test_fwd_bwd_vs_oracle, bit-identical repeats, the f32 carry both ways.  The device runs
the same cases in tests/test_gpu_dq16.py."""
import numpy as np
import pytest

from tests import _dq16_cases as Q, _emu


def _dq(case, **kw):
    q, k, v, do = case.operands(False)
    out, lse, *_ = Q.reference(case.name)
    return _emu.attn_bwd(q, k, v, out, lse, do, **case.kw, **kw)[0]


@pytest.mark.parametrize("case", Q.CASES, ids=repr)
def test_dq_vs_oracle(case):
    Q.verify_dq(case, _dq(case))


@pytest.mark.parametrize("name", ["walk_sk320", "segments", "ragged_sk100_causal"])
def test_dq_is_deterministic(name):
    case = next(c for c in Q.CASES if c.name == name)
    assert np.array_equal(_dq(case), _dq(case))


@pytest.mark.parametrize("carry_in", [False, True], ids=["fresh", "carry_in"])
@pytest.mark.parametrize("final", [False, True], ids=["to_acc", "final"])
def test_dq_carry(carry_in, final):
    case = Q.CARRY_CASE
    q, k, v, _ = case.operands(False)
    B, Sq, H, D = q.shape
    Sk = k.shape[1]
    carry, offset = None, None
    if carry_in:
        offset = (np.random.default_rng(7).standard_normal((B, Sq, H, D)) * 0.05).astype(np.float32)
        acc = _emu.aligned((B, Sq, H, D), np.float32)
        acc[...] = offset
        carry = (acc, _emu.aligned((B, Sk, H, D), np.float32), _emu.aligned((B, Sk, H, D), np.float32))
    Q.verify_dq(case, _dq(case, carry=carry, final=final), offset=None if offset is None else offset.astype(np.float64))
