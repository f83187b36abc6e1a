"""The dK/dV kernel (attn_bwd_dkdv4_kernel / _meta, 16x16x32 bf16 MFMAs) on the host emulator at the shapes of
tests/_dkdv16_cases.py: every element of dk and dv against the fp64 oracle with the bound of
tests/test_gpu_attention.py::test_fwd_bwd_vs_oracle, exact zeros for keys that no query sees, bit-identical repeats, the
f32 carries both ways.  The device runs the same cases in tests/test_gpu_dkdv16.py."""
import numpy as np
import pytest

from tests import _dkdv16_cases as K, _emu


def _dkdv(case, **kw):
    q, k, v, do = case.operands(False)
    out, lse, *_ = K.reference(case.name)
    return _emu.attn_bwd(q, k, v, out, lse, do, **case.kw, **kw)[1:]


@pytest.mark.parametrize("case", K.CASES, ids=repr)
def test_dkdv_vs_oracle(case):
    K.verify_dkdv(case, *_dkdv(case))


@pytest.mark.parametrize("name", ["walk_sq320", "segments", "ragged_sq100_causal"])
def test_dkdv_is_deterministic(name):
    case = next(c for c in K.CASES if c.name == name)
    a, b = _dkdv(case), _dkdv(case)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("carry_in", [False, True], ids=["fresh", "carry_in"])
@pytest.mark.parametrize("final", [False, True], ids=["to_acc", "final"])
def test_dkdv_carry(carry_in, final):
    case = K.CARRY_CASE
    q, k, v, _ = case.operands(False)
    B, Sq, H, D = q.shape
    Sk = k.shape[1]
    offset = None

    def run():
        carry = None
        if carry_in:
            accs = [_emu.aligned((B, Sk, H, D), np.float32) for _ in range(2)]
            for a, o in zip(accs, offset):
                a[...] = o
            carry = (_emu.aligned((B, Sq, H, D), np.float32), *accs)
        dk, dv = _dkdv(case, carry=carry, final=final)
        return np.array(dk), np.array(dv)

    if carry_in:
        rng = np.random.default_rng(7)
        offset = [(rng.standard_normal((B, Sk, H, D)) * 0.05).astype(np.float32) for _ in range(2)]
    dk, dv = run()
    assert dk.dtype == np.float32 and dv.dtype == np.float32
    K.verify_dkdv(case, dk, dv, offset=None if offset is None else [o.astype(np.float64) for o in offset])
    again = run()
    assert np.array_equal(dk, again[0]) and np.array_equal(dv, again[1])
