"""The dQ kernel at the smallest shapes that reach each of its paths: case table and verdict shared by the host emulator
(tests/test_emu_dq16.py) and the device (tests/test_gpu_dq16.py).  TEST INFRASTRUCTURE ONLY.

The kernel walks the keys in steps of 64 (two units of 32 keys x the wave's 32 queries, each unit cut into 16 x 16
tiles for v_mfma_f32_16x16x32_bf16); a workgroup holds 128 queries, a wave 32.  Sk = 32 .. 320 gives walks of 1, 1, 2,
3 and 5 steps: the short-walk branch (fewer than three steps, nothing pipelined), the first piped step, the steady loop
and the drain; an Sk that is no multiple of 64, segment ids or key_valid select the `_meta` kernel.

Cases are tests/_attn_cases.py's Case objects (its builders, and its strided pair as the B = 2 instance).  The bound is
the one tests/test_gpu_attention.py::test_fwd_bwd_vs_oracle holds dq to: tests/_parity.py::check_dq against the fp64
oracle -- per row against the gradient for the saved (bf16) output, globally against the exact one; every element of
dq takes part."""
import functools

import numpy as np

from oracle import attention_ref as R
from tests import _attn_cases as A, _parity

Case, _qkvdo = A.Case, A._qkvdo


def _walk_cases():
    out = []
    for Sk in (32, 64, 128, 192, 320):
        # every key visible to every query: the whole walk, no mask code (Sk = 32: the ragged `_meta` kernel)
        out.append(Case(f"walk_sk{Sk}", *_qkvdo(1, 64, Sk, 2, 900 + Sk), dict(causal=False)))
    for Sk in (128, 320):
        # the diagonal: the units that need the causal mask, walks that end early for the first q block
        out.append(Case(f"causal_sk{Sk}", *_qkvdo(1, Sk, Sk, 2, 950 + Sk), dict(causal=True)))
    return out


def _shape_cases():
    out = []
    # a ragged last tile (Sk % 64 = 36), bare and below the diagonal
    out.append(Case("ragged_sk100", *_qkvdo(1, 64, 100, 2, 1000), dict(causal=False)))
    out.append(Case("ragged_sk100_causal", *_qkvdo(1, 64, 100, 2, 1001), dict(causal=True, q_start=36)))
    out.append(Case("ragged_sk228_causal", *_qkvdo(1, 64, 228, 2, 1002), dict(causal=True, q_start=164)))     # n = 4, ragged tail behind a piped walk
    # a wave past the end of the queries (Sq = 40: wave 1 holds 8 rows, waves 2 and 3 none)
    out.append(Case("sq40", *_qkvdo(1, 40, 128, 2, 1010), dict(causal=True, q_start=88)))
    # an off-diagonal block of a ring: position offsets on both sides
    out.append(Case("offdiag_causal", *_qkvdo(1, 64, 160, 2, 1020), dict(causal=True, q_start=512, k_start=256)))
    out.append(Case("offdiag_full", *_qkvdo(1, 64, 160, 2, 1021), dict(causal=False, q_start=512, k_start=256)))
    out.append(Case("offdiag_crossing", *_qkvdo(1, 64, 160, 2, 1022), dict(causal=True, q_start=70, k_start=3)))
    return out


def _mask_cases():
    out = []
    # packed documents: keys 0..63 are one document (a segment-uniform step), the cuts at 100 and 200 fall inside steps
    seg = A._segments(1, 256, cuts=(64, 100, 200))
    out.append(Case("segments", *_qkvdo(1, 256, 256, 2, 1030), dict(causal=True, seg_q=seg, seg_k=seg)))
    out.append(Case("key_valid", *_qkvdo(1, 64, 192, 2, 1040), dict(causal=False, key_valid=A._sparse_valid(1, 192, 13, p=0.3))))
    # rows with no visible key: the first 32 queries lie before every key
    out.append(Case("empty_rows", *_qkvdo(1, 64, 64, 2, 1050), dict(causal=True, q_start=0, k_start=32), empty_rows=64))
    kv = np.ones((1, 128), np.uint8)
    kv[:, :40] = 0
    out.append(Case("empty_rows_meta", *_qkvdo(1, 64, 128, 2, 1051), dict(causal=True, key_valid=kv), empty_rows=80))
    return out


def _map_cases():
    # the two branches of the block -> (q block, head, batch) map: B * H a multiple of 8 or not; more than one q block
    return [Case("map_h8", *_qkvdo(1, 256, 128, 8, 1060), dict(causal=True, q_start=0)),
            Case("map_h2", *_qkvdo(1, 256, 128, 2, 1061), dict(causal=True, q_start=0))] + A.strided_cases()       # (B = 2)


CASES = _walk_cases() + _shape_cases() + _mask_cases() + _map_cases()
CARRY_CASE = next(c for c in CASES if c.name == "walk_sk192")


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (out saved as bf16 values, lse, dq for the saved output, exact dq, rows with no visible key): computed once"""
    case = next(c for c in CASES if c.name == name)
    q, k, v, do = case.operands(False)
    ro, rl = R.dense_attention(q, k, v, **case.kw)
    out_saved = R.round_bf16(ro.astype(np.float32))
    rq_saved, _, _, rq = R.dense_attention_bwd(q, k, v, do, out_saved=out_saved, **case.kw)
    empty = ~A.visibility(case, q.shape[1], k.shape[1], q.shape[0]).any(axis=2)
    if case.empty_rows is not None:
        assert int(empty.sum()) * q.shape[2] == case.empty_rows, (name, int(empty.sum()))
    for a in (out_saved, rq_saved, rq):
        a.setflags(write=False)
    return out_saved, rl.astype(np.float32), rq_saved, rq, empty


def verify_dq(case, dq, offset=None):
    """dq: what the kernel wrote, float; offset: what it was asked to add onto (the f32 carry)"""
    _, _, rq_saved, rq, empty = reference(case.name)
    dq = np.asarray(dq, np.float64)
    assert not np.isnan(dq).any(), f"{case.name}: NaN in dq"
    if offset is not None:
        rq_saved, rq = rq_saved + offset, rq + offset
    elif empty.any():
        assert not dq[empty].any(), f"{case.name}: rows with no visible key must be 0"
    g = np.abs(dq - rq).max() / max(np.abs(rq).max(), 1e-9)
    print(f"{case.name}.dq: max|err| / max|ref| = {g:.3e} (bound {_parity.TOL})")
    _parity.check_dq(f"{case.name}.dq", dq, rq_saved, rq)
