"""The dS hand-over of the attention backward (attn_bwd_dkdv4_ds_kernel -> workspace -> attn_bwd_dq_ds_kernel) at the
smallest shapes that reach each of its paths: case table, references and verdicts shared by the host emulator
(tests/test_emu_ds_handover.py) and the device (tests/test_gpu_ds_handover.py).  TEST INFRASTRUCTURE ONLY.

The producer walks the queries in steps of 64 per 128-key block and stores one 4-KiB tile per (step, wave); the consumer
holds 256 queries per workgroup, 64 per wave, and walks the keys in steps of 32 -- one tile per step and wave.

  diag_s128        one key block, the diagonal only: a two-step walk (the producer's short-walk branch), the consumer's
                   waves 0 and 1 stop at different key steps, waves 2 and 3 hold no query
  causal_s384      B = 2, H = 2: key-block walks of 6, 4 and 2 steps (the pipelined loop, its two tail steps, the short
                   branch), a second consumer workgroup with 128 rows, tiles above the diagonal that do not exist
  rect_256x512     not causal, Sq != Sk: every tile exists
  offdiag_256x512  causal with q_start = 256, k_start = 0: whole tiles below a diagonal away from the origin
Ineligible calls, which must run exactly as without a workspace: Sk = 192 (no multiple of 128), segment ids, carry_in.

The bound is the one tests/test_gpu_attention.py::test_fwd_bwd_vs_oracle holds the gradients to (tests/_parity.py: check
for dk and dv, check_dq for dq) against the fp64 oracle."""
import functools

import numpy as np

from oracle import attention_ref as R
from tests import _attn_cases as A, _parity

Case, _qkvdo = A.Case, A._qkvdo

CASES = [
    Case("diag_s128", *_qkvdo(1, 128, 128, 1, 2000), dict(causal=True)),
    Case("causal_s384", *_qkvdo(2, 384, 384, 2, 2010), dict(causal=True)),
    Case("rect_256x512", *_qkvdo(1, 256, 512, 2, 2020), dict(causal=False)),
    Case("offdiag_256x512", *_qkvdo(1, 256, 512, 2, 2030), dict(causal=True, q_start=256, k_start=0)),
]
_SEG = A._segments(1, 256, cuts=(64, 100, 200))
# (name, case, carry_in)
FALLBACKS = [
    ("sk192", Case("fb_sk192", *_qkvdo(1, 128, 192, 2, 2040), dict(causal=False)), False),
    ("segment_ids", Case("fb_segments", *_qkvdo(1, 256, 256, 2, 2050), dict(causal=True, seg_q=_SEG, seg_k=_SEG)), False),
    ("carry_in", Case("fb_carry", *_qkvdo(1, 128, 128, 2, 2060), dict(causal=True)), True),
]
_ALL = {c.name: c for c in CASES + [f[1] for f in FALLBACKS]}


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (out saved as bf16 values, lse, dq for the saved output, exact dq, dk, dv): computed once, read-only"""
    case = _ALL[name]
    q, k, v, do = case.operands(False)
    ro, rl = R.dense_attention(q, k, v, **case.kw)
    out_saved = R.round_bf16(ro.astype(np.float32))
    rq_saved, rk, rv, rq = R.dense_attention_bwd(q, k, v, do, out_saved=out_saved, **case.kw)
    lse = rl.astype(np.float32)
    for a in (out_saved, lse, rq_saved, rq, rk, rv):
        a.setflags(write=False)
    return out_saved, lse, rq_saved, rq, rk, rv


def ws_bytes(lib, case):
    """lwm_attn_bwd_ds_bytes of the case (0: not eligible by shape)"""
    q, k, _, _ = case.operands(False)
    B, Sq, H, _ = q.shape
    return lib.lwm_attn_bwd_ds_bytes(B, H, Sq, k.shape[1], int(case.kw.get("causal", True)), case.kw.get("q_start", 0),
                                     case.kw.get("k_start", 0))


def expected_ws_bytes(case):
    """the visited (64 queries x 32 keys) tiles, counted one by one"""
    q, k, _, _ = case.operands(False)
    B, Sq, H, _ = q.shape
    tiles = 0
    for kbi in range(k.shape[1] // 128):
        for st in range(Sq // 64):
            if not case.kw.get("causal", True) or case.kw.get("q_start", 0) + 64 * st + 63 >= case.kw.get("k_start", 0) + 128 * kbi:
                tiles += 4
    return B * H * tiles * 4096


def verify(case, dq, dk, dv, tag):
    """every element of the three gradients against the oracle; prints each figure before it asserts"""
    _, _, rq_saved, rq, rk, rv = reference(case.name)
    for n, got, ref in (("dq", dq, rq), ("dk", dk, rk), ("dv", dv, rv)):
        got = np.asarray(got, np.float64)
        assert np.isfinite(got).all(), f"{case.name} [{tag}]: {n} is not finite"
        g = np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-9)
        print(f"{case.name} [{tag}] {n}: max|err| / max|ref| = {g:.3e} (bound {_parity.TOL})")
    _parity.check_dq(f"{case.name}.dq [{tag}]", dq, rq_saved, rq)
    _parity.check(f"{case.name}.dk [{tag}]", dk, rk)
    _parity.check(f"{case.name}.dv [{tag}]", dv, rv)


def report_dq_difference(case, dq_on, dq_off):
    """dq with the hand-over against dq without: reported, not asserted (both are held to the oracle bound)"""
    a, b = np.asarray(dq_on, np.float64), np.asarray(dq_off, np.float64)
    rel = np.abs(a - b).max() / max(np.abs(b).max(), 1e-9)
    print(f"{case.name}: dq on vs off: max|diff| / max|dq| = {rel:.3e}, {int((a != b).sum())} of {a.size} elements differ")
