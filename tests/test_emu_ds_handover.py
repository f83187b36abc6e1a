"""The dS hand-over of the attention backward on the host emulator, at the shapes of tests/_ds_handover_cases.py: the
three gradients against the fp64 oracle with the bound of tests/test_gpu_attention.py::test_fwd_bwd_vs_oracle, dk and dv
bit-equal with and without the workspace, bit-equal repeats, a workspace of NaNs (the consumer reads only what the
producer wrote), the fallbacks, and the refusal of a short workspace.  The device runs the same cases in
tests/test_gpu_ds_handover.py."""
import ctypes as C
import functools

import numpy as np
import pytest

from lwm_amd import _capi
from tests import _ds_handover_cases as H, _emu

EINVAL = -1


def _bwd(case, ws=None, ws_bytes=None, carry_in=False, fill=None):
    """(rc of dkdv, rc of dq, dq, dk, dv as bf16 bits); ws: None or a uint8 array"""
    L = _emu.lib()
    q, k, v, do = case.operands(False)
    out, lse, *_ = H.reference(case.name)
    qb, kb, vb, ob, dob = (_emu.bf16_array(t) for t in (q, k, v, out, do))
    B, Sq, Hh, D = q.shape
    Sk = k.shape[1]
    a, keep = _emu.base_args(qb, kb, vb, causal=case.kw.get("causal", True), q_start=case.kw.get("q_start", 0),
                             k_start=case.kw.get("k_start", 0), seg_q=case.kw.get("seg_q"), seg_k=case.kw.get("seg_k"),
                             key_valid=None, scale=None)
    lse_a = _emu.aligned((B, Hh, Sq), np.float32)
    lse_a[...] = lse
    delta = _emu.aligned((L.lwm_attn_bwd_delta_bytes(B, Hh, Sq) // 4,), np.float32)
    dq, dk, dv = (_emu.aligned((B, Sq, Hh, D), np.uint16), _emu.aligned((B, Sk, Hh, D), np.uint16), _emu.aligned((B, Sk, Hh, D), np.uint16))
    if fill is not None:
        for t in (dq, dk, dv):
            t[...] = fill
    accs = [_emu.aligned((B, S, Hh, D), np.float32) for S in (Sq, Sk, Sk)]
    for i, t in enumerate(accs):
        t[...] = (np.random.default_rng(70 + i).standard_normal(t.shape) * 0.05).astype(np.float32)
    a.out, a.dout = _emu._t4(ob), _emu._t4(dob)
    a.dq, a.dk, a.dv = _emu._t4(dq), _emu._t4(dk), _emu._t4(dv)
    a.lse, a.delta, a.delta_bytes = lse_a.ctypes.data, delta.ctypes.data, delta.nbytes
    a.dq_acc, a.dk_acc, a.dv_acc = (t.ctypes.data for t in accs)
    a.final_out, a.carry_in = 1, int(carry_in)
    if ws is not None:
        a.ds_ws, a.ds_ws_bytes = ws.ctypes.data, ws.nbytes if ws_bytes is None else ws_bytes
    _capi.check(L, L.lwm_attn_bwd_delta(C.byref(a), None), "lwm_attn_bwd_delta")
    rc_kv = L.lwm_attn_bwd_dkdv(C.byref(a), None)
    rc_q = L.lwm_attn_bwd_dq(C.byref(a), None)
    return rc_kv, rc_q, dq, dk, dv


def _workspace(case, fill=0):
    n = H.ws_bytes(_emu.lib(), case)
    ws = _emu.aligned((max(n, 16),), np.uint8)
    ws[...] = fill
    return ws


def _f(bits):
    return _emu.from_bf16_bits(bits)


@functools.lru_cache(maxsize=None)
def _off(name):
    case = next(c for c in H.CASES if c.name == name)
    rc_kv, rc_q, dq, dk, dv = _bwd(case)
    assert rc_kv == 0 and rc_q == 0
    return dq, dk, dv


@pytest.mark.parametrize("case", H.CASES, ids=repr)
def test_workspace_size(case):
    assert H.ws_bytes(_emu.lib(), case) == H.expected_ws_bytes(case)


@pytest.mark.parametrize("case", H.CASES, ids=repr)
def test_handover_vs_oracle(case):
    # the workspace starts as NaNs (0xFFFF is a bf16 NaN): finite, correct results prove that the consumer reads only
    # tiles the producer wrote
    rc_kv, rc_q, dq, dk, dv = _bwd(case, _workspace(case, 0xFF))
    assert rc_kv == 0 and rc_q == 0
    dq0, dk0, dv0 = _off(case.name)
    H.verify(case, _f(dq0), _f(dk0), _f(dv0), "off")
    H.verify(case, _f(dq), _f(dk), _f(dv), "on")
    assert np.array_equal(dk, dk0) and np.array_equal(dv, dv0), "dk / dv must not depend on the hand-over"
    H.report_dq_difference(case, _f(dq), _f(dq0))
    # bit-equal repeat
    again = _bwd(case, _workspace(case, 0))
    assert all(np.array_equal(x, y) for x, y in zip((dq, dk, dv), again[2:]))


@pytest.mark.parametrize("name,case,carry_in", H.FALLBACKS, ids=[f[0] for f in H.FALLBACKS])
def test_fallback(name, case, carry_in):
    ws = _emu.aligned((1 << 16,), np.uint8)
    ws[...] = 0xFF
    on = _bwd(case, ws, carry_in=carry_in)
    off = _bwd(case, None, carry_in=carry_in)
    assert on[:2] == (0, 0) and off[:2] == (0, 0)
    assert all(np.array_equal(x, y) for x, y in zip(on[2:], off[2:]))
    assert (ws == 0xFF).all(), "an ineligible call must not touch the workspace"


def test_short_workspace_is_refused():
    case = H.CASES[0]
    ws = _workspace(case)
    rc_kv, rc_q, dq, dk, dv = _bwd(case, ws, ws_bytes=ws.nbytes - 1, fill=0x1234)
    assert rc_kv == EINVAL and rc_q == EINVAL
    assert all((t == 0x1234).all() for t in (dq, dk, dv)), "a refused call must leave the outputs untouched"
    assert not ws.any()
    rc_kv, rc_q, *_ = _bwd(case, ws[8:], ws_bytes=ws.nbytes)       # misaligned
    assert rc_kv == EINVAL and rc_q == EINVAL
