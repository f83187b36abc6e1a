"""The dS hand-over of the attention backward on the device, at the shapes of tests/_ds_handover_cases.py: the three
gradients against the fp64 oracle with the bound of tests/test_gpu_attention.py::test_fwd_bwd_vs_oracle, dk and dv
bit-equal with and without the workspace, bit-equal repeats, a workspace of NaNs (the consumer reads only what the
producer wrote), the fallbacks -- through the ops and through ring_backward with LWM_BWD_DS_MB=0 --, and the refusal of a
short workspace.  The kernels take the saved output and the LSE of the case's reference, so the verdict is about them
alone."""
import numpy as np
import pytest

from tests import _ds_handover_cases as H

pytestmark = pytest.mark.gpu


def _dev(a, dt=None):
    import torch
    t = torch.from_numpy(np.array(a)).cuda()      # (a copy: the shared references are read-only)
    return t if dt is None else t.to(dt)


def _operands(case):
    import torch
    from lwm_amd import ops
    q, k, v, do = (_dev(t, torch.bfloat16) for t in case.operands(False))
    out, lse, *_ = H.reference(case.name)
    kw = dict(case.kw)
    for n in ("seg_q", "seg_k"):
        if kw.get(n) is not None:
            kw[n] = _dev(kw[n], torch.int32)
    lse_d = _dev(lse)
    return q, k, v, do, lse_d, ops.attn_bwd_delta(_dev(out, torch.bfloat16), do, lse_d), kw


def _workspace(case, fill):
    import torch
    from lwm_amd._lib import lib
    return torch.full((max(H.ws_bytes(lib(), case), 16),), fill, dtype=torch.uint8, device="cuda")


def _bwd(case, ws=None, **extra):
    import torch
    from lwm_amd import ops
    q, k, v, do, lse, delta, kw = _operands(case)
    dk, dv = ops.attn_bwd_dkdv_block(q, k, v, do, lse, delta, **kw, **extra.get("kv", {}), ds_ws=ws)
    dq = ops.attn_bwd_dq_block(q, k, v, do, lse, delta, **kw, **extra.get("q", {}), ds_ws=ws)
    torch.cuda.synchronize()
    return dq, dk, dv


def _np(t):
    return t.float().cpu().numpy()


@pytest.mark.parametrize("case", H.CASES, ids=repr)
def test_handover_vs_oracle(case):
    import torch
    # 0xFFFF is a bf16 NaN: finite, correct results prove that the consumer reads only tiles the producer wrote
    dq, dk, dv = _bwd(case, _workspace(case, 0xFF))
    dq0, dk0, dv0 = _bwd(case)
    H.verify(case, _np(dq0), _np(dk0), _np(dv0), "off")
    H.verify(case, _np(dq), _np(dk), _np(dv), "on")
    assert torch.equal(dk, dk0) and torch.equal(dv, dv0), "dk / dv must not depend on the hand-over"
    H.report_dq_difference(case, _np(dq), _np(dq0))
    again = _bwd(case, _workspace(case, 0))
    assert all(torch.equal(x, y) for x, y in zip((dq, dk, dv), again)), "the hand-over is not bit-reproducible"


@pytest.mark.parametrize("name,case,carry_in", H.FALLBACKS, ids=[f[0] for f in H.FALLBACKS])
def test_fallback(name, case, carry_in):
    import torch
    B, Sq, Hh, D = case.operands(False)[0].shape
    Sk = case.operands(False)[1].shape[1]
    def extra():
        if not carry_in:
            return {}
        acc = lambda S, seed: _dev((np.random.default_rng(seed).standard_normal((B, S, Hh, D)) * 0.05).astype(np.float32))
        return dict(kv=dict(carry_in=True, dk_acc=acc(Sk, 71), dv_acc=acc(Sk, 72)), q=dict(carry_in=True, dq_acc=acc(Sq, 70)))
    ws = torch.full((1 << 16,), 0xFF, dtype=torch.uint8, device="cuda")
    on, off = _bwd(case, ws, **extra()), _bwd(case, None, **extra())
    assert all(torch.equal(x, y) for x, y in zip(on, off))
    assert bool((ws == 0xFF).all()), "an ineligible call must not touch the workspace"


def test_ring_backward_takes_the_handover_and_the_budget_switches_it_off(monkeypatch):
    import torch
    from lwm_amd import ops
    from lwm_amd.ring import HipBlockOps, SeqLayout, SingleComm, ring_backward
    case = H.CASES[1]
    q, k, v, do, lse, delta, kw = _operands(case)
    out = _dev(H.reference(case.name)[0], torch.bfloat16)
    S = q.shape[1]
    seen = []

    class Ops(HipBlockOps):
        bwd_dq = staticmethod(lambda *a, **kw: (seen.append(kw.get("ds_ws") is not None), ops.attn_bwd_dq_block(*a, **kw))[1])

    run = lambda: ring_backward(Ops, SingleComm(), q, k, v, out, [lse], do, layout=SeqLayout("contiguous", 1, S), causal=True)
    monkeypatch.delenv("LWM_BWD_DS_MB", raising=False)
    on = run()
    monkeypatch.setenv("LWM_BWD_DS_MB", "0")
    off = run()
    torch.cuda.synchronize()
    assert seen == [True, False]
    ref = _bwd(case)
    assert all(torch.equal(x, y) for x, y in zip(off, ref)), "LWM_BWD_DS_MB=0 must give the recompute kernels' bits"
    assert torch.equal(on[1], off[1]) and torch.equal(on[2], off[2])
    H.verify(case, _np(on[0]), _np(on[1]), _np(on[2]), "ring, on")


def test_short_workspace_is_refused():
    import torch
    from lwm_amd import ops
    case = H.CASES[0]
    q, k, v, do, lse, delta, kw = _operands(case)
    ws = _workspace(case, 0)
    mark = lambda t: torch.full_like(t, 7.0)
    dq, dk, dv = mark(q), mark(k), mark(v)
    for bad in (ws[:-1], ws[8:]):       # short; misaligned (and short)
        with pytest.raises(RuntimeError):
            ops.attn_bwd_dkdv_block(q, k, v, do, lse, delta, **kw, dk=dk, dv=dv, ds_ws=bad)
        with pytest.raises(RuntimeError):
            ops.attn_bwd_dq_block(q, k, v, do, lse, delta, **kw, dq=dq, ds_ws=bad)
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in (dq, dk, dv)), "a refused call must leave the outputs untouched"
    assert not bool(ws.any())
