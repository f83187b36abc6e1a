"""No tensor reaches the C library unchecked (the device half of tests/test_op_boundary.py).

Per row of tests/_boundary.py: one well-formed call with device tensors through the REAL library, then -- under the
tripwire library, so that a missing check fails an assertion instead of handing a bad pointer to a kernel -- every bad
call of the row, each of which must raise ValueError before the library is touched.  Nothing here launches a kernel on
a malformed operand."""
import numpy as np
import pytest

from oracle import llama_ops_ref as R
from tests import _boundary as Bd

pytestmark = pytest.mark.gpu

ROWS = Bd.table()
CASES = Bd.cases()


@pytest.mark.parametrize("row", ROWS, ids=[r.name for r in ROWS])
def test_good_call_runs_on_the_device(row):
    import torch
    row.call(row.make("cuda"))
    torch.cuda.synchronize()


@pytest.mark.parametrize("row,name,edit", CASES, ids=[f"{r.name}: {n}" for r, n, _ in CASES])
def test_bad_call_is_refused_before_the_library(row, name, edit):
    from lwm_amd._lib import lib
    kw = row.make("cuda")
    edit(kw, "cuda")
    with Bd.tripwire(lib()) as wire:
        with pytest.raises(ValueError):
            row.call(kw)
    assert wire.reached == []


def _np(t):
    return t.detach().float().cpu().numpy()


def test_rope_takes_one_row_of_positions_for_the_whole_batch():
    """An HF-style (1,S) position_ids with B = 2: the reference's jnp.take(freqs_cis, position_ids) broadcasts it over the
    batch (lwm/llama.py:515).  apply_rotary_emb and qkv_rope give the bits of the (B,S)-expanded call, and match the
    oracle at the tolerance of tests/test_gpu_llama_ops.py::test_rope_fwd_bwd (one bf16 ulp, 2^-7 of max|ref|).  The
    positions are a ramp that is not arange and differs from row to row of a (B,S) reading: a kernel that read
    pos[b * S + s] from the (1,S) buffer would rotate batch row 1 by other (clamped) positions."""
    import torch
    from lwm_amd.llama_ops import apply_rotary_emb, precompute_freqs_cis, qkv_rope
    B, S, H, D, d, max_pos = 2, 333, 2, 128, 256, 4096
    g = torch.Generator().manual_seed(1)
    rnd = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16).cuda()
    pos1 = ((torch.arange(S) * 7 + 13) % max_pos).to(torch.int32)[None]           # (1, S)
    posB = pos1.expand(B, S).contiguous()
    tab = precompute_freqs_cis(D, max_pos, 10000.0, device="cuda")
    fc = R.precompute_freqs_cis(D, max_pos, 10000.0)
    xq, xk = rnd(B, S, H, D), rnd(B, S, H, D)
    for p1 in (pos1.cuda(), pos1.to(torch.int64).cuda()):
        q1, k1 = apply_rotary_emb(xq, xk, tab, p1)
        qB, kB = apply_rotary_emb(xq, xk, tab, posB.cuda())
        assert torch.equal(q1, qB) and torch.equal(k1, kB)
    for got, x in ((q1, xq), (k1, xk)):
        ref = R.apply_rotary_emb(_np(x), fc, posB.numpy())
        assert np.abs(_np(got) - ref).max() <= 2 ** -7 * np.abs(ref).max()
    assert not torch.equal(q1[0], apply_rotary_emb(xq, xk, tab)[0][0])              # (the ramp is not the default arange)
    # the fused projection: the same three launches' worth of work in one operator
    x, wq, wk, wv = rnd(B, S, d), rnd(d, H * D) * 0.06, rnd(d, H * D) * 0.06, rnd(d, H * D) * 0.06
    f1 = qkv_rope(x, wq, wk, wv, tab, pos1.cuda(), H)
    fB = qkv_rope(x, wq, wk, wv, tab, posB.cuda(), H)
    assert all(torch.equal(a, b) for a, b in zip(f1, fB))
    # position 0 rotates by (cos, sin) = (1, 0): the projections as the kernel saw them
    pre = qkv_rope(x, wq, wk, wv, tab, torch.zeros(1, S, dtype=torch.int32, device="cuda"), H)
    assert torch.equal(pre[2], f1[2])
    for got, unrot in zip(f1[:2], pre[:2]):
        ref = R.apply_rotary_emb(_np(unrot), fc, posB.numpy())
        assert np.abs(_np(got) - ref).max() <= 2 ** -7 * np.abs(ref).max()
        assert not torch.equal(got, unrot)
    torch.cuda.synchronize()
