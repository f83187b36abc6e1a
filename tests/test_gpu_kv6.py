"""The 6-bit (MXFP6 e2m3) KV cache on MI355X.  First the packing order: every code at every position of a block through
the decode kernel's conversion instruction, against kv6_dequant.  Then the quantising write bit for bit against the numpy
restatement (tests/_kv6_ref.py), the decode kernel against the fp64 oracle and against the bf16 decode kernel on the same
numbers, its mask behaviour, the block kernel torch.equal with the bf16 split-K kernel on a bf16 copy of the dequantised
cache, and the model-level wiring of generate(kv_dtype="fp6"[, prefill_chunk=N]) on the tiny HF fixture.  What
quantisation itself costs is measured and printed beside the 8-bit and the 4-bit cache's, not gated
(profiles/r23_kv6_decode.md records it); the gated statement about precision is elementwise (tests/test_emu_kv6.py).

Bounds are those of tests/test_gpu_kv4.py and tests/test_gpu_kv8_prefill.py: decode and block kernel against the oracle
2e-2 of max / lse 2e-3; two forms of the same attention 1.6e-2 of max; graph against eager logits 1e-3 of max; blocks
against one token at a time 2e-2 of max.  The oracle and the bf16 kernels get the DEQUANTISED cache, so quantisation
error is in no gated comparison."""
import functools
import os
import sys

import numpy as np
import pytest

from oracle import attention_ref as R
from tests import _kv6_ref as K6

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))


def _rand(shape, seed, mag=1.0):
    import torch
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * mag).to(torch.bfloat16)


def _np(t):
    return t.detach().float().cpu().numpy()


def _quant(x):
    """bf16 (B,S,H,128) device tensor -> (e2m3 blocks u8 (B,S,H,96), e8m0 bytes u8 (B,S,H,4)) through kv6_cache_write"""
    import torch
    from lwm_amd import kv6
    B, S, H, D = x.shape
    q = torch.full((B, S, H, 96), 0xAB, dtype=torch.uint8, device=x.device)
    s = torch.full((B, S, H, 4), 0xAB, dtype=torch.uint8, device=x.device)
    kv6.kv6_cache_write(q, s, x.contiguous(), dst_row0=0)
    return q, s


def _decode(q, kq, ks, vq, vs, mask, splits):
    from lwm_amd import kv6, ops
    return ops.attn_combine(*kv6.attn_decode_kv6(q, kq, ks, vq, vs, k_splits=splits, dense_mask=mask))


# ---------------------------------------------------------------- first: the packing order
def test_packing_order_of_the_conversion_instruction():
    """Key row c holds code (position + c) % 64 at every position of every block, each block under another scale byte.
    Values: one key per decode call is visible, so the output IS that key's value row as the kernel converted it
    (softmax weight exactly 1; f32 partials).  Keys: a one-hot query picks one element of every key, and the lse of a
    single visible key is its score.  Both against kv6_dequant: a conversion that read its registers in another order
    than the format states would permute elements here."""
    import torch
    from lwm_amd import kv6
    pos = np.arange(32)
    cd = np.stack([np.tile((pos + c) % 64, 4) for c in range(64)]).astype(np.uint8)          # (64 keys, 128)
    rows = torch.from_numpy(K6.pack(cd)).cuda().reshape(1, 64, 1, 96)
    sc = torch.tensor([125, 126, 127, 129], dtype=torch.uint8, device="cuda").expand(1, 64, 1, 4).contiguous()
    want = kv6.kv6_dequant(rows, sc).float()                                                 # (1, 64, 1, 128)
    assert np.array_equal(_np(want).astype(np.float64), K6.dequant(K6.pack(cd), np.broadcast_to([125, 126, 127, 129], (64, 4))).reshape(1, 64, 1, 128))
    q = torch.zeros(1, 1, 1, 128, dtype=torch.bfloat16, device="cuda")
    got_v = torch.empty(64, 128, device="cuda")
    for j in range(64):
        mask = torch.zeros(1, 1, 64, dtype=torch.uint8, device="cuda")
        mask[0, 0, j] = 1
        o, _ = kv6.attn_decode_kv6(q, rows, sc, rows, sc, k_splits=1, dense_mask=mask)
        got_v[j] = o[0, 0, 0, 0]
    assert torch.equal(got_v, want[0, :, 0]), torch.nonzero(got_v != want[0, :, 0])[:8]
    # keys: q = e_d (scale 1): the score of key j is element d of its row, and with one visible key lse = score
    got_k = torch.empty(64, 128, device="cuda")
    for d in range(128):
        q1 = torch.zeros(1, 1, 1, 128, dtype=torch.bfloat16, device="cuda")
        q1[..., d] = 1.0
        for j in (d % 64, (d + 17) % 64, (d + 40) % 64):
            mask = torch.zeros(1, 1, 64, dtype=torch.uint8, device="cuda")
            mask[0, 0, j] = 1
            _, l = kv6.attn_decode_kv6(q1, rows, sc, rows, sc, k_splits=1, dense_mask=mask, scale=1.0)
            got_k[j, d] = l[0, 0, 0, 0]
            # (lse = (m + log2 l) ln 2 with m = score * log2 e: within a few f32 ulps of the score, far below a code's step)
            w = want[0, j, 0, d].item()
            assert abs(got_k[j, d].item() - w) <= 1e-5 * max(1.0, abs(w)), (j, d, got_k[j, d].item(), w)


# ---------------------------------------------------------------- quantiser
def test_quantiser_bit_for_bit():
    """4096 random rows over magnitudes 1e-6 .. 1e3 and the edge rows of tests/_kv6_ref.edge_rows: blocks and scale bytes
    equal the restatement, at H = 32 and H = 1"""
    import torch
    from lwm_amd import kv6
    rng = np.random.default_rng(0)
    mags = 10.0 ** rng.uniform(-6, 3, size=(4096, 1))
    x = np.concatenate([R.round_bf16((rng.standard_normal((4096, 128)) * mags).astype(np.float32)), K6.edge_rows(rng)])
    x = np.concatenate([x, np.zeros((-x.shape[0] % 32, 128), np.float32)])
    for H in (32, 1):
        src = x.reshape(1, -1, H, 128)
        q, s = _quant(torch.from_numpy(src).to(torch.bfloat16).cuda())
        rq, rs = K6.quantise(src)
        assert np.array_equal(s.cpu().numpy(), rs), np.argwhere(s.cpu().numpy() != rs)[:8]
        bad = np.argwhere(K6.codes(q.cpu().numpy()) != K6.codes(rq))
        assert bad.size == 0, [(tuple(i), K6.codes(q.cpu().numpy())[tuple(i)], K6.codes(rq)[tuple(i)], src[tuple(i)]) for i in bad[:8]]
        assert np.array_equal(q.cpu().numpy(), rq)
    # the yardstick on the device: dequantised bytes are the restatement's numbers exactly (wherever they are normal
    # numbers below the top of bf16)
    ok = (rs >= 4).all(-1) & (np.abs(src).max(-1) < 1e38)
    assert ok.sum() >= ok.size - 5
    d = _np(kv6.kv6_dequant(q, s)).astype(np.float64)
    assert np.array_equal(d[ok], K6.dequant(rq, rs)[ok])


def test_write_at_equals_host_index_and_skips_outside_rows():
    import torch
    from lwm_amd import kv6
    B, S, H, n = 2, 12, 4, 4
    src = _rand((B, 6, H, 128), 5, 3.0).cuda()
    q, s = _quant(src)
    fresh = lambda: (torch.full((B, S, H, 96), 0xAB, dtype=torch.uint8, device="cuda"),
                     torch.full((B, S, H, 4), 0xAB, dtype=torch.uint8, device="cuda"))
    dev = lambda i: torch.tensor([i], dtype=torch.int32, device="cuda")
    ch, sh = fresh()
    kv6.kv6_cache_write(ch, sh, src, dst_row0=5, src_row0=1, nrows=n)
    cd, sd = fresh()
    kv6.kv6_cache_write_at(cd, sd, src, dev(3), row_offset=2, src_row0=1, nrows=n)
    assert torch.equal(ch, cd) and torch.equal(sh, sd)
    assert torch.equal(ch[:, 5:9], q[:, 1:5]) and torch.equal(sh[:, 5:9], s[:, 1:5])
    assert (ch[:, :5] == 0xAB).all() and (ch[:, 9:] == 0xAB).all() and (sh[:, :5] == 0xAB).all() and (sh[:, 9:] == 0xAB).all()
    cd, sd = fresh()
    kv6.kv6_cache_write_at(cd, sd, src, dev(10), nrows=n)                    # rows 10, 11 land; 12, 13 are outside
    assert torch.equal(cd[:, 10:12], q[:, 0:2]) and torch.equal(sd[:, 10:12], s[:, 0:2])
    assert (cd[:, :10] == 0xAB).all() and (sd[:, :10] == 0xAB).all()
    cd, sd = fresh()
    kv6.kv6_cache_write_at(cd, sd, src, dev(3), row_offset=-S, nrows=n)      # another shard's rows: nothing is written
    assert (cd == 0xAB).all() and (sd == 0xAB).all()
    kv6.kv6_cache_write_at(cd, sd, src, dev(3), row_offset=-5, nrows=n)      # rows -2, -1, 0, 1
    assert torch.equal(cd[:, 0:2], q[:, 2:4]) and (cd[:, 2:] == 0xAB).all() and (sd[:, 2:] == 0xAB).all()
    assert torch.equal(sd[:, 0:2], s[:, 2:4])


# ---------------------------------------------------------------- decode kernel
@pytest.mark.parametrize("B,K,H,splits,cache_index", [
    (2, 4096, 4, 8, 4000),
    (1, 1000, 2, 3, 999),
    (1, 8192, 32, 16, 100),      # mostly-empty cache: whole pieces masked
    (1, 1024, 2, 1, 700),
    (1, 257, 130, 2, 256),       # more heads than slots
])
def test_decode_vs_oracle_and_vs_the_bf16_kernel(B, K, H, splits, cache_index):
    import torch
    from lwm_amd import kv6, ops
    q, k, v = _rand((B, 1, H, 128), 1).cuda(), _rand((B, K, H, 128), 2).cuda(), _rand((B, K, H, 128), 3).cuda()
    k[..., 32:64] *= 0.25                # blocks of different magnitude inside a head: a wrong scale byte or block order shows
    k[..., 64:96] *= 4.0
    v[..., 96:] *= 8.0
    am = (np.random.default_rng(4).random((B, K)) > 0.1).astype(np.uint8)
    am[:, 0] = 1
    mask = R.decode_mask(B, 1, K, cache_index, am)
    md = torch.from_numpy(mask.astype(np.uint8)).cuda()
    (kq, ks), (vq, vs) = _quant(k), _quant(v)
    out, lse = _decode(q, kq, ks, vq, vs, md, splits)
    kd, vd = kv6.kv6_dequant(kq, ks), kv6.kv6_dequant(vq, vs)
    ro, rl = R.dense_attention(_np(q), _np(kd), _np(vd), causal=False, dense_mask=mask)
    e_out, e_lse = np.abs(_np(out) - ro).max() / np.abs(ro).max(), np.abs(_np(lse) - rl).max()
    ob, lb = ops.attn_combine(*ops.attn_fwd_splitk(q, kd, vd, k_splits=splits, dense_mask=md))
    e_bf = (out.float() - ob.float()).abs().max().item() / np.abs(ro).max()
    e_lb = (lse - lb).abs().max().item()
    print(f"kv6 decode B={B} K={K} H={H} splits={splits}: vs oracle out {e_out:.3e} lse {e_lse:.3e}; vs bf16 kernel {e_bf:.3e} "
          f"lse {e_lb:.3e}")
    assert e_out <= 2e-2
    assert e_lse <= 2e-3
    assert e_bf <= 1.6e-2
    assert e_lb <= 2e-3


def test_decode_mask_behaviour():
    """garbage under the mask -- 0xFF code bytes and 0xFF scale bytes included -- leaves the outputs torch.equal; a
    hole is handled per key; nothing visible gives (0, -inf)"""
    import torch
    B, K, H = 2, 2048, 32
    q, k, v = _rand((B, 1, H, 128), 11).cuda(), _rand((B, K, H, 128), 12).cuda(), _rand((B, K, H, 128), 13).cuda()
    (kq, ks), (vq, vs) = _quant(k), _quant(v)
    mask = torch.zeros(B, 1, K, dtype=torch.uint8, device="cuda")
    mask[:, :, 7:1500] = 1
    mask[:, :, 500:600] = 0
    out, lse = _decode(q, kq, ks, vq, vs, mask, 6)
    assert torch.isfinite(out.float()).all() and torch.isfinite(lse).all()
    hid = (mask[:, 0] == 0)
    g = torch.Generator(device="cuda").manual_seed(0)
    for fill_q, fill_s in ((0xFF, 0xFF), (0x77, 0xFE), (None, None)):
        k2, s2, v2, t2 = kq.clone(), ks.clone(), vq.clone(), vs.clone()
        for c, s in ((k2, s2), (v2, t2)):
            if fill_q is None:
                c[hid] = torch.randint(0, 256, c[hid].shape, generator=g, device="cuda", dtype=torch.uint8)
                s[hid] = torch.randint(0, 256, s[hid].shape, generator=g, device="cuda", dtype=torch.uint8)
            else:
                c[hid], s[hid] = fill_q, fill_s
        o2, l2 = _decode(q, k2, s2, v2, t2, mask, 6)
        assert torch.equal(o2, out) and torch.equal(l2, lse), (fill_q, fill_s)
    full, lf = _decode(q, kq, ks, vq, vs, None, 6)
    assert not torch.equal(full, out)
    ones, lo = _decode(q, kq, ks, vq, vs, torch.ones_like(mask), 6)
    assert torch.equal(full, ones) and torch.equal(lf, lo)
    o0, l0 = _decode(q, kq, ks, vq, vs, torch.zeros_like(mask), 6)
    assert (o0 == 0).all() and torch.isneginf(l0).all()


# ---------------------------------------------------------------- block kernel
# (B, Q, idx, cache_rows, H, k_splits, left padding of batch row 0 in key_valid or None): tests/test_emu_kv6.py has the reasons
CASES = [
    (1, 3, 8, 32, 2, 1, 5),
    (2, 300, 70, 512, 2, 2, 9),
    (1, 256, 256, 1024, 8, 4, None),
    (1, 64, 1000, 1100, 3, 3, 5),
    (1, 1, 500, 512, 4, 2, 5),
    (1, 5, 60, 128, 2, 4, None),
    (1, 40, 0, 64, 1, 2, 3),
]
IDS = ["B%d-Q%d-idx%d-rows%d-H%d-splits%d" % c[:6] for c in CASES]
SPLIT = [i for i, c in enumerate(CASES) if c[5] >= 2]


def _prefill(q, kq, ks, vq, vs, Sk, idx, kv, n):
    """the partials over the first Sk rows of the caches: VIEWS of the whole cache, key_valid rows strided likewise"""
    from lwm_amd import kv6
    return kv6.attn_prefill_kv6(q, kq[:, :Sk], ks[:, :Sk], vq[:, :Sk], vs[:, :Sk], q_start=idx, k_splits=n,
                                key_valid=None if kv is None else kv[:, :Sk])


@functools.lru_cache(maxsize=None)
def _case(i):
    """inputs of case i and the kernel's answer, computed once and shared; nothing below writes to them"""
    import torch
    B, Q, idx, rows, H, n, pad = CASES[i]
    q = _rand((B, Q, H, 128), 100 + i).cuda()
    k, v = _rand((B, rows, H, 128), 200 + i, 1.5).cuda(), _rand((B, rows, H, 128), 300 + i, 0.7).cuda()
    k[..., 32:64] *= 0.25
    v[..., 96:] *= 8.0
    (kq, ks), (vq, vs) = _quant(k), _quant(v)
    kv = None
    if pad is not None:
        kv = torch.ones(B, rows, dtype=torch.uint8, device="cuda")
        kv[0, :pad] = 0
    op, lp = _prefill(q, kq, ks, vq, vs, idx + Q, idx, kv, n)
    return q, kq, ks, vq, vs, kv, op, lp


def _dequant(i):
    from lwm_amd import kv6
    B, Q, idx, rows, H, n, pad = CASES[i]
    q, kq, ks, vq, vs, kv, op, lp = _case(i)
    Sk = idx + Q
    return kv6.kv6_dequant(kq[:, :Sk], ks[:, :Sk]), kv6.kv6_dequant(vq[:, :Sk], vs[:, :Sk]), \
        (None if kv is None else kv[:, :Sk].contiguous())


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_prefill_kv6_vs_oracle(i):
    import torch
    from lwm_amd import ops
    B, Q, idx, rows, H, n, pad = CASES[i]
    q, kq, ks, vq, vs, kv, op, lp = _case(i)
    out, lse = ops.attn_combine(op, lp)
    kd, vd, kvc = _dequant(i)
    ro, rl = R.dense_attention(_np(q), _np(kd), _np(vd), causal=True, q_start=idx, key_valid=None if kvc is None else kvc.cpu().numpy())
    none = np.isneginf(rl)              # rows that see nothing: -inf exactly (-inf minus -inf is no error, it is nan)
    assert np.array_equal(np.isneginf(_np(lse)), none)
    eo, el = np.abs(_np(out) - ro).max() / np.abs(ro).max(), np.abs(_np(lse)[~none] - rl[~none]).max()
    print(f"kv6 prefill {IDS[i]}: vs oracle out {eo:.3e} of max (bound 2e-2), lse {el:.3e} (bound 2e-3)")
    assert eo <= 2e-2
    assert el <= 2e-3
    o2, l2 = _prefill(q, kq, ks, vq, vs, idx + Q, idx, kv, n)              # the same launch again: the same bits
    assert torch.equal(o2, op) and torch.equal(l2, lp)


@pytest.mark.parametrize("i", SPLIT, ids=[IDS[i] for i in SPLIT])
def test_prefill_kv6_partials_equal_the_bf16_kernel_bit_for_bit(i):
    """the staged tiles are exact, so the partials ARE those of the bf16 split-K kernel on a bf16 copy of the dequantised
    cache: pins the conversion instruction's element order, the staging, the swizzle and the scale indexing on the device"""
    import torch
    from lwm_amd import ops
    B, Q, idx, rows, H, n, pad = CASES[i]
    q, kq, ks, vq, vs, kv, op, lp = _case(i)
    kd, vd, kvc = _dequant(i)
    fo, fl = ops.attn_fwd_splitk(q, kd, vd, k_splits=n, q_start=idx, causal=True, key_valid=kvc)
    assert torch.equal(op.view(torch.int32), fo.view(torch.int32))
    assert torch.equal(lp.view(torch.int32), fl.view(torch.int32))


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_prefill_kv6_hidden_rows_reach_nothing(i):
    """rows at or past idx + Q and rows with key_valid == 0 hold 0xFF bytes with 0xFF scales, or random bytes: the same
    bits come out"""
    import torch
    B, Q, idx, rows, H, n, pad = CASES[i]
    q, kq, ks, vq, vs, kv, op, lp = _case(i)
    Sk = idx + Q
    hid = torch.zeros(B, rows, dtype=torch.bool, device="cuda")
    hid[:, Sk:] = True
    if kv is not None:
        hid |= kv == 0
    assert hid.any()
    g = torch.Generator(device="cuda").manual_seed(3)
    for fill_q, fill_s in ((0xFF, 0xFF), (0x77, 0x00), (None, None)):
        k2, s2, v2, t2 = kq.clone(), ks.clone(), vq.clone(), vs.clone()
        for c, s in ((k2, s2), (v2, t2)):
            if fill_q is None:
                c[hid] = torch.randint(0, 256, c[hid].shape, generator=g, device="cuda", dtype=torch.uint8)
                s[hid] = torch.randint(0, 256, s[hid].shape, generator=g, device="cuda", dtype=torch.uint8)
            else:
                c[hid], s[hid] = fill_q, fill_s
        o2, l2 = _prefill(q, k2, s2, v2, t2, Sk, idx, kv, n)
        assert torch.equal(o2.view(torch.int32), op.view(torch.int32)) and torch.equal(l2.view(torch.int32), lp.view(torch.int32)), \
            (fill_q, fill_s)


def test_prefill_kv6_one_query_against_the_decode_kernel():
    import torch
    from lwm_amd import kv6, ops
    i = [c[1] for c in CASES].index(1)
    B, Q, idx, rows, H, n, pad = CASES[i]
    q, kq, ks, vq, vs, kv, op, lp = _case(i)
    Sk = idx + Q
    out, lse = ops.attn_combine(op, lp)
    mask = torch.from_numpy(R.decode_mask(B, 1, Sk, idx, kv[:, :Sk].cpu().numpy()).astype(np.uint8)).cuda()
    do, dl = ops.attn_combine(*kv6.attn_decode_kv6(q, kq[:, :Sk], ks[:, :Sk], vq[:, :Sk], vs[:, :Sk], k_splits=n, dense_mask=mask))
    eo = (out.float() - do.float()).abs().max().item() / do.float().abs().max().item()
    el = (lse - dl).abs().max().item()
    print(f"block kernel against decode kernel at Q = 1: out {eo:.3e} of max (bound 1.6e-2), lse {el:.3e} (bound 2e-3)")
    assert eo <= 1.6e-2
    assert el <= 2e-3


# ---------------------------------------------------------------- model level (the tiny HF fixture)
def _model(max_positions=None):
    import hf_fixture as F
    from lwm_amd import weights as W
    from lwm_amd.llama import LLaMAForCausalLM
    hf = dict(F.HF_CONFIG) if max_positions is None else dict(F.HF_CONFIG, max_position_embeddings=max_positions)
    cfg = W.config_from_hf(hf)
    model = LLaMAForCausalLM(cfg).cuda()
    W.load_params(model, W.hf_to_lwm(F.state_dict(), cfg.num_attention_heads))
    return cfg, model


def _prompt():
    import torch
    gold = np.load(os.path.join(HERE, "golden", "hf_llama_tiny.npz"))
    seq = torch.from_numpy(gold["gen_tokens"]).cuda()
    mask = torch.from_numpy(gold["gen_mask"]).cuda()
    return seq, mask, mask.shape[1], gold["gen_scores"].shape[1]


def test_init_cache_fp6_layout():
    import torch
    cfg, model = _model()
    H = cfg.num_attention_heads
    for chunked in (False, True):
        cache = model.init_cache(2, 64, kv_dtype="fp6", chunked_prefill=chunked)
        assert len(cache) == cfg.num_hidden_layers
        for c in cache:
            for n in ("cached_key", "cached_value"):
                assert c[n].dtype == torch.uint8 and tuple(c[n].shape) == (2, 64, H, 96)
            for n in ("key_scale_e8m0", "value_scale_e8m0"):
                assert c[n].dtype == torch.uint8 and tuple(c[n].shape) == (2, 64, H, 4) and (c[n] == 127).all()
            assert "key_scale" not in c and c["cache_index"] == 0 and c.get("kv8_blocks", False) is chunked
    assert tuple(model.init_cache(2, 64, kv_dtype="fp4")[0]["cached_key"].shape) == (2, 64, H, 64)       # what it was


def test_generate_fp6_graph_equals_eager_and_what_the_cache_costs():
    import torch
    cfg, model = _model()
    seq, mask, PL, NEW = _prompt()
    kw = dict(attention_mask=mask, max_new_tokens=NEW, return_logits=True)
    eager, le = model.generate(seq[:, :PL], kv_dtype="fp6", **kw)
    graph, lg = model.generate(seq[:, :PL], kv_dtype="fp6", graph=True, **kw)
    d = (lg - le).abs().max().item() / le.abs().max().item()
    print(f"fp6 cache, graph against eager: logits differ by {d:.3e} of max")
    assert torch.equal(graph, eager)
    assert d <= 1e-3
    # the cost of quantisation, teacher forced, beside the other caches: printed, not gated
    L = PL + NEW
    ext = torch.ones(1, L, dtype=torch.int32, device="cuda")
    ext[:, :PL] = mask

    def run(kind):
        cache = model.init_cache(1, L, **({} if kind is None else dict(kv_dtype=kind)))
        pos = (mask.cumsum(-1) - 1).clamp_min(0).to(torch.int32).contiguous()
        step_in, logits = seq[:, :PL], []
        with torch.no_grad():
            for t in range(NEW):
                h = model.hidden_states(step_in, ext, None, pos, cache)
                logits.append((h[:, -1].float() @ model.lm_head.float()).cpu())
                step_in, pos = seq[:, PL + t:PL + t + 1], (pos[:, -1:] + 1).contiguous()
        return torch.stack(logits, 1)
    lb = run(None)
    for kind in ("fp8", "fp6", "fp4"):
        lq = run(kind)
        dd = ((lq - lb).abs().amax(-1) / lb.abs().max()).flatten()
        changed = int((lq.argmax(-1) != lb.argmax(-1)).sum().item())
        print(f"COST {kind} cache against the bf16 cache (teacher forced, {NEW} steps): per-step logit difference of max "
              f"{[f'{x:.2e}' for x in dd.tolist()]}; changed greedy tokens {changed} of {NEW}")


def test_seeded_sampling_and_generate_vision_with_fp6_cache():
    import torch
    from tests.test_gpu_sample import _prompts, _vision_model
    model = _vision_model(torch.bfloat16, mode="text")
    ids, am = _prompts(2, 24, 2048, 3)
    kw = dict(attention_mask=am, max_new_tokens=12, do_sample=True, temperature=0.9, top_k=50, seed=1234, kv_dtype="fp6")
    a, b = model.generate(ids, **kw), model.generate(ids, **kw)
    g, g2 = model.generate(ids, graph=True, **kw), model.generate(ids, graph=True, **kw)
    assert torch.equal(a, b) and torch.equal(g, g2)
    assert a.shape == (2, 12) and g.shape == (2, 12)
    assert not torch.equal(a, model.generate(ids, **{**kw, "seed": 99}))
    c, c2 = model.generate(ids, prefill_chunk=8, **kw), model.generate(ids, prefill_chunk=8, graph=True, **kw)
    assert c.shape == (2, 12) and c2.shape == (2, 12) and torch.equal(c, model.generate(ids, prefill_chunk=8, **kw))
    # generate_vision: eager and captured steps draw the same tokens from the same logits
    vmodel = _vision_model(torch.bfloat16)
    ids, am = _prompts(4, 40, 2048, 2)
    vm = torch.zeros_like(ids, dtype=torch.bool)
    vkw = dict(attention_mask=am, vision_masks=vm, max_new_tokens=20, temperature=1.0, top_k=100, seed=42, kv_dtype="fp6")
    e6 = vmodel.generate_vision(ids, [5.0, 5.0], graph=False, **vkw)
    g6 = vmodel.generate_vision(ids, [5.0, 5.0], graph=True, **vkw)
    assert torch.equal(e6, g6) and e6.shape[-1] == 20


PL, NEW, PAD = 40, 6, 5


def _batch(total):
    """B = 2, `total` random tokens per row, row 0 left-padded by PAD -> (tokens, mask over the tokens)"""
    import torch
    g = torch.Generator().manual_seed(11)
    seq = torch.randint(0, 384, (2, total), generator=g).cuda()
    mask = torch.ones(2, total, dtype=torch.int32, device="cuda")
    mask[0, :PAD] = 0
    return seq, mask


def test_blocks_into_a_live_fp6_cache_equal_one_token_at_a_time():
    """A 6-bit cache that takes blocks (chunked_prefill=True), fed 16 + 16 + 8 prompt tokens and 6 teacher-forced decode
    steps, against the same kind of cache fed the first 16 tokens as one block and every later prompt token one at a
    time through the decode path: the comparison and the bound of the 8-bit file's test of this name."""
    import torch
    cfg, model = _model()
    L = PL + 16
    seq, mask = _batch(PL + NEW)
    ext = torch.ones(2, L, dtype=torch.int32, device="cuda")
    ext[:, :PL] = mask[:, :PL]
    pos = (mask.cumsum(-1) - 1).clamp_min(0).to(torch.int32).contiguous()

    def run(cuts):
        cache = model.init_cache(2, L, kv_dtype="fp6", chunked_prefill=True)
        assert all(c["kv8_blocks"] is True for c in cache)
        logits = []
        with torch.no_grad():
            for a, z in zip(cuts[:-1], cuts[1:]):
                h = model.hidden_states(seq[:, a:z], ext, None, pos[:, a:z].contiguous(), cache)
                assert all(c["cache_index"] == z for c in cache)
                if z >= PL:
                    logits.append((h[:, -1].float() @ model.lm_head.float()).cpu())
        return torch.stack(logits, 1)

    tail = list(range(PL, PL + NEW + 1))
    blocks = run([0, 16, 32] + tail)
    singly = run([0] + list(range(16, PL)) + tail)
    assert blocks.shape == (2, NEW + 1, 384)
    d = ((blocks - singly).abs().amax(-1) / singly.abs().max()).flatten()
    print(f"fp6 cache, prompt in blocks 16 + 16 + 8 against one token at a time: logit difference of max, last prompt "
          f"position then {NEW} decode steps, both rows: {[f'{x:.2e}' for x in d.tolist()]} (bound 2e-2)")
    assert d.max().item() <= 2e-2


def test_generate_fp6_chunked_graph_equals_eager():
    import torch
    cfg, model = _model()
    seq, mask = _batch(PL)
    kw = dict(attention_mask=mask, max_new_tokens=16, return_logits=True, kv_dtype="fp6", prefill_chunk=16)
    eager, le = model.generate(seq, **kw)
    graph, lg = model.generate(seq, graph=True, **kw)
    d = (lg - le).abs().max().item() / le.abs().max().item()
    print(f"fp6 cache, prefill_chunk=16, graph against eager: logits differ by {d:.3e} of max (bound 1e-3)")
    assert eager.shape == (2, PL + 16)
    assert torch.equal(graph, eager)
    assert d <= 1e-3


def test_chunked_fp6_prefill_lowers_the_peak_memory():
    """a 4096-token prompt on the fixture: the prefill in blocks of 512 peaks strictly below the one-shot prefill over the
    same 6-bit cache (a condition, not a measurement: both values are printed)"""
    import torch
    cfg, model = _model(max_positions=8192)
    S = 4096
    ids = torch.randint(0, 384, (1, S), generator=torch.Generator().manual_seed(5)).cuda()
    pos = torch.arange(S, dtype=torch.int32, device="cuda")[None]
    peaks = {}
    for chunk in (S, 512):
        cache = model.init_cache(1, S + 8, kv_dtype="fp6", chunked_prefill=True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        with torch.no_grad():
            for a in range(0, S, chunk):
                h = model.hidden_states(ids[:, a:a + chunk], None, None, pos[:, a:a + chunk].contiguous(), cache)
        torch.cuda.synchronize()
        peaks[chunk] = (torch.cuda.max_memory_allocated() - base, torch.cuda.max_memory_allocated())
        assert all(c["cache_index"] == S for c in cache)
        del cache, h
    print("fp6 cache, prefill of 4096 tokens, peak bytes above the cache (and in all): " +
          "; ".join(f"block {c}: {v[0]} ({v[1]})" for c, v in peaks.items()))
    assert peaks[512][1] < peaks[S][1]


def test_refused_cases_are_named(monkeypatch):
    import torch
    from lwm_amd.llama import LLaMAForCausalLM
    from lwm_amd import weights as W
    import hf_fixture as F
    cfg, model = _model()
    with pytest.raises(ValueError, match="'fp8' or 'fp4'"):
        model.init_cache(1, 32, kv_dtype="fp5")
    f32 = LLaMAForCausalLM(W.config_from_hf(F.HF_CONFIG), dtype=torch.float32).cuda()
    with pytest.raises(NotImplementedError, match="float32"):
        f32.init_cache(1, 32, kv_dtype="fp6")
    with pytest.raises(NotImplementedError, match="float32"):
        f32.generate(torch.zeros(1, 4, dtype=torch.int64, device="cuda"), max_new_tokens=2, kv_dtype="fp6")
    # a block of tokens after the prompt into a cache that was not made for blocks
    ids = torch.randint(0, 384, (1, 8), device="cuda")
    pos = torch.arange(8, dtype=torch.int32, device="cuda")[None]
    cache = model.init_cache(1, 32, kv_dtype="fp6")
    with torch.no_grad():
        model.hidden_states(ids, None, None, pos, cache)
        with pytest.raises(NotImplementedError, match="Q > 1 at cache_index > 0"):
            model.hidden_states(ids[:, :3], None, None, pos[:, :3] + 8, cache)
    # ... and through the device-index (graph) form of a cache that takes blocks: not captured
    cache = model.init_cache(1, 32, kv_dtype="fp6", chunked_prefill=True)
    with torch.no_grad():
        model.hidden_states(ids, None, None, pos, cache)
        dcache = model.device_index_cache(cache, torch.tensor([8], dtype=torch.int32, device="cuda"))
        with pytest.raises(NotImplementedError, match="Q > 1 at cache_index > 0"):
            model.hidden_states(ids[:, :3], None, None, pos[:, :3] + 8, dcache)
    # the 4-bit cache's refusal of blocks is what it was
    with pytest.raises(NotImplementedError, match="block kernel over the 4-bit cache is not built"):
        model.init_cache(1, 32, kv_dtype="fp4", chunked_prefill=True)
    # another head_dim
    monkeypatch.setattr(model.cfg, "num_attention_heads", 2 * cfg.num_attention_heads)
    with pytest.raises(NotImplementedError, match="head_dim 64"):
        model.init_cache(1, 32, kv_dtype="fp6")
    monkeypatch.undo()
    # a sequence ring
    from lwm_amd import llama as M
    monkeypatch.setattr(M, "sp_size_rank", lambda axis: (2, 0))
    with pytest.raises(NotImplementedError, match="sp > 1"):
        model.init_cache(1, 32, kv_dtype="fp6")
