"""Chunked prefill over the 8-bit (e4m3) KV cache on MI355X: the block kernel of csrc/attn_prefill_kv8.h through
lwm_amd.kv8.attn_prefill_kv8 -- against the fp64 oracle, torch.equal with the bf16 split-K kernel on a bf16 copy of the
cache, garbage in hidden rows, a row that sees nothing, the decode kernel at Q = 1 -- and the model wiring:
init_cache(chunked_prefill=True), generate(prefill_chunk=), the vision model's routes, peak memory, the induction needle.

Bounds are the project's own: out against the oracle 2e-2 of max, lse 2e-3; two routes of the same attention 1.6e-2 of
max (tests/test_gpu_infer.py, tests/test_gpu_kv8.py); two decode routes at the logits 2e-2 of max; graph against eager
1e-3 (tests/test_gpu_hf_anchor.py)."""
import functools
import os
import sys

import numpy as np
import pytest

from oracle import attention_ref as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

# (B, Q, idx, cache_rows, H, k_splits, left padding of batch row 0 in key_valid or None = no key_valid tensor)
CASES = [
    (1, 3, 8, 32, 2, 1, 5),            # the shape the unmarked cache refuses
    (2, 300, 70, 512, 2, 2, 9),        # two q tiles, idx off the 64 grid, ragged last key tile, batch strides, left padding
    (1, 256, 256, 1024, 8, 4, None),   # B * H a multiple of 8; no key meta at all
    (1, 64, 1000, 1100, 3, 3, 5),      # B * H no multiple of 8, idle waves
    (1, 1, 500, 512, 4, 2, 5),         # one query
    (1, 5, 60, 128, 2, 4, None),       # Sk = 65: two key tiles cut into four pieces, pieces 2 and 3 walk no tile -> (0, -inf), all written
    (1, 40, 0, 64, 1, 2, 3),           # q_start = 0, one ragged tile with the diagonal inside, second piece empty, left padding
]
IDS = ["B%d-Q%d-idx%d-rows%d-H%d-splits%d" % c[:6] for c in CASES]
SPLIT = [i for i, c in enumerate(CASES) if c[5] >= 2]


def _rand(shape, seed, mag=1.0):
    import torch
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * mag).to(torch.bfloat16)


def _np(t):
    return t.detach().float().cpu().numpy()


def _quant(x):
    """bf16 (B,S,H,128) device tensor -> (bytes u8 (B,S,H,128), scales f32 (B,S,H)) through ops.kv8_cache_write"""
    import torch
    from lwm_amd import ops
    B, S, H, D = x.shape
    q = torch.empty(B, S, H, D, dtype=torch.uint8, device=x.device)
    s = torch.empty(B, S, H, dtype=torch.float32, device=x.device)
    ops.kv8_cache_write(q, s, x.contiguous(), dst_row0=0)
    return q, s


def _prefill(q, kq, ks, vq, vs, Sk, idx, kv, n):
    """the partials over the first Sk rows of the caches: VIEWS of the whole cache, key_valid rows strided likewise"""
    from lwm_amd import kv8
    return kv8.attn_prefill_kv8(q, kq[:, :Sk], ks[:, :Sk], vq[:, :Sk], vs[:, :Sk], q_start=idx, k_splits=n,
                                key_valid=None if kv is None else kv[:, :Sk])


@functools.lru_cache(maxsize=None)
def _case(i):
    """inputs of case i and the kernel's answer, computed once and shared; nothing below writes to them"""
    import torch
    B, Q, idx, rows, H, n, pad = CASES[i]
    q = _rand((B, Q, H, 128), 100 + i).cuda()
    (kq, ks), (vq, vs) = _quant(_rand((B, rows, H, 128), 200 + i, 1.5).cuda()), _quant(_rand((B, rows, H, 128), 300 + i, 0.7).cuda())
    kv = None
    if pad is not None:
        kv = torch.ones(B, rows, dtype=torch.uint8, device="cuda")
        kv[0, :pad] = 0
    op, lp = _prefill(q, kq, ks, vq, vs, idx + Q, idx, kv, n)
    return q, kq, ks, vq, vs, kv, op, lp


def _dequant(i):
    from lwm_amd import ops
    B, Q, idx, rows, H, n, pad = CASES[i]
    q, kq, ks, vq, vs, kv, op, lp = _case(i)
    Sk = idx + Q
    return ops.kv8_dequant(kq[:, :Sk], ks[:, :Sk]), ops.kv8_dequant(vq[:, :Sk], vs[:, :Sk]), \
        (None if kv is None else kv[:, :Sk].contiguous())


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_prefill_kv8_vs_oracle(i):
    from lwm_amd import ops
    B, Q, idx, rows, H, n, pad = CASES[i]
    q, kq, ks, vq, vs, kv, op, lp = _case(i)
    out, lse = ops.attn_combine(op, lp)
    kd, vd, kvc = _dequant(i)
    # the oracle gets the DEQUANTISED cache: quantisation error is not in the comparison
    ro, rl = R.dense_attention(_np(q), _np(kd), _np(vd), causal=True, q_start=idx, key_valid=None if kvc is None else kvc.cpu().numpy())
    none = np.isneginf(rl)              # rows that see nothing: -inf exactly (-inf minus -inf is no error, it is nan)
    assert np.array_equal(np.isneginf(_np(lse)), none)
    eo, el = np.abs(_np(out) - ro).max() / np.abs(ro).max(), np.abs(_np(lse)[~none] - rl[~none]).max()
    print(f"kv8 prefill {IDS[i]}: vs oracle out {eo:.3e} of max (bound 2e-2), lse {el:.3e} (bound 2e-3)")
    assert eo <= 2e-2
    assert el <= 2e-3
    # the same launch again: the same bits
    import torch
    o2, l2 = _prefill(q, kq, ks, vq, vs, idx + Q, idx, kv, n)
    assert torch.equal(o2, op) and torch.equal(l2, lp)


@pytest.mark.parametrize("i", SPLIT, ids=[IDS[i] for i in SPLIT])
def test_prefill_kv8_partials_equal_the_bf16_kernel_bit_for_bit(i):
    """the staged tiles are exact, so the partials ARE those of the bf16 split-K kernel on a bf16 copy of the cache: pins
    the staging, the swizzle and the scale indexing on the device"""
    import torch
    from lwm_amd import ops
    B, Q, idx, rows, H, n, pad = CASES[i]
    q, kq, ks, vq, vs, kv, op, lp = _case(i)
    kd, vd, kvc = _dequant(i)
    fo, fl = ops.attn_fwd_splitk(q, kd, vd, k_splits=n, q_start=idx, causal=True, key_valid=kvc)
    assert torch.equal(op.view(torch.int32), fo.view(torch.int32))
    assert torch.equal(lp.view(torch.int32), fl.view(torch.int32))


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_prefill_kv8_hidden_rows_reach_nothing(i):
    """rows at or past idx + Q and rows with key_valid == 0 hold e4m3 NaN patterns with NaN / Inf scales, or random bytes
    with scales of 1e30: the same bits come out"""
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
    for fill_q, fill_s in ((0x7f, float("nan")), (0xff, float("inf")), (None, None)):
        k2, s2, v2, t2 = kq.clone(), ks.clone(), vq.clone(), vs.clone()
        for c, s in ((k2, s2), (v2, t2)):
            if fill_q is None:
                c[hid] = torch.randint(0, 256, c[hid].shape, generator=g, device="cuda", dtype=torch.uint8)
                s[hid] = torch.randn(s[hid].shape, generator=g, device="cuda") * 1e30
            else:
                c[hid], s[hid] = fill_q, fill_s
        o2, l2 = _prefill(q, k2, s2, v2, t2, Sk, idx, kv, n)
        assert torch.equal(o2.view(torch.int32), op.view(torch.int32)) and torch.equal(l2.view(torch.int32), lp.view(torch.int32)), \
            (fill_q, fill_s)


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_prefill_kv8_a_row_that_sees_nothing(i):
    """the last batch row with key_valid all zero: out 0 and lse -inf in every partial"""
    import torch
    from lwm_amd import ops
    B, Q, idx, rows, H, n, pad = CASES[i]
    q, kq, ks, vq, vs, kv, op, lp = _case(i)
    kv2 = torch.ones(B, rows, dtype=torch.uint8, device="cuda") if kv is None else kv.clone()
    kv2[B - 1] = 0
    o2, l2 = _prefill(q, kq, ks, vq, vs, idx + Q, idx, kv2, n)
    assert (o2[:, B - 1] == 0).all() and torch.isneginf(l2[:, B - 1]).all()
    out, lse = ops.attn_combine(o2, l2)
    assert (out[B - 1] == 0).all() and torch.isneginf(lse[B - 1]).all()
    if B > 1 and kv is not None:
        assert torch.equal(o2[:, :B - 1], op[:, :B - 1]) and torch.equal(l2[:, :B - 1], lp[:, :B - 1])


def test_prefill_kv8_one_query_against_the_decode_kernel():
    import torch
    from lwm_amd import ops
    i = [c[1] for c in CASES].index(1)
    B, Q, idx, rows, H, n, pad = CASES[i]
    q, kq, ks, vq, vs, kv, op, lp = _case(i)
    Sk = idx + Q
    out, lse = ops.attn_combine(op, lp)
    mask = torch.from_numpy(R.decode_mask(B, 1, Sk, idx, kv[:, :Sk].cpu().numpy()).astype(np.uint8)).cuda()
    do, dl = ops.attn_combine(*ops.attn_decode_kv8(q, kq[:, :Sk], ks[:, :Sk], vq[:, :Sk], vs[:, :Sk], k_splits=n, dense_mask=mask))
    eo = (out.float() - do.float()).abs().max().item() / do.float().abs().max().item()
    el = (lse - dl).abs().max().item()
    print(f"block kernel against decode kernel at Q = 1: out {eo:.3e} of max (bound 1.6e-2), lse {el:.3e} (bound 2e-3)")
    assert eo <= 1.6e-2
    assert el <= 2e-3


def test_one_piece_cast_equals_the_combine():
    """_cached_kvq rounds a single piece with the cast kernel instead of merging it: the same bits"""
    import torch
    from lwm_amd import ops
    i = [c[5] for c in CASES].index(1)
    q, kq, ks, vq, vs, kv, op, lp = _case(i)
    assert op.shape[0] == 1
    assert torch.equal(ops.cast_f32_to_bf16(op[0]).view(torch.int16), ops.attn_combine(op, lp, want_bf16=True)[0].view(torch.int16))
    # ... also where a row sees nothing (out 0, lse -inf)
    B, Q, idx, rows, H, n, pad = CASES[i]
    o0, l0 = _prefill(q, kq, ks, vq, vs, idx + Q, idx, torch.zeros(B, rows, dtype=torch.uint8, device="cuda"), 1)
    assert torch.equal(ops.cast_f32_to_bf16(o0[0]).view(torch.int16), ops.attn_combine(o0, l0, want_bf16=True)[0].view(torch.int16))


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


PL, NEW, PAD = 40, 6, 5


def _batch(total):
    """B = 2, `total` random tokens per row, row 0 left-padded by PAD -> (tokens, mask over the tokens)"""
    import torch
    g = torch.Generator().manual_seed(11)
    seq = torch.randint(0, 384, (2, total), generator=g).cuda()
    mask = torch.ones(2, total, dtype=torch.int32, device="cuda")
    mask[0, :PAD] = 0
    return seq, mask


def test_blocks_into_a_live_fp8_cache_equal_one_token_at_a_time():
    """An 8-bit cache that takes blocks (chunked_prefill=True), fed 16 + 16 + 8 prompt tokens and 6 teacher-forced decode
    steps, against the same kind of cache fed the first 16 tokens as one block and every later prompt token one at a
    time through the decode path: a block is quantised, then attends over the quantised rows -- the decode step's rule --
    so the two differ by the attention route only.  Without the feature the second block raises NotImplementedError."""
    import torch
    cfg, model = _model()
    L = PL + 16
    seq, mask = _batch(PL + NEW)
    ext = torch.ones(2, L, dtype=torch.int32, device="cuda")
    ext[:, :PL] = mask[:, :PL]
    pos = (mask.cumsum(-1) - 1).clamp_min(0).to(torch.int32).contiguous()

    def run(cuts):
        cache = model.init_cache(2, L, kv_dtype="fp8", chunked_prefill=True)
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
    print(f"fp8 cache, prompt in blocks 16 + 16 + 8 against one token at a time: logit difference of max, last prompt "
          f"position then {NEW} decode steps, both rows: {[f'{x:.2e}' for x in d.tolist()]} (bound 2e-2)")
    assert d.max().item() <= 2e-2


def test_generate_fp8_chunked_graph_equals_eager():
    import torch
    cfg, model = _model()
    seq, mask = _batch(PL)
    kw = dict(attention_mask=mask, max_new_tokens=16, return_logits=True, kv_dtype="fp8", prefill_chunk=16)
    eager, le = model.generate(seq, **kw)
    graph, lg = model.generate(seq, graph=True, **kw)
    d = (lg - le).abs().max().item() / le.abs().max().item()
    print(f"fp8 cache, prefill_chunk=16, graph against eager: logits differ by {d:.3e} of max (bound 1e-3)")
    assert eager.shape == (2, PL + 16)
    assert torch.equal(graph, eager)
    assert d <= 1e-3


def test_generate_default_cache_chunked_against_one_shot():
    import torch
    cfg, model = _model()
    seq, mask = _batch(PL)
    kw = dict(attention_mask=mask, max_new_tokens=16, return_logits=True)
    one, l1 = model.generate(seq, **kw)
    chk, lc = model.generate(seq, prefill_chunk=16, **kw)
    d = ((lc - l1).abs().amax(-1) / l1.abs().max()).flatten()
    agree = (one == chk).float().mean().item()
    print(f"default cache, prefill_chunk=16 against one shot: per-step logit difference of max "
          f"{[f'{x:.2e}' for x in d.tolist()]} (bound 2e-2); token agreement {agree:.3f}")
    assert d.max().item() <= 2e-2
    # a chunk as long as the prompt, or longer, is the one-shot prefill
    same, ls = model.generate(seq, prefill_chunk=PL + 3, **kw)
    assert torch.equal(same, one) and torch.equal(ls, l1)


def test_seeded_sampling_with_chunked_fp8_prefill_is_reproducible():
    import torch
    from lwm_amd.vision_llama import VideoLLaMAConfig, VideoLLaMAForCausalLM
    torch.manual_seed(0)
    cfg = VideoLLaMAConfig(vocab_size=384, hidden_size=256, intermediate_size=512, num_hidden_layers=2,
                           num_attention_heads=2, max_sequence_length=512, vision_vocab_size=64, sample_mode="text")
    model = VideoLLaMAForCausalLM(cfg).cuda()
    ids = torch.randint(0, 384, (2, 27), device="cuda")
    kw = dict(max_new_tokens=12, do_sample=True, temperature=0.9, top_k=50, seed=1234, kv_dtype="fp8", prefill_chunk=8)
    a = model.generate(ids, **kw)
    b = model.generate(ids, **kw)
    assert torch.equal(a, b) and a.shape == (2, 12)
    g = model.generate(ids, graph=True, **kw)
    g2 = model.generate(ids, graph=True, **kw)
    assert torch.equal(g, g2)


def test_chunked_prefill_lowers_the_peak_memory():
    """a 4096-token prompt on the fixture: the prefill in blocks of 512 peaks strictly below the one-shot prefill, same
    cache kind (a condition, not a measurement: both values are printed)"""
    import torch
    cfg, model = _model(max_positions=8192)
    S = 4096
    ids = torch.randint(0, 384, (1, S), generator=torch.Generator().manual_seed(5)).cuda()
    pos = torch.arange(S, dtype=torch.int32, device="cuda")[None]
    peaks = {}
    for kind in ("fp8", None):
        for chunk in (S, 512):
            cache = model.init_cache(1, S + 8, **({} if kind is None else dict(kv_dtype=kind, chunked_prefill=True)))
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            with torch.no_grad():
                for a in range(0, S, chunk):
                    h = model.hidden_states(ids[:, a:a + chunk], None, None, pos[:, a:a + chunk].contiguous(), cache)
            torch.cuda.synchronize()
            peaks[(kind or "default", chunk)] = (torch.cuda.max_memory_allocated() - base, torch.cuda.max_memory_allocated())
            assert all(c["cache_index"] == S for c in cache)
            del cache, h
    print("prefill of 4096 tokens, peak bytes above the cache (and in all): " +
          "; ".join(f"{k} cache, block {c}: {v[0]} ({v[1]})" for (k, c), v in peaks.items()))
    assert peaks[("fp8", 512)][1] < peaks[("fp8", S)][1]
    assert peaks[("default", 512)][1] < peaks[("default", S)][1]


def test_needle_through_a_chunked_fp8_prefill():
    """tests/_induction.py at theta 1e7, 32768 tokens, needle at depth 0.5: rows [0, S - 1) go into the cache in blocks of
    4096 (the last is 4095), the final token is a decode step.  With the 8-bit cache every block after the first sees
    quantised keys; the argmax must stay on the planted value.  The margin is printed beside the default cache's."""
    import torch
    from lwm_amd.llama import LLaMAConfig, LLaMAForCausalLM
    from lwm_amd.weights import load_params
    from tests import _induction as I
    theta, S, depth, chunk = 1e7, 32768, 0.5, 4096
    cfg_kw, st = I.build(theta, S)
    cfg = LLaMAConfig(**cfg_kw, scan_mlp_chunk_size=65536)
    with torch.device("cuda"):
        model = load_params(LLaMAForCausalLM(cfg), st)
    toks, where = I.haystack(S, depth)
    toks = toks.cuda()
    ar = torch.arange(S, dtype=torch.int32, device="cuda")[None]
    margins = {}
    for kind in ("fp8", None):
        cache = model.init_cache(1, S, **({} if kind is None else dict(kv_dtype=kind, chunked_prefill=True)))
        with torch.no_grad():
            for a in range(0, S - 1, chunk):
                z = min(a + chunk, S - 1)
                model.hidden_states(toks[:, a:z], None, None, ar[:, a:z].contiguous(), cache)
            assert all(c["cache_index"] == S - 1 for c in cache)
            h = model.hidden_states(toks[:, S - 1:], None, None, ar[:, S - 1:].contiguous(), cache)
            logits = (h[0, -1].float() @ model.lm_head.float()).cpu()
        top = logits.topk(2)
        margins[kind or "default"] = (top.indices[0].item(), (top.values[0] - top.values[1]).item())
        del cache, h
    print(f"NEEDLE S={S} depth={depth} (needle at {where}), prefill in blocks of {chunk}: argmax / margin over the runner-up: {margins}")
    assert margins["default"][0] == I.VALUE_TOKEN
    assert margins["fp8"][0] == I.VALUE_TOKEN, margins


def test_refused_cases_are_named():
    import torch
    cfg, model = _model()
    ids = torch.randint(0, 384, (1, 8), device="cuda")
    for bad in (0, -3):
        with pytest.raises(ValueError, match="prefill_chunk"):
            model.generate(ids, max_new_tokens=2, prefill_chunk=bad)
    # a sequence ring
    from lwm_amd import llama as M
    orig = M.sp_size_rank
    try:
        M.sp_size_rank = lambda axis: (2, 0)
        with pytest.raises(NotImplementedError, match="one rank"):
            model.generate(ids, max_new_tokens=2, prefill_chunk=4)
    finally:
        M.sp_size_rank = orig
    # a block through the device-index (graph) form of a cache that takes blocks: not captured, the message it had
    cache = model.init_cache(1, 32, kv_dtype="fp8", chunked_prefill=True)
    pos = torch.arange(8, dtype=torch.int32, device="cuda")[None]
    with torch.no_grad():
        model.hidden_states(ids, None, None, pos, cache)
        dcache = model.device_index_cache(cache, torch.tensor([8], dtype=torch.int32, device="cuda"))
        with pytest.raises(NotImplementedError, match="Q > 1 at cache_index > 0"):
            model.hidden_states(ids[:, :3], None, None, pos[:, :3] + 8, dcache)
    # the flag does not widen what kv_dtype takes
    with pytest.raises(ValueError, match="kv_dtype"):
        model.init_cache(1, 32, kv_dtype="int4", chunked_prefill=True)
    # ... and the default cache ignores it
    assert "kv8_blocks" not in model.init_cache(1, 32, chunked_prefill=True)[0]
