"""The 8-bit (e4m3) KV cache on MI355X: the quantising write bit for bit against the numpy restatement of the format
(tests/_kv8_ref.py), the decode kernel of csrc/attn_decode_kv8.h against the fp64 oracle and against the bf16 decode
kernel on the same numbers, its mask behaviour, the device-index write, and the model-level wiring of
generate(kv_dtype="fp8") on the tiny HF fixture.  What quantisation itself costs is measured and printed, not gated
(profiles/r08_kv8_decode.md records it); only the needle's argmax is asserted.

Bounds: decode against the oracle 2e-2 of max / lse 2e-3 (bf16 q, f32 accumulation: tests/test_gpu_infer.py); two
forms of the same attention 1.6e-2 of max (ibid.); graph against eager logits 1e-3 of max and two decode routes 2e-2 of
max (tests/test_gpu_hf_anchor.py)."""
import os
import sys

import numpy as np
import pytest

from oracle import attention_ref as R
from tests import _kv8_ref as K8

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
    """bf16 (B,S,H,128) device tensor -> (bytes u8 (B,S,H,128), scales f32 (B,S,H)) through ops.kv8_cache_write"""
    import torch
    from lwm_amd import ops
    B, S, H, D = x.shape
    q = torch.empty(B, S, H, D, dtype=torch.uint8, device=x.device)
    s = torch.empty(B, S, H, dtype=torch.float32, device=x.device)
    ops.kv8_cache_write(q, s, x.contiguous(), dst_row0=0)
    return q, s


def _decode(q, kq, ks, vq, vs, mask, splits):
    from lwm_amd import ops
    return ops.attn_combine(*ops.attn_decode_kv8(q, kq, ks, vq, vs, k_splits=splits, dense_mask=mask))


# ---------------------------------------------------------------- quantiser
def test_quantiser_bit_for_bit():
    """random rows over magnitudes 1e-6 .. 1e3 and the edge rows of tests/_kv8_ref.edge_rows: bytes and scales equal the
    restatement.  A disagreement of the hardware conversion with OCP e4m3fn would show here."""
    import torch
    rng = np.random.default_rng(0)
    mags = 10.0 ** rng.uniform(-6, 3, size=(4096, 1))
    x = np.concatenate([R.round_bf16((rng.standard_normal((4096, 128)) * mags).astype(np.float32)), K8.edge_rows(rng)])
    x = np.concatenate([x, np.zeros((-x.shape[0] % 32, 128), np.float32)])
    for H in (32, 1):
        src = x.reshape(1, -1, H, 128)
        q, s = _quant(torch.from_numpy(src).to(torch.bfloat16).cuda())
        rq, rs = K8.quantise(src)
        bad = np.argwhere(q.cpu().numpy() != rq)
        assert np.array_equal(s.cpu().numpy(), rs), np.argwhere(s.cpu().numpy() != rs)[:8]
        assert bad.size == 0, [(tuple(i), src[tuple(i)], q.cpu().numpy()[tuple(i)], rq[tuple(i)]) for i in bad[:8]]
    # the yardstick on the device: dequantised bytes are the restatement's numbers exactly
    from lwm_amd import ops
    assert np.array_equal(_np(ops.kv8_dequant(q, s)), K8.dequant(rq, rs))


def test_write_at_equals_host_index_and_skips_outside_rows():
    import torch
    from lwm_amd import ops
    B, S, H, n = 2, 12, 4, 4
    src = _rand((B, 6, H, 128), 5, 3.0).cuda()
    q, s = _quant(src)
    fresh = lambda: (torch.full((B, S, H, 128), 0xAB, dtype=torch.uint8, device="cuda"),
                     torch.full((B, S, H), 7.5, dtype=torch.float32, device="cuda"))
    dev = lambda i: torch.tensor([i], dtype=torch.int32, device="cuda")
    ch, sh = fresh()
    ops.kv8_cache_write(ch, sh, src, dst_row0=5, src_row0=1, nrows=n)
    cd, sd = fresh()
    ops.kv8_cache_write_at(cd, sd, src, dev(3), row_offset=2, src_row0=1, nrows=n)
    assert torch.equal(ch, cd) and torch.equal(sh, sd)
    assert torch.equal(ch[:, 5:9], q[:, 1:5]) and torch.equal(sh[:, 5:9], s[:, 1:5])
    assert (ch[:, :5] == 0xAB).all() and (ch[:, 9:] == 0xAB).all() and (sh[:, :5] == 7.5).all() and (sh[:, 9:] == 7.5).all()
    cd, sd = fresh()
    ops.kv8_cache_write_at(cd, sd, src, dev(10), nrows=n)                    # rows 10, 11 land; 12, 13 are outside
    assert torch.equal(cd[:, 10:12], q[:, 0:2]) and torch.equal(sd[:, 10:12], s[:, 0:2])
    assert (cd[:, :10] == 0xAB).all() and (sd[:, :10] == 7.5).all()
    cd, sd = fresh()
    ops.kv8_cache_write_at(cd, sd, src, dev(3), row_offset=-S, nrows=n)      # another shard's rows: nothing is written
    assert (cd == 0xAB).all() and (sd == 7.5).all()
    ops.kv8_cache_write_at(cd, sd, src, dev(3), row_offset=-5, nrows=n)      # rows -2, -1, 0, 1
    assert torch.equal(cd[:, 0:2], q[:, 2:4]) and (cd[:, 2:] == 0xAB).all() and (sd[:, 2:] == 7.5).all()


# ---------------------------------------------------------------- decode kernel
@pytest.mark.parametrize("B,K,H,splits,cache_index", [
    (2, 4096, 4, 8, 4000),
    (1, 1000, 2, 3, 999),
    (1, 2048, 2, 4, 1500),
    (1, 8192, 32, 16, 100),      # mostly-empty cache: whole pieces masked
    (1, 1024, 2, 1, 700),
])
def test_decode_vs_oracle_and_vs_the_bf16_kernel(B, K, H, splits, cache_index):
    """the shapes of tests/test_gpu_infer.py::test_decode_vs_oracle at Q = 1.  The oracle and the bf16 kernel get the
    DEQUANTISED cache, so quantisation error is in neither comparison."""
    import torch
    from lwm_amd import ops
    q, k, v = _rand((B, 1, H, 128), 1).cuda(), _rand((B, K, H, 128), 2).cuda(), _rand((B, K, H, 128), 3).cuda()
    am = (np.random.default_rng(4).random((B, K)) > 0.1).astype(np.uint8)
    am[:, 0] = 1
    mask = R.decode_mask(B, 1, K, cache_index, am)
    md = torch.from_numpy(mask.astype(np.uint8)).cuda()
    (kq, ks), (vq, vs) = _quant(k), _quant(v)
    out, lse = _decode(q, kq, ks, vq, vs, md, splits)
    kd, vd = ops.kv8_dequant(kq, ks), ops.kv8_dequant(vq, vs)
    ro, rl = R.dense_attention(_np(q), _np(kd), _np(vd), causal=False, dense_mask=mask)
    e_out, e_lse = np.abs(_np(out) - ro).max() / np.abs(ro).max(), np.abs(_np(lse) - rl).max()
    ob, lb = ops.attn_combine(*ops.attn_fwd_splitk(q, kd, vd, k_splits=splits, dense_mask=md))
    e_bf = (out.float() - ob.float()).abs().max().item() / np.abs(ro).max()
    print(f"kv8 decode B={B} K={K} H={H} splits={splits}: vs oracle out {e_out:.3e} lse {e_lse:.3e}; vs bf16 kernel {e_bf:.3e} "
          f"lse {(lse - lb).abs().max().item():.3e}")
    assert e_out <= 2e-2
    assert e_lse <= 2e-3
    assert e_bf <= 1.6e-2
    assert (lse - lb).abs().max().item() <= 2e-3


def test_decode_full_size_cache_properties():
    """LWM-7B decode shapes, 32 heads over a 131072-row cache with 100000 rows visible: one head against the oracle,
    the bf16 kernel on the dequantised cache, V = ones, garbage (NaN patterns included) in masked rows, a row that
    sees nothing."""
    import torch
    from lwm_amd import ops
    from lwm_amd.ring import _pick_splits
    B, K, H = 1, 131072, 32
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=g, device="cuda", dtype=torch.float32).to(torch.bfloat16)
    k, v, q = rnd(B, K, H, 128), rnd(B, K, H, 128), rnd(B, 1, H, 128)
    (kq, ks), (vq, vs) = _quant(k), _quant(v)
    del k, v
    mask = torch.zeros(B, 1, K, dtype=torch.uint8, device="cuda")
    mask[:, :, :100000] = 1
    ns = _pick_splits(B, 1, H, K)
    out, lse = _decode(q, kq, ks, vq, vs, mask, ns)
    # one head against the oracle, every head against the bf16 kernel on the same numbers
    h = 11
    kd, vd = ops.kv8_dequant(kq, ks), ops.kv8_dequant(vq, vs)
    ro, rl = R.dense_attention(_np(q[:, :, h:h + 1]), _np(kd[:, :, h:h + 1]), _np(vd[:, :, h:h + 1]), causal=False,
                               dense_mask=mask.cpu().numpy())
    e_out = np.abs(_np(out[:, :, h:h + 1]) - ro).max() / np.abs(ro).max()
    e_lse = np.abs(_np(lse[:, h:h + 1]) - rl).max()
    ob, lb = ops.attn_combine(*ops.attn_fwd_splitk(q, kd, vd, k_splits=ns, dense_mask=mask))
    e_bf = (out.float() - ob.float()).abs().max().item() / ob.float().abs().max().item()
    print(f"kv8 decode H=32 Sk=131072 (100000 visible, {ns} pieces): vs oracle out {e_out:.3e} lse {e_lse:.3e}; "
          f"vs bf16 kernel {e_bf:.3e} lse {(lse - lb).abs().max().item():.3e}")
    assert e_out <= 2e-2 and e_lse <= 2e-3
    assert e_bf <= 1.6e-2 and (lse - lb).abs().max().item() <= 2e-3
    del kd, vd, ob, lb
    # V = ones: 1.0 is an e4m3 value, the output is a weighted mean of ones
    oq, os_ = _quant(torch.ones(B, K, H, 128, dtype=torch.bfloat16, device="cuda"))
    o1, _ = _decode(q, kq, ks, oq, os_, mask, ns)
    assert (o1.float() - 1).abs().max().item() <= 8e-3
    del oq, os_
    # garbage bytes and garbage scales in masked rows, NaN bit patterns among them, change nothing
    for fill_q, fill_s in ((0x7f, float("nan")), (0xff, float("inf")), (None, -3e38)):
        k2, s2, v2, t2 = kq.clone(), ks.clone(), vq.clone(), vs.clone()
        for c, s in ((k2, s2), (v2, t2)):
            if fill_q is None:
                c[:, 100000:] = torch.randint(0, 256, c[:, 100000:].shape, generator=g, device="cuda", dtype=torch.uint8)
            else:
                c[:, 100000:] = fill_q
            s[:, 100000:] = fill_s
        o2, l2 = _decode(q, k2, s2, v2, t2, mask, ns)
        assert torch.equal(o2, out) and torch.equal(l2, lse), (fill_q, fill_s)
    del k2, s2, v2, t2
    # a hole inside the visible range is handled per key, whatever it holds
    hole = mask.clone()
    hole[:, :, 5000:5100] = 0
    oh, lh = _decode(q, kq, ks, vq, vs, hole, ns)
    k2, s2 = kq.clone(), ks.clone()
    k2[:, 5000:5100], s2[:, 5000:5100] = 0x7f, float("nan")
    oh2, lh2 = _decode(q, k2, s2, vq, vs, hole, ns)
    assert torch.equal(oh, oh2) and torch.equal(lh, lh2) and not torch.equal(oh, out)
    # nothing visible: out 0, lse -inf
    o0, l0 = _decode(q, kq, ks, vq, vs, torch.zeros_like(mask), ns)
    assert (o0 == 0).all() and torch.isneginf(l0).all()


# ---------------------------------------------------------------- model level (the tiny HF fixture)
def _model():
    import hf_fixture as F
    from lwm_amd import weights as W
    from lwm_amd.llama import LLaMAForCausalLM
    cfg = W.config_from_hf(F.HF_CONFIG)
    model = LLaMAForCausalLM(cfg).cuda()
    W.load_params(model, W.hf_to_lwm(F.state_dict(), cfg.num_attention_heads))
    return cfg, model


def _prompt():
    import torch
    gold = np.load(os.path.join(HERE, "golden", "hf_llama_tiny.npz"))
    seq = torch.from_numpy(gold["gen_tokens"]).cuda()
    mask = torch.from_numpy(gold["gen_mask"]).cuda()
    return seq, mask, mask.shape[1], gold["gen_scores"].shape[1]


def test_init_cache_fp8_layout():
    import torch
    cfg, model = _model()
    cache = model.init_cache(2, 64, kv_dtype="fp8")
    assert len(cache) == cfg.num_hidden_layers
    H = cfg.num_attention_heads
    for c in cache:
        assert c["cached_key"].dtype == torch.uint8 and tuple(c["cached_key"].shape) == (2, 64, H, 128)
        assert c["cached_value"].dtype == torch.uint8 and tuple(c["cached_value"].shape) == (2, 64, H, 128)
        assert c["key_scale"].dtype == torch.float32 and tuple(c["key_scale"].shape) == (2, 64, H)
        assert c["value_scale"].dtype == torch.float32 and tuple(c["value_scale"].shape) == (2, 64, H)
        assert c["cache_index"] == 0
    assert "key_scale" not in model.init_cache(2, 64)[0]                    # the default cache is what it was


def test_generate_fp8_graph_equals_eager():
    import torch
    cfg, model = _model()
    seq, mask, PL, NEW = _prompt()
    eager, le = model.generate(seq[:, :PL], attention_mask=mask, max_new_tokens=NEW, return_logits=True, kv_dtype="fp8")
    graph, lg = model.generate(seq[:, :PL], attention_mask=mask, max_new_tokens=NEW, return_logits=True, kv_dtype="fp8",
                               graph=True)
    d = (lg - le).abs().max().item() / le.abs().max().item()
    print(f"fp8 cache, graph against eager: logits differ by {d:.3e} of max")
    assert torch.equal(graph, eager)
    assert d <= 1e-3


def test_fp8_cache_steps_equal_a_bf16_cache_of_the_dequantised_rows(monkeypatch):
    """hidden_states stepped by hand: an 8-bit cache against a bf16 cache whose newly written rows are replaced by
    kv8_dequant(quantise(row)) after every call -- the same numbers in both caches, so the per-step logits differ by
    the two decode routes only (and by the one row a bf16 step sees before it is replaced: its own).  Pins the wiring,
    the unquantised prefill included.  Then the cost of quantisation itself, measured: fp8 against the plain bf16 cache."""
    import torch
    from lwm_amd import ops
    cfg, model = _model()
    seq, mask, PL, NEW = _prompt()
    L = PL + NEW
    ext = torch.ones(1, L, dtype=torch.int32, device="cuda")
    ext[:, :PL] = mask

    def run(kind, fused):
        monkeypatch.setenv("LWM_DECODE_FUSED", "1" if fused else "0")
        cache = model.init_cache(1, L, kv_dtype="fp8" if kind == "fp8" else None)
        pos = (mask.cumsum(-1) - 1).clamp_min(0).to(torch.int32).contiguous()
        step_in, done, logits = seq[:, :PL], 0, []
        with torch.no_grad():
            for t in range(NEW):
                h = model.hidden_states(step_in, ext, None, pos, cache)
                logits.append((h[:, -1].float() @ model.lm_head.float()).cpu())
                new = int(cache[0]["cache_index"])
                if kind == "bf16-of-dequantised":
                    for c in cache:
                        for n in ("cached_key", "cached_value"):
                            rows = c[n][:, done:new].contiguous()
                            c[n][:, done:new] = ops.kv8_dequant(*_quant(rows))
                done = new
                step_in, pos = seq[:, PL + t:PL + t + 1], (pos[:, -1:] + 1).contiguous()
        assert all(c["cache_index"] == L - 1 for c in cache)
        return torch.stack(logits, 1)

    for fused in (True, False):
        l8, ld = run("fp8", fused), run("bf16-of-dequantised", fused)
        d = ((l8 - ld).abs().amax(-1) / ld.abs().max()).flatten()
        print(f"fp8 cache against a bf16 cache of the dequantised rows (fused={fused}): per-step logit difference of max "
              f"{[f'{x:.2e}' for x in d.tolist()]}")
        assert d.max().item() <= 2e-2
    lb = run("bf16", True)
    d = ((l8 - lb).abs().amax(-1) / lb.abs().max()).flatten()
    agree = (l8.argmax(-1) == lb.argmax(-1)).float().mean().item()
    print(f"COST fp8 cache against the bf16 cache (teacher forced, {NEW} steps): per-step logit difference of max "
          f"{[f'{x:.2e}' for x in d.tolist()]}; argmax agreement {agree:.3f}")


def test_seeded_sampling_with_fp8_cache_is_reproducible():
    import torch
    from lwm_amd.vision_llama import VideoLLaMAConfig, VideoLLaMAForCausalLM
    torch.manual_seed(0)
    cfg = VideoLLaMAConfig(vocab_size=384, hidden_size=256, intermediate_size=512, num_hidden_layers=2,
                           num_attention_heads=2, max_sequence_length=512, vision_vocab_size=64, sample_mode="text")
    model = VideoLLaMAForCausalLM(cfg).cuda()
    ids = torch.randint(0, 384, (2, 24), device="cuda")
    kw = dict(max_new_tokens=12, do_sample=True, temperature=0.9, top_k=50, seed=1234, kv_dtype="fp8")
    a = model.generate(ids, **kw)
    b = model.generate(ids, **kw)
    g = model.generate(ids, graph=True, **kw)
    g2 = model.generate(ids, graph=True, **kw)
    assert torch.equal(a, b) and torch.equal(g, g2)
    assert a.shape == (2, 12) and g.shape == (2, 12)
    c = model.generate(ids, **{**kw, "seed": 99})
    assert not torch.equal(a, c)


def test_refused_cases_are_named():
    import torch
    from lwm_amd.llama import LLaMAForCausalLM
    from lwm_amd import weights as W
    import hf_fixture as F
    cfg, model = _model()
    with pytest.raises(ValueError, match="kv_dtype"):
        model.init_cache(1, 32, kv_dtype="int4")
    f32 = LLaMAForCausalLM(W.config_from_hf(F.HF_CONFIG), dtype=torch.float32).cuda()
    with pytest.raises(NotImplementedError, match="float32"):
        f32.init_cache(1, 32, kv_dtype="fp8")
    with pytest.raises(NotImplementedError, match="float32"):
        f32.generate(torch.zeros(1, 4, dtype=torch.int64, device="cuda"), max_new_tokens=2, kv_dtype="fp8")
    # a block of tokens after the prompt
    cache = model.init_cache(1, 32, kv_dtype="fp8")
    ids = torch.randint(0, 384, (1, 8), device="cuda")
    pos = torch.arange(8, dtype=torch.int32, device="cuda")[None]
    with torch.no_grad():
        model.hidden_states(ids, None, None, pos, cache)
        with pytest.raises(NotImplementedError, match="Q > 1 at cache_index > 0"):
            model.hidden_states(ids[:, :3], None, None, pos[:, :3] + 8, cache)
    # a sequence ring
    from lwm_amd import llama as M
    orig = M.sp_size_rank
    try:
        M.sp_size_rank = lambda axis: (2, 0)
        with pytest.raises(NotImplementedError, match="sp > 1"):
            model.init_cache(1, 32, kv_dtype="fp8")
    finally:
        M.sp_size_rank = orig
    # the decode wrapper: a query that is not (B,1,H,D), more pieces than the entry takes
    from lwm_amd import ops
    q = torch.zeros(1, 1, 2, 128, dtype=torch.bfloat16, device="cuda")
    kq, sc = torch.zeros(1, 8, 2, 128, dtype=torch.uint8, device="cuda"), torch.ones(1, 8, 2, device="cuda")
    with pytest.raises(ValueError, match=r"attn_decode_kv8: q: expected a bf16 \(B,1,H,D\)"):
        ops.attn_decode_kv8(q[0], kq, sc, kq, sc, k_splits=1)
    with pytest.raises(ValueError, match="attn_decode_kv8: k_splits = 4097 > 4096"):
        ops.attn_decode_kv8(q, kq, sc, kq, sc, k_splits=4097)


# ---------------------------------------------------------------- what quantisation costs: the induction needle
def test_needle_through_the_fp8_cache_at_one_million_tokens():
    """tests/_induction.py at its longest context (2^20 tokens, theta 5e7; tests/test_gpu_induction_needle.py): the
    prompt up to the final token is prefilled into the cache, the final token -- the second occurrence of the key --
    is a decode step over it.  The argmax must stay on the planted value with the 8-bit cache; the margin is printed
    beside the bf16 cache's."""
    import torch
    from lwm_amd.llama import LLaMAConfig, LLaMAForCausalLM
    from lwm_amd.weights import load_params
    from tests import _induction as I
    theta, S, depth = 5e7, 1 << 20, 0.35
    cfg_kw, st = I.build(theta, S)
    assert (S - 1) % 25 == 0
    cfg = LLaMAConfig(**cfg_kw, scan_mlp_chunk_size=(S - 1) // 25)          # (the prefill is S - 1 rows)
    with torch.device("cuda"):
        model = load_params(LLaMAForCausalLM(cfg), st)
    toks, pos = I.haystack(S, depth)
    toks = toks.cuda()
    ar = torch.arange(S, dtype=torch.int32, device="cuda")[None]
    margins = {}
    for kv in ("fp8", None):
        cache = model.init_cache(1, S, kv_dtype=kv)
        with torch.no_grad():
            model.hidden_states(toks[:, :S - 1], None, None, ar[:, :S - 1].contiguous(), cache)
            h = model.hidden_states(toks[:, S - 1:], None, None, ar[:, S - 1:].contiguous(), cache)
            logits = (h[0, -1].float() @ model.lm_head.float()).cpu()
        top = logits.topk(2)
        margins[kv or "bf16"] = (top.indices[0].item(), (top.values[0] - top.values[1]).item())
        del cache, h
    print(f"NEEDLE S={S} depth={depth} (needle at {pos}): argmax / margin over the runner-up: {margins}")
    assert margins["bf16"][0] == I.VALUE_TOKEN
    assert margins["fp8"][0] == I.VALUE_TOKEN, margins
