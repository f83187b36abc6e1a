"""The 4-bit (MXFP4) KV cache on MI355X: the quantising write bit for bit against the numpy restatement of the format
(tests/_kv4_ref.py), the decode kernel of csrc/attn_decode_kv4.h against the fp64 oracle and against the bf16 decode
kernel on the same numbers, its mask behaviour, the device-index write, and the model-level wiring of
generate(kv_dtype="fp4") on the tiny HF fixture.  What quantisation itself costs is measured and printed, not gated
(profiles/r14_kv4_decode.md records it).

Bounds: decode against the oracle 2e-2 of max / lse 2e-3 (bf16 q, f32 accumulation: tests/test_gpu_infer.py); two
forms of the same attention 1.6e-2 of max (ibid.); graph against eager logits 1e-3 of max and two decode routes 2e-2 of
max (tests/test_gpu_hf_anchor.py).  They are the bounds of tests/test_gpu_kv8.py: the oracle and the bf16 kernel get the
DEQUANTISED cache, so the arithmetic class is the same and quantisation error is in no comparison."""
import os
import sys

import numpy as np
import pytest

from oracle import attention_ref as R
from tests import _kv4_ref as K4

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
    """bf16 (B,S,H,128) device tensor -> (nibble bytes u8 (B,S,H,64), e8m0 bytes u8 (B,S,H,4)) through kv4_cache_write"""
    import torch
    from lwm_amd import kv4
    B, S, H, D = x.shape
    q = torch.full((B, S, H, D // 2), 0xAB, dtype=torch.uint8, device=x.device)
    s = torch.full((B, S, H, 4), 0xAB, dtype=torch.uint8, device=x.device)
    kv4.kv4_cache_write(q, s, x.contiguous(), dst_row0=0)
    return q, s


def _decode(q, kq, ks, vq, vs, mask, splits):
    from lwm_amd import kv4, ops
    return ops.attn_combine(*kv4.attn_decode_kv4(q, kq, ks, vq, vs, k_splits=splits, dense_mask=mask))


# ---------------------------------------------------------------- quantiser
def test_quantiser_bit_for_bit():
    """4096 random rows over magnitudes 1e-6 .. 1e3 and the edge rows of tests/_kv4_ref.edge_rows: nibbles and scale bytes
    equal the restatement, at H = 32 and H = 1"""
    import torch
    from lwm_amd import kv4
    rng = np.random.default_rng(0)
    mags = 10.0 ** rng.uniform(-6, 3, size=(4096, 1))
    x = np.concatenate([R.round_bf16((rng.standard_normal((4096, 128)) * mags).astype(np.float32)), K4.edge_rows(rng)])
    x = np.concatenate([x, np.zeros((-x.shape[0] % 32, 128), np.float32)])
    for H in (32, 1):
        src = x.reshape(1, -1, H, 128)
        q, s = _quant(torch.from_numpy(src).to(torch.bfloat16).cuda())
        rq, rs = K4.quantise(src)
        assert np.array_equal(s.cpu().numpy(), rs), np.argwhere(s.cpu().numpy() != rs)[:8]
        bad = np.argwhere(q.cpu().numpy() != rq)
        assert bad.size == 0, [(tuple(i), q.cpu().numpy()[tuple(i)], rq[tuple(i)]) for i in bad[:8]]
    # the yardstick on the device: dequantised bytes are the restatement's numbers exactly (wherever they are normal
    # numbers below the top of bf16: every row but the all-2^-130 and the all-3e38 one)
    ok = (rs >= 2).all(-1) & (np.abs(src).max(-1) < 1e38)
    assert ok.sum() >= ok.size - 2
    d = _np(kv4.kv4_dequant(q, s)).astype(np.float64)
    assert np.array_equal(d[ok], K4.dequant(rq, rs)[ok])


def test_write_at_equals_host_index_and_skips_outside_rows():
    import torch
    from lwm_amd import kv4
    B, S, H, n = 2, 12, 4, 4
    src = _rand((B, 6, H, 128), 5, 3.0).cuda()
    q, s = _quant(src)
    fresh = lambda: (torch.full((B, S, H, 64), 0xAB, dtype=torch.uint8, device="cuda"),
                     torch.full((B, S, H, 4), 0xAB, dtype=torch.uint8, device="cuda"))
    dev = lambda i: torch.tensor([i], dtype=torch.int32, device="cuda")
    ch, sh = fresh()
    kv4.kv4_cache_write(ch, sh, src, dst_row0=5, src_row0=1, nrows=n)
    cd, sd = fresh()
    kv4.kv4_cache_write_at(cd, sd, src, dev(3), row_offset=2, src_row0=1, nrows=n)
    assert torch.equal(ch, cd) and torch.equal(sh, sd)
    assert torch.equal(ch[:, 5:9], q[:, 1:5]) and torch.equal(sh[:, 5:9], s[:, 1:5])
    assert (ch[:, :5] == 0xAB).all() and (ch[:, 9:] == 0xAB).all() and (sh[:, :5] == 0xAB).all() and (sh[:, 9:] == 0xAB).all()
    cd, sd = fresh()
    kv4.kv4_cache_write_at(cd, sd, src, dev(10), nrows=n)                    # rows 10, 11 land; 12, 13 are outside
    assert torch.equal(cd[:, 10:12], q[:, 0:2]) and torch.equal(sd[:, 10:12], s[:, 0:2])
    assert (cd[:, :10] == 0xAB).all() and (sd[:, :10] == 0xAB).all()
    cd, sd = fresh()
    kv4.kv4_cache_write_at(cd, sd, src, dev(3), row_offset=-S, nrows=n)      # another shard's rows: nothing is written
    assert (cd == 0xAB).all() and (sd == 0xAB).all()
    kv4.kv4_cache_write_at(cd, sd, src, dev(3), row_offset=-5, nrows=n)      # rows -2, -1, 0, 1
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
    from lwm_amd import kv4, ops
    q, k, v = _rand((B, 1, H, 128), 1).cuda(), _rand((B, K, H, 128), 2).cuda(), _rand((B, K, H, 128), 3).cuda()
    k[..., 32:64] *= 0.25                # blocks of different magnitude inside a head: a wrong scale byte shows
    v[..., 96:] *= 8.0
    am = (np.random.default_rng(4).random((B, K)) > 0.1).astype(np.uint8)
    am[:, 0] = 1
    mask = R.decode_mask(B, 1, K, cache_index, am)
    md = torch.from_numpy(mask.astype(np.uint8)).cuda()
    (kq, ks), (vq, vs) = _quant(k), _quant(v)
    out, lse = _decode(q, kq, ks, vq, vs, md, splits)
    kd, vd = kv4.kv4_dequant(kq, ks), kv4.kv4_dequant(vq, vs)
    ro, rl = R.dense_attention(_np(q), _np(kd), _np(vd), causal=False, dense_mask=mask)
    e_out, e_lse = np.abs(_np(out) - ro).max() / np.abs(ro).max(), np.abs(_np(lse) - rl).max()
    ob, lb = ops.attn_combine(*ops.attn_fwd_splitk(q, kd, vd, k_splits=splits, dense_mask=md))
    e_bf = (out.float() - ob.float()).abs().max().item() / np.abs(ro).max()
    e_lb = (lse - lb).abs().max().item()
    print(f"kv4 decode B={B} K={K} H={H} splits={splits}: vs oracle out {e_out:.3e} lse {e_lse:.3e}; vs bf16 kernel {e_bf:.3e} "
          f"lse {e_lb:.3e}")
    assert e_out <= 2e-2
    assert e_lse <= 2e-3
    assert e_bf <= 1.6e-2
    assert e_lb <= 2e-3


def test_decode_mask_behaviour():
    """garbage under the mask -- 0xFF nibble bytes and 0xFF scale bytes included -- leaves the outputs torch.equal; a
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
    full, _ = _decode(q, kq, ks, vq, vs, None, 6)
    assert not torch.equal(full, out)
    o0, l0 = _decode(q, kq, ks, vq, vs, torch.zeros_like(mask), 6)
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


def test_init_cache_fp4_layout():
    import torch
    cfg, model = _model()
    cache = model.init_cache(2, 64, kv_dtype="fp4")
    assert len(cache) == cfg.num_hidden_layers
    H = cfg.num_attention_heads
    for c in cache:
        for n in ("cached_key", "cached_value"):
            assert c[n].dtype == torch.uint8 and tuple(c[n].shape) == (2, 64, H, 64)
        for n in ("key_scale_e8m0", "value_scale_e8m0"):
            assert c[n].dtype == torch.uint8 and tuple(c[n].shape) == (2, 64, H, 4)
        assert "key_scale" not in c and c["cache_index"] == 0
    for other in (model.init_cache(2, 64)[0], model.init_cache(2, 64, kv_dtype="fp8")[0]):
        assert not any(n.endswith("_e8m0") for n in other)          # the default and the fp8 caches are what they were


def test_generate_fp4_graph_equals_eager():
    import torch
    cfg, model = _model()
    seq, mask, PL, NEW = _prompt()
    eager, le = model.generate(seq[:, :PL], attention_mask=mask, max_new_tokens=NEW, return_logits=True, kv_dtype="fp4")
    graph, lg = model.generate(seq[:, :PL], attention_mask=mask, max_new_tokens=NEW, return_logits=True, kv_dtype="fp4",
                               graph=True)
    d = (lg - le).abs().max().item() / le.abs().max().item()
    print(f"fp4 cache, graph against eager: logits differ by {d:.3e} of max")
    assert torch.equal(graph, eager)
    assert d <= 1e-3


def test_fp4_cache_steps_equal_a_bf16_cache_holding_the_same_numbers(monkeypatch):
    """hidden_states stepped by hand: a 4-bit cache against a bf16 cache that holds identical numbers at every step.  The
    reference run wraps LLaMAAttention._cached: a one-token step's xk, xv are replaced by kv4_dequant(quantise(.)) before
    the call, and after a prompt call its rows in the cache are replaced likewise -- the prompt itself attends over its
    unquantised keys on both sides.  (At 4 bits one unrounded row is far outside a route-difference bound, so unlike the
    kv8 test the bf16 step does not see its own row unrounded.)  The per-step logits differ by the two decode routes only:
    2e-2 of max, with LWM_DECODE_FUSED 1 and 0.  Then the cost of quantisation itself against the plain bf16 cache,
    printed, not gated."""
    import torch
    from lwm_amd import kv4
    from lwm_amd.llama import LLaMAAttention
    cfg, model = _model()
    seq, mask, PL, NEW = _prompt()
    L = PL + NEW
    ext = torch.ones(1, L, dtype=torch.int32, device="cuda")
    ext[:, :PL] = mask
    orig = LLaMAAttention._cached
    rnd = lambda t: kv4.kv4_dequant(*_quant(t.contiguous()))

    def same_numbers(self, xq, xk, xv, attention_mask, cache):
        Q = xq.shape[1]
        if Q == 1:
            return orig(self, xq, rnd(xk), rnd(xv), attention_mask, cache)
        i0 = int(cache["cache_index"])
        out = orig(self, xq, xk, xv, attention_mask, cache)
        for n in ("cached_key", "cached_value"):
            cache[n][:, i0:i0 + Q] = rnd(cache[n][:, i0:i0 + Q])
        return out

    def run(kind, fused):
        monkeypatch.setenv("LWM_DECODE_FUSED", "1" if fused else "0")
        monkeypatch.setattr(LLaMAAttention, "_cached", same_numbers if kind == "bf16-same-numbers" else orig)
        cache = model.init_cache(1, L, kv_dtype="fp4" if kind == "fp4" else None)
        pos = (mask.cumsum(-1) - 1).clamp_min(0).to(torch.int32).contiguous()
        step_in, logits = seq[:, :PL], []
        with torch.no_grad():
            for t in range(NEW):
                h = model.hidden_states(step_in, ext, None, pos, cache)
                logits.append((h[:, -1].float() @ model.lm_head.float()).cpu())
                step_in, pos = seq[:, PL + t:PL + t + 1], (pos[:, -1:] + 1).contiguous()
        assert all(c["cache_index"] == L - 1 for c in cache)
        return torch.stack(logits, 1)

    for fused in (True, False):
        l4, ld = run("fp4", fused), run("bf16-same-numbers", fused)
        d = ((l4 - ld).abs().amax(-1) / ld.abs().max()).flatten()
        print(f"fp4 cache against a bf16 cache holding the same numbers (fused={fused}): per-step logit difference of max "
              f"{[f'{x:.2e}' for x in d.tolist()]}")
        assert d.max().item() <= 2e-2
    lb = run("bf16", True)
    d = ((l4 - lb).abs().amax(-1) / lb.abs().max()).flatten()
    agree = (l4.argmax(-1) == lb.argmax(-1)).float().mean().item()
    print(f"COST fp4 cache against the bf16 cache (teacher forced, {NEW} steps): per-step logit difference of max "
          f"{[f'{x:.2e}' for x in d.tolist()]}; argmax agreement {agree:.3f}")


def test_seeded_sampling_with_fp4_cache_is_reproducible():
    import torch
    from lwm_amd.vision_llama import VideoLLaMAConfig, VideoLLaMAForCausalLM
    torch.manual_seed(0)
    cfg = VideoLLaMAConfig(vocab_size=384, hidden_size=256, intermediate_size=512, num_hidden_layers=2,
                           num_attention_heads=2, max_sequence_length=512, vision_vocab_size=64, sample_mode="text")
    model = VideoLLaMAForCausalLM(cfg).cuda()
    ids = torch.randint(0, 384, (2, 24), device="cuda")
    kw = dict(max_new_tokens=12, do_sample=True, temperature=0.9, top_k=50, seed=1234, kv_dtype="fp4")
    a = model.generate(ids, **kw)
    b = model.generate(ids, **kw)
    g = model.generate(ids, graph=True, **kw)
    g2 = model.generate(ids, graph=True, **kw)
    assert torch.equal(a, b) and torch.equal(g, g2)
    assert a.shape == (2, 12) and g.shape == (2, 12)
    c = model.generate(ids, **{**kw, "seed": 99})
    assert not torch.equal(a, c)


def test_refused_cases_are_named(monkeypatch):
    import torch
    from lwm_amd.llama import LLaMAForCausalLM
    from lwm_amd import weights as W
    import hf_fixture as F
    cfg, model = _model()
    with pytest.raises(ValueError, match="'fp8' or 'fp4'"):
        model.init_cache(1, 32, kv_dtype="int4")
    f32 = LLaMAForCausalLM(W.config_from_hf(F.HF_CONFIG), dtype=torch.float32).cuda()
    with pytest.raises(NotImplementedError, match="float32"):
        f32.init_cache(1, 32, kv_dtype="fp4")
    with pytest.raises(NotImplementedError, match="float32"):
        f32.generate(torch.zeros(1, 4, dtype=torch.int64, device="cuda"), max_new_tokens=2, kv_dtype="fp4")
    # chunked prefill: the cache flag and generate's block length
    with pytest.raises(NotImplementedError, match="block kernel over the 4-bit cache is not built"):
        model.init_cache(1, 32, kv_dtype="fp4", chunked_prefill=True)
    with pytest.raises(NotImplementedError, match="block kernel over the 4-bit cache is not built"):
        model.generate(torch.zeros(1, 8, dtype=torch.int64, device="cuda"), max_new_tokens=2, kv_dtype="fp4", prefill_chunk=4)
    # a block of tokens after the prompt
    cache = model.init_cache(1, 32, kv_dtype="fp4")
    ids = torch.randint(0, 384, (1, 8), device="cuda")
    pos = torch.arange(8, dtype=torch.int32, device="cuda")[None]
    with torch.no_grad():
        model.hidden_states(ids, None, None, pos, cache)
        with pytest.raises(NotImplementedError, match="Q > 1 at cache_index > 0"):
            model.hidden_states(ids[:, :3], None, None, pos[:, :3] + 8, cache)
    # another head_dim (a config refuses it when it is made; the cache checks what it is given)
    monkeypatch.setattr(model.cfg, "num_attention_heads", 2 * cfg.num_attention_heads)
    with pytest.raises(NotImplementedError, match="head_dim 64"):
        model.init_cache(1, 32, kv_dtype="fp4")
    monkeypatch.undo()
    # a sequence ring
    from lwm_amd import llama as M
    monkeypatch.setattr(M, "sp_size_rank", lambda axis: (2, 0))
    with pytest.raises(NotImplementedError, match="sp > 1"):
        model.init_cache(1, 32, kv_dtype="fp4")


def test_cli_accepts_fp4(monkeypatch):
    import torch
    from lwm_amd.cli import _common

    class _Model:
        dtype = torch.bfloat16
    for v in ("LWM_PREFILL_CHUNK", "LWM_DECODE_GRAPH"):
        monkeypatch.delenv(v, raising=False)
    gen = object()
    monkeypatch.setenv("LWM_KV_CACHE", "fp4")
    assert _common.sampler_kwargs(_Model(), 7, gen) == dict(generator=gen, kv_dtype="fp4")
    monkeypatch.setenv("LWM_DECODE_GRAPH", "1")
    assert _common.sampler_kwargs(_Model(), 7, gen) == dict(seed=7, graph=True, kv_dtype="fp4")
    monkeypatch.setenv("LWM_KV_CACHE", "fp2")
    with pytest.raises(SystemExit, match="'fp4', 'fp8', 'bf16'"):
        _common.sampler_kwargs(_Model(), 7, gen)
