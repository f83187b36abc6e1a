"""The token sampler on the MI355X: the device kernel (ops.sample_tokens, csrc/sample.h) against the numpy restatement
of tests/_sample_ref.py token for token, its distribution, and the seed-driven decode paths of VideoLLaMAForCausalLM --
eager and captured in a hipGraph -- down to the entry points."""
import math

import numpy as np
import pytest

from tests import _sample_ref as R
from tests.test_emu_sample import GRID, _logits

pytestmark = pytest.mark.gpu


def _dev_sample(lg, *, cfg=None, step_dev=None, done=None, copies=1, seq_cols=0, **kw):
    import torch
    from lwm_amd import ops
    d = torch.from_numpy(lg).cuda()
    rows = lg.shape[0]
    B = rows // 2 if cfg is not None else rows
    cf = None if cfg is None else torch.tensor(np.broadcast_to(np.asarray(cfg, np.float32), (B,)).copy()).cuda()
    sd = None if step_dev is None else torch.tensor([step_dev], dtype=torch.int32).cuda()
    dn = None if done is None else torch.from_numpy(np.asarray(done, np.uint8)).cuda()
    seq = None if not seq_cols else torch.full((B, seq_cols), -7, dtype=torch.int64).cuda()
    toks = ops.sample_tokens(d, cfg_scale=cf, step_dev=sd, done=dn, copies=copies, seq_out=seq, **kw)
    return (toks.cpu().numpy().reshape(copies, B), None if dn is None else dn.cpu().numpy(),
            None if seq is None else seq.cpu().numpy())


@pytest.mark.parametrize("V,rows,cfg,T,k", GRID)
def test_device_kernel_matches_numpy_reference(V, rows, cfg, T, k):
    rng = np.random.default_rng(V * 7 + rows * 131 + int(T * 10) + k)
    lg = _logits(rng, rows, V, neg_inf=0 if cfg else min(5, V // 4))
    seed, step = 0x5EED0000 + V + k, 17 + rows
    toks, _, _ = _dev_sample(lg, temperature=T, top_k=k, seed=seed, step=step, cfg=cfg)
    ref, _, near = R.sample(lg, temperature=T, top_k=k, seed=seed, step=step, cfg=cfg)
    assert near == 0
    assert np.array_equal(toks[0], ref), (toks[0], ref)


def test_device_bookkeeping_matches_reference():
    """done / pad / eos latching, forced code at every 257th token, copies = 2, the seq column, device step"""
    rng = np.random.default_rng(9)
    lg = _logits(rng, 4, 8448)
    base = dict(temperature=1.0, top_k=8192, seed=1234, cfg=(5.0, 1.0), force_period=257, force_token=8192, copies=2,
                seq_cols=600)
    for step in (255, 256, 513):
        toks, _, seq = _dev_sample(lg, step=step, **base)
        ref, _, near = R.sample(lg, temperature=1.0, top_k=8192, seed=1234, step=step, cfg=(5.0, 1.0), force_period=257,
                                force_token=8192)
        assert near == 0 and np.array_equal(toks[0], ref) and np.array_equal(toks[1], ref)
        assert np.array_equal(seq[:, step], ref) and (np.delete(seq, step, 1) == -7).all()
        toks_d, _, seq_d = _dev_sample(lg, step=0, step_dev=step + 1000, step_base=1000, **base)
        assert np.array_equal(toks_d, toks) and np.array_equal(seq_d, seq)
    lg = _logits(rng, 4, 37)
    eos = int(np.argmax(lg[2]))
    done = np.array([0, 1, 0, 0], np.uint8)
    toks, dn, _ = _dev_sample(lg, temperature=0.0, top_k=0, seed=0, step=0, done=done, eos=eos, pad=33)
    ref, rdone, _ = R.sample(lg, temperature=0.0, top_k=0, seed=0, step=0, done=done, eos=eos, pad=33)
    assert np.array_equal(toks[0], ref) and np.array_equal(dn, rdone) and toks[0, 1] == 33


def _chi2_sf(x, k):
    """upper tail of chi-square with k degrees of freedom (Wilson-Hilferty)"""
    z = ((x / k) ** (1 / 3) - (1 - 2 / (9 * k))) / math.sqrt(2 / (9 * k))
    return 0.5 * math.erfc(z / math.sqrt(2))


@pytest.mark.parametrize("V,T,k", [(8448, 1.0, 1000), (32000, 0.2, 0)])
def test_distribution_of_draws(V, T, k):
    """>= 1e5 draws of ONE row (the row replicated over 1000 output rows, 100 steps): chi-square against
    softmax(filtered / T) at p > 1e-4 (fixed seed: the outcome is deterministic); nothing outside the top-k set"""
    import torch
    from lwm_amd import ops
    rng = np.random.default_rng(V)
    row = (rng.standard_normal(V) * (2.0 if T >= 1 else 0.5)).astype(np.float32)
    rows, steps = 1000, 100
    d = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(row, (rows, V)))).cuda()
    out = torch.empty((steps, rows), dtype=torch.int64, device="cuda")
    for s in range(steps):
        ops.sample_tokens(d, temperature=T, top_k=k, seed=777, step=s, tokens_out=out[s])
    counts = np.bincount(out.cpu().numpy().ravel(), minlength=V).astype(np.float64)
    s = row.astype(np.float64) / np.float32(T)
    keep = np.ones(V, bool)
    if 0 < k < V:
        keep = (row / np.float32(T)) >= np.sort(row / np.float32(T))[V - k]
        assert counts[~keep].sum() == 0
    p = np.where(keep, np.exp(s - s[keep].max()), 0.0)
    p /= p.sum()
    n = counts.sum()
    assert n == rows * steps
    exp = p * n
    big = exp >= 5
    obs_b, exp_b = list(counts[big]), list(exp[big])
    if (~big & keep).any():                   # the small-probability entries pooled into one bin
        obs_b.append(counts[~big & keep].sum())
        exp_b.append(exp[~big & keep].sum())
    obs_b, exp_b = np.array(obs_b), np.array(exp_b)
    x = float(((obs_b - exp_b) ** 2 / exp_b).sum())
    dof = len(obs_b) - 1
    assert dof >= 10
    assert _chi2_sf(x, dof) > 1e-4, (x, dof)


def test_greedy_cases_are_argmax():
    import torch
    from lwm_amd import ops
    rng = np.random.default_rng(1)
    for V in (37, 8448, 32000):
        lg = torch.from_numpy(_logits(rng, 4, V)).cuda()
        ref = lg.argmax(-1)
        assert torch.equal(ops.sample_tokens(lg, temperature=0.0, top_k=0, seed=3)[:, 0], ref)
        assert torch.equal(ops.sample_tokens(lg, temperature=0.7, top_k=1, seed=3, step=5)[:, 0], ref)


def _vision_model(dtype, mode="vision", layers=2):
    import torch
    from lwm_amd.vision_llama import VideoLLaMAConfig, VideoLLaMAForCausalLM
    cfg = VideoLLaMAConfig(vocab_size=2048, hidden_size=256, intermediate_size=512, num_hidden_layers=layers,
                           num_attention_heads=2, max_sequence_length=4096, theta=1e7, scan_mlp=False, sample_mode=mode)
    torch.manual_seed(0)
    return VideoLLaMAForCausalLM(cfg, dtype).cuda()


def _prompts(B, S, vocab, seed):
    """(B, S) text-token prompts (ids < vocab: the wte rows of the model) and a key mask with one left-padded row"""
    import torch
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, vocab, (B, S), generator=g)
    am = torch.ones(B, S, dtype=torch.int32)
    am[-1, :5] = 0                                             # a left-padded row
    return ids.cuda(), am.cuda()


@pytest.mark.parametrize("B,cfg_scale", [(1, 1.0), (2, 5.0)])
def test_generate_vision_graph_equals_eager_seeded(B, cfg_scale):
    """seed=, graph=True against seed=, graph=False over two frames (514 new tokens): the same tokens and bit-identical
    logits at every step (same kernels, same order), the end-of-frame code at every 257th position"""
    import torch
    model = _vision_model(torch.bfloat16)
    ids, am = _prompts(2 * B, 40, 2048, B)
    vm = torch.zeros_like(ids, dtype=torch.bool)
    kw = dict(attention_mask=am, vision_masks=vm, max_new_tokens=514, temperature=1.0, top_k=100, seed=42,
              return_logits=True)
    eager, le = model.generate_vision(ids, [cfg_scale] * B, graph=False, **kw)
    graph, lg = model.generate_vision(ids, [cfg_scale] * B, graph=True, **kw)
    assert eager.shape == (B, 514) and le.shape == (2 * B, 514, 8448)
    assert torch.equal(eager, graph)
    assert torch.equal(le, lg)
    assert (eager[:, 256] == 8192).all() and (eager[:, 513] == 8192).all()
    assert len(torch.unique(eager)) > 50                      # draws, not a constant
    again = model.generate_vision(ids, [cfg_scale] * B, graph=True, **kw)[0]
    assert torch.equal(again, graph)                          # the seed reproduces the run
    other = model.generate_vision(ids, [cfg_scale] * B, graph=True, **dict(kw, seed=43))[0]
    assert not torch.equal(other, graph)


def test_text_generate_with_eos_graph_equals_eager_and_stops():
    import torch
    model = _vision_model(torch.bfloat16, mode="text")
    ids, am = _prompts(2, 30, 2048, 7)
    kw = dict(attention_mask=am, max_new_tokens=96, temperature=1.0, do_sample=True, seed=5, return_logits=True)
    free, _ = model.generate(ids, graph=False, **kw)
    row0 = free[0].tolist()
    e = next(i for i in range(3, 96) if row0[i] not in row0[:i])       # the first token of row 0 new at step >= 3
    eos = row0[e]
    for graph in (False, True):
        out, logits = model.generate(ids, graph=graph, eos_token_id=eos, pad_token_id=0, **kw)
        assert out.shape == (2, 96)
        assert out[0, :e + 1].tolist() == row0[:e + 1] and (out[0, e + 1:] == 0).all()     # pad after eos
        for r in range(2):
            hit = (out[r] == eos).nonzero()
            if len(hit):
                assert (out[r, int(hit[0]) + 1:] == 0).all()
        if graph:
            assert torch.equal(out, ref_out) and torch.equal(logits, ref_logits)
        ref_out, ref_logits = out, logits
    # one row that hits eos at step e: the loop stops within one check interval of it
    one = dict(kw, attention_mask=am[:1])
    row = model.generate(ids[:1], graph=True, **one)[0][0].tolist()
    e = next(i for i in range(3, 96) if row[i] not in row[:i])
    out, logits = model.generate(ids[:1], graph=True, eos_token_id=row[e], **one)
    every = model.DONE_CHECK_EVERY
    assert logits.shape[1] == (e // every + 1) * every < 96
    assert out[0, :e + 1].tolist() == row[:e + 1] and (out[0, e + 1:] == 0).all()


def test_fp32_model_samples_eagerly_and_refuses_graph():
    import torch
    model = _vision_model(torch.float32)
    ids, am = _prompts(2, 24, 2048, 3)
    out = model.generate_vision(ids, [3.0], attention_mask=am, max_new_tokens=20, temperature=1.0, top_k=50, seed=1)
    assert out.shape == (1, 20) and (out < 8448).all()
    with pytest.raises(NotImplementedError, match="bf16"):
        model.generate_vision(ids, [3.0], attention_mask=am, max_new_tokens=20, seed=1, graph=True)
    with pytest.raises(ValueError, match="seed"):
        model.generate_vision(ids, [3.0], attention_mask=am, max_new_tokens=20, graph=True)


def test_entry_points_with_decode_graph(tmp_path, monkeypatch):
    from lwm_amd.cli import vision_chat, vision_generation
    monkeypatch.setenv("LWM_DECODE_GRAPH", "1")
    small = ["--load_llama_config=debug", "--mesh_dim=1,-1,1,1", "--dtype=bf16", "--tokenizer=synthetic"]
    ans = vision_chat.main(small + ["--prompt=What is the video about?", "--input_file=synthetic:2", "--max_n_frames=2",
                                    "--update_llama_config=dict(sample_mode='text',max_sequence_length=2048,vocab_size=32000)"],
                           max_new_tokens=8)
    assert isinstance(ans, str)
    out = str(tmp_path / "img.npy")
    img = vision_generation.main(small + ["--prompt=Fireworks", f"--output_file={out}", "--n_frames=1", "--top_k_image=50",
                                          "--cfg_scale_image=5.0",
                                          "--update_llama_config=dict(sample_mode='vision',max_sequence_length=2048)"])
    assert img.shape == (1, 256, 256, 3) and img.dtype == np.uint8 and np.load(out).shape == (1, 256, 256, 3)
