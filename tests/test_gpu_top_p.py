"""Nucleus (top-p) sampling on the MI355X: the device kernel through ops.sample_tokens against the fp64 restatement of
tests/_top_p_ref.py (the cases of tests/test_emu_top_p.py), the distribution of its draws, and generate / generate_vision
with top_p on the eager torch sampler, the seed-driven route and the captured step."""
import numpy as np
import pytest

from tests import _top_p_ref as R
from tests.test_emu_top_p import CASES, DECIDABLE, DEEP, check_deep_case, check_grid_case, decidable_rows
from tests.test_gpu_sample import _chi2_sf, _dev_sample, _prompts, _vision_model

pytestmark = pytest.mark.gpu


def dev_top_p(lg, *, temperature, top_k, top_p, seed, step=0, cfg=None):
    """ops.sample_tokens with the struct's switch values (0 or >= 1: off) -> tokens (B,)"""
    off = not 0 < top_p < 1
    return _dev_sample(lg, temperature=temperature, top_k=top_k, top_p=None if off else top_p, seed=seed, step=step,
                       cfg=cfg)[0][0]


@pytest.mark.parametrize("V,rows,cfg,T,k,p", CASES)
def test_device_grid_token_for_token(V, rows, cfg, T, k, p):
    check_grid_case(dev_top_p, V, rows, cfg, T, k, p)


@pytest.mark.parametrize("V,rows,cfg,T,k,p", DEEP)
def test_device_deep_sums_band_acceptance(V, rows, cfg, T, k, p):
    check_deep_case(dev_top_p, V, rows, cfg, T, k, p)


@pytest.mark.parametrize("which", DECIDABLE)
def test_device_exactly_decidable_rows(which):
    decidable_rows(dev_top_p, which)


@pytest.mark.parametrize("V,T,k,p", [(8448, 1.0, 1000, 0.9), (32000, 0.2, 0, 0.95)])
def test_distribution_of_nucleus_draws(V, T, k, p):
    """1e5 draws of ONE row (replicated over 1000 output rows, 100 steps): nothing outside S+ is drawn; chi-square against
    the renormalised nucleus distribution with the statistic, pooling and 1e-4 tail of test_distribution_of_draws, the
    entries of the band (at most 8) left out of it"""
    import torch
    from lwm_amd import ops
    rng = np.random.default_rng(V)
    row = (rng.standard_normal(V) * (2.0 if T >= 1 else 0.5)).astype(np.float32)
    rows, steps = 1000, 100
    d = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(row, (rows, V)))).cuda()
    out = torch.empty((steps, rows), dtype=torch.int64, device="cuda")
    for s in range(steps):
        ops.sample_tokens(d, temperature=T, top_k=k, top_p=p, seed=777, step=s, tokens_out=out[s])
    counts = np.bincount(out.cpu().numpy().ravel(), minlength=V).astype(np.float64)
    s32 = (row / np.float32(T)).astype(np.float32)
    lo, hi, _ = R.top_p_sets(s32, R.top_k_keep(s32, k), p)
    band = hi & ~lo
    assert band.sum() <= 8
    assert counts[~hi].sum() == 0
    assert 1 < lo.sum() < R.top_k_keep(s32, k).sum()          # the nucleus filters, and not down to one entry
    s = s32.astype(np.float64)
    keep = lo
    pr = np.where(keep, np.exp(s - s[keep].max()), 0.0)
    pr /= pr.sum()
    n = counts[keep].sum()
    assert n + counts[band].sum() == rows * steps
    exp = pr * n
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


def test_device_determinism_and_batch_independence():
    """the same call twice gives the same tokens; a row's token in a batch of 1 is its token in a batch of 4 (same row
    index: row 0)"""
    rng = np.random.default_rng(12)
    lg = (rng.standard_normal((4, 32000)) * 3.0).astype(np.float32)
    kw = dict(temperature=1.0, top_k=0, top_p=0.9, seed=21)
    for step in range(6):
        four = dev_top_p(lg, step=step, **kw)
        assert np.array_equal(four, dev_top_p(lg, step=step, **kw))
        assert dev_top_p(lg[:1], step=step, **kw)[0] == four[0]


def _in_s_plus(logits, tokens, T, k, p, cfg=None):
    """every token (B, steps) lies in S+ of its step's logits (rows, steps, V)"""
    lg = logits.float().cpu().numpy()
    tk = tokens.cpu().numpy()
    for i in range(tk.shape[1]):
        mixed = R.mixed_logits(lg[:, i], cfg)
        for b in range(tk.shape[0]):
            s = (mixed[b] / np.float32(T)).astype(np.float32)
            hi = R.top_p_sets(s, R.top_k_keep(s, k), p)[1]
            if not hi[int(tk[b, i])]:
                return False, (b, i, int(tk[b, i]))
    return True, None


def test_generate_vision_top_p_graph_equals_eager_and_stays_in_the_nucleus():
    import torch
    model = _vision_model(torch.bfloat16)
    ids, am = _prompts(4, 40, 2048, 2)
    vm = torch.zeros_like(ids, dtype=torch.bool)
    kw = dict(attention_mask=am, vision_masks=vm, max_new_tokens=40, temperature=1.0, top_k=100, seed=42, return_logits=True)
    eager, le = model.generate_vision(ids, [5.0, 5.0], graph=False, top_p=0.9, **kw)
    graph, lg = model.generate_vision(ids, [5.0, 5.0], graph=True, top_p=0.9, **kw)
    assert torch.equal(eager, graph) and torch.equal(le, lg)
    assert torch.equal(graph, model.generate_vision(ids, [5.0, 5.0], graph=True, top_p=0.9, **kw)[0])
    ok, where = _in_s_plus(le, eager, 1.0, 100, 0.9, cfg=(5.0, 5.0))
    assert ok, where
    plain = model.generate_vision(ids, [5.0, 5.0], graph=True, **kw)[0]
    assert not torch.equal(plain, graph)                      # the filter changes draws
    for off in (None, 1.0):                                   # off is off, on the seeded and the captured route
        for g in (False, True):
            assert torch.equal(model.generate_vision(ids, [5.0, 5.0], graph=g, top_p=off, **kw)[0], plain)
    # the 8-bit KV cache composes
    e8 = model.generate_vision(ids, [5.0, 5.0], graph=False, top_p=0.9, kv_dtype="fp8", **kw)[0]
    g8 = model.generate_vision(ids, [5.0, 5.0], graph=True, top_p=0.9, kv_dtype="fp8", **kw)[0]
    assert torch.equal(e8, g8)


def test_text_generate_top_p_graph_equals_eager_and_stops():
    import torch
    model = _vision_model(torch.bfloat16, mode="text")
    ids, am = _prompts(2, 30, 2048, 7)
    kw = dict(attention_mask=am, max_new_tokens=48, temperature=1.0, do_sample=True, seed=5, top_p=0.8, return_logits=True)
    free, lf = model.generate(ids, graph=False, **kw)
    ok, where = _in_s_plus(lf, free, 1.0, 0, 0.8)
    assert ok, where
    row0 = free[0].tolist()
    e = next(i for i in range(3, 48) if row0[i] not in row0[:i])       # the first token of row 0 new at step >= 3
    eos = row0[e]
    outs = [model.generate(ids, graph=g, eos_token_id=eos, pad_token_id=0, **kw) for g in (False, True)]
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    out = outs[1][0]
    assert out[0, :e + 1].tolist() == row0[:e + 1] and (out[0, e + 1:] == 0).all()     # it stops: pad after eos
    # one row: the loop itself ends within one check interval of the eos
    one = dict(kw, attention_mask=am[:1])
    row = model.generate(ids[:1], graph=True, **one)[0][0].tolist()
    e = next(i for i in range(3, 48) if row[i] not in row[:i])
    out, logits = model.generate(ids[:1], graph=True, eos_token_id=row[e], **one)
    every = model.DONE_CHECK_EVERY
    assert logits.shape[1] == (e // every + 1) * every <= 48
    # off is off on all three routes
    base = dict(attention_mask=am, max_new_tokens=24, temperature=1.0, do_sample=True)
    for route in (dict(seed=5), dict(seed=5, graph=True)):
        ref = model.generate(ids, **base, **route)
        for off in (None, 1.0):
            assert torch.equal(model.generate(ids, top_p=off, **base, **route), ref)
    gen = lambda: torch.Generator(device="cuda").manual_seed(3)
    ref = model.generate(ids, generator=gen(), **base)
    for off in (None, 1.0):
        assert torch.equal(model.generate(ids, generator=gen(), top_p=off, **base), ref)


def test_torch_sampler_route_only_emits_nucleus_tokens():
    import torch
    model = _vision_model(torch.bfloat16, mode="text")
    ids, am = _prompts(2, 30, 2048, 9)
    out, logits = model.generate(ids, attention_mask=am, max_new_tokens=48, temperature=1.0, do_sample=True, top_p=0.5,
                                 generator=torch.Generator(device="cuda").manual_seed(1), return_logits=True)
    ok, where = _in_s_plus(logits, out, 1.0, 0, 0.5)
    assert ok, where
    vmodel = _vision_model(torch.bfloat16)
    vids, vam = _prompts(2, 24, 2048, 4)
    out, logits = vmodel.generate_vision(vids, [3.0], attention_mask=vam, max_new_tokens=32, temperature=1.0, top_k=200,
                                         top_p=0.7, generator=torch.Generator(device="cuda").manual_seed(2),
                                         return_logits=True)
    ok, where = _in_s_plus(logits, out, 1.0, 200, 0.7, cfg=(3.0,))
    assert ok, where
