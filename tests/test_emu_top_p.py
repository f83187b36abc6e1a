"""Nucleus (top-p) sampling of the token sampler (lwm_sample_tokens, lwm_amd/csrc/sample.h; the rule and its eps are in
include/lwm_hip.h) in the host emulation, through the C ABI, against the fp64 restatement of tests/_top_p_ref.py: token
for token where the threshold is decided by more than the band, by band acceptance where the sums are deep; rows whose
keep set is known exactly; top-p off = the launch as it was; the validation of the real library; the refusals of
ops.sample_tokens / generate and LWM_TOP_P, which need no device."""
import ctypes as C
import math
import os
import types
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from lwm_amd import _capi
from tests import _emu
from tests import _top_p_ref as R
from tests.test_emu_sample import GRID, _logits, emu_sample, real_lib  # noqa: F401  (real_lib: a fixture)

EPS = R.TOP_P_EPS

# (V, rows, cfg scales or None, T, k, p): V below / at / past the register-held entries, guidance on and off, every T, top-k
# off / small / large under the nucleus, p from 0.1 to 0.95
CASES = [(37, 1, None, 1.0, 0, 0.9), (37, 4, (5.0, 0.5), 3.0, 0, 0.5), (8448, 2, (1.0,), 0.2, 0, 0.95),
         (8448, 4, None, 1.0, 50, 0.9), (8448, 2, None, 3.0, 1000, 0.5), (32000, 4, (1.5, 7.0), 1.0, 0, 0.5),
         (32000, 2, None, 1.0, 1000, 0.5), (32000, 1, None, 3.0, 50, 0.95), (40000, 2, (2.0,), 1.0, 100, 0.9),
         (40000, 1, None, 0.2, 0, 0.95), (8448, 2, None, 1.0, 0, 0.1)]
# deep sums: about 19600 and 6300 entries stay and the fp64 margin is about 1e-6
DEEP = [(32000, 2, None, 3.0, 0, 0.9), (40000, 1, None, 3.0, 0, 0.5)]
STEPS = (0, 5, 18)


def emu_top_p(logits, *, temperature, top_k, top_p, seed, step=0, cfg=None, ld_pad=3):
    """lwm_sample_tokens on the emulated kernel with LwmSampleArgs.top_p = top_p (the struct's own switch values: 0 or
    >= 1 is off).  Rows ld_pad NaN columns apart.  -> tokens (B,)"""
    L = _emu.lib()
    rows, V = logits.shape
    B = rows // 2 if cfg is not None else rows
    buf = _emu.aligned((rows, V + ld_pad), np.float32)
    buf[:] = np.nan
    buf[:, :V] = logits
    a = _capi.LwmSampleArgs()
    a.logits, a.ld, a.rows, a.V = buf.ctypes.data, V + ld_pad, rows, V
    if cfg is not None:
        cf = _emu.aligned((B,), np.float32)
        cf[:] = cfg
        a.cfg_scale = cf.ctypes.data
    a.temperature, a.top_k, a.top_p, a.seed, a.step = temperature, top_k, top_p, seed, step
    a.eos = -1
    toks = _emu.aligned((1, B), np.int64)
    toks[:] = -1
    a.tokens, a.copies = toks.ctypes.data, 1
    _capi.check(L, L.lwm_sample_tokens(C.byref(a), None), "lwm_sample_tokens")
    return toks[0].copy()


def threaded(fn, items):
    """map for the emulated sampler: a launch costs a few tenths of a second whatever V is (a fibre per lane) and holds
    no lock, so independent launches run side by side"""
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
        return list(ex.map(fn, items))


def scaled_rows(lg, cfg, T):
    """the f32 s = logit / T of every output row"""
    return (R.mixed_logits(lg, cfg) / np.float32(T)).astype(np.float32)


def row_sets(lg, cfg, T, k, p, eps=EPS):
    """[(s, S_minus, S_plus, margin)] per output row"""
    out = []
    for s in scaled_rows(lg, cfg, T):
        lo, hi, margin = R.top_p_sets(s, R.top_k_keep(s, k), p, eps)
        out.append((s, lo, hi, margin))
    return out


def case_logits(V, rows, cfg, T, k, p, need=4 * EPS):
    """the logits of a case: the first draw t of range(64) at which every row's threshold is decided by `need` (None: t =
    0 whatever the margin).  -> (logits, t or None when no draw qualifies)"""
    for t in range(64):
        lg = (np.random.default_rng([V, rows, int(T * 10), k, int(p * 1000), t]).standard_normal((rows, V)) * 3.0
              ).astype(np.float32)
        if need is None or all(m >= need for _, _, _, m in row_sets(lg, cfg, T, k, p)):
            return lg, t
    return None, None


def check_grid_case(sampler, V, rows, cfg, T, k, p, pmap=map):
    """`sampler(lg, temperature=, top_k=, top_p=, seed=, step=, cfg=) -> tokens (B,)` against the restatement; pmap
    maps it over the independent launches of the case"""
    lg, t = case_logits(V, rows, cfg, T, k, p)
    assert t is not None, "no draw of the logits decides every row's threshold by 4 eps"
    for _, lo, hi, _ in row_sets(lg, cfg, T, k, p):
        assert np.array_equal(lo, hi)                      # so the expected token is unique
    seed = 0x70B0000 + V + k
    got = list(pmap(lambda step: sampler(lg, temperature=T, top_k=k, top_p=p, seed=seed, step=step, cfg=cfg), STEPS))
    for step, toks in zip(STEPS, got):
        ref, _, near = R.sample(lg, temperature=T, top_k=k, top_p=p, seed=seed, step=step, cfg=cfg)
        assert near == 0
        assert np.array_equal(toks, ref), (step, toks, ref)


def check_deep_case(sampler, V, rows, cfg, T, k, p, steps=64, pmap=map):
    lg, _ = case_logits(V, rows, cfg, T, k, p, need=None)
    sets = row_sets(lg, cfg, T, k, p)
    for _, lo, hi, _ in sets:
        assert (hi & ~lo).sum() <= 8                       # a condition of the test: the band cannot hide a wrong threshold
        assert lo.sum() > 4096                             # deep: every lane holds kept entries
    got = list(pmap(lambda step: sampler(lg, temperature=T, top_k=k, top_p=p, seed=99, step=step, cfg=cfg), range(steps)))
    for step, toks in enumerate(got):
        for b, (s, lo, hi, _) in enumerate(sets):
            assert int(toks[b]) in R.band_tokens(s, lo, hi, b, 99, step), (step, b, int(toks[b]))


DECIDABLE = ("zeros among -inf", "one dominant entry", "two levels", "one finite entry", "tied k-th value")


def decidable_rows(sampler, which, pmap=map):
    """rows whose keep set needs no arithmetic to know; `which`: one of DECIDABLE"""
    V = 8448
    assert which in DECIDABLE

    def draws(lg, steps, **kw):
        """[tokens (B,)] of the steps"""
        return list(pmap(lambda step: sampler(lg, step=step, **kw), range(steps)))

    if which == "zeros among -inf":      # n entries at 0 and the rest -inf: all n stay for every p, and all are drawn
        return _zeros_among_neg_inf(draws, V)
    if which == "one dominant entry":    # 30 above the rest: it holds all but 1e-9 of the mass
        lg = np.zeros((1, V), np.float32)
        lg[:, 5001] = 30.0
        for seed in (1, 2, 3):
            assert all(t.tolist() == [5001] for t in draws(lg, 4, temperature=1.0, top_k=0, top_p=0.9, seed=seed))
        return
    if which == "two levels":            # m entries at 0, the rest at -20; p just under the top group's share
        m = 7
        lg = np.full((1, V), -20.0, np.float32)
        top = np.arange(m) * 1200 + 11
        lg[0, top] = 0.0
        share = m / (m + (V - m) * math.exp(-20.0))
        seen = {int(t[0]) for t in draws(lg, 16, temperature=1.0, top_k=0, top_p=share * (1 - 1e-3), seed=8)}
        assert seen <= set(top.tolist()) and len(seen) > 1, seen      # the group alone stays
        return
    if which == "one finite entry":      # it is the token for any p and k
        one = np.full((1, 37), -np.inf, np.float32)
        one[0, 29] = -1e30
        for k in (0, 1, 5):
            for p in (0.01, 0.999):
                assert sampler(one, temperature=1.0, top_k=k, top_p=p, seed=1, step=0).tolist() == [29]
        return
    _tied_kth_value(draws, V)


def _zeros_among_neg_inf(draws, V):
    lg = np.full((1, V), -np.inf, np.float32)
    at = np.array([3, 4095, 4096, 8447])
    lg[:, at] = 0.0
    for p in (0.05, 0.99):
        seen = {int(t[0]) for t in draws(lg, 40, temperature=1.0, top_k=0, top_p=p, seed=5)}
        assert seen == set(at.tolist()), (p, seen)


def _tied_kth_value(draws, V):
    # top-k and top-p together with the k-th value tied (the rows of test_ties_at_the_kth_value_and_neg_inf_entries):
    # 35 entries above 100 tied at 2.5, k = 50 lands inside the tie -> K has 135 entries; p = 0.97 keeps the tie, 0.3 not
    rng = np.random.default_rng(3)
    lg = np.full((2, V), -np.inf, np.float32)
    lg[:, :600] = rng.standard_normal((2, 600)).astype(np.float32)
    lg[:, 600:700] = 2.5
    lg[:, :600][lg[:, :600] > 2.5] = 0.0
    lg[:, 5:40] = 3.0 + np.arange(35, dtype=np.float32) / 64
    for p, tied_stay in ((0.97, True), (0.3, False)):
        for s, lo, hi, margin in row_sets(lg, None, 1.0, 50, p):
            assert margin >= 4 * EPS and lo[600:700].all() == tied_stay and lo[600:700].any() == tied_stay
            assert not lo[:5].any() and not lo[40:600].any()
        seen = set()
        for step, toks in enumerate(draws(lg, 16, temperature=1.0, top_k=50, top_p=p, seed=11)):
            ref, _, near = R.sample(lg, temperature=1.0, top_k=50, top_p=p, seed=11, step=step)
            assert near == 0 and np.array_equal(toks, ref)
            seen |= set(toks.tolist())
        assert all(5 <= t < 40 or (tied_stay and 600 <= t < 700) for t in seen)
        assert any(600 <= t < 700 for t in seen) == tied_stay


@pytest.mark.parametrize("V,rows,cfg,T,k,p", CASES)
def test_grid_token_for_token(V, rows, cfg, T, k, p):
    check_grid_case(emu_top_p, V, rows, cfg, T, k, p, pmap=threaded)


@pytest.mark.parametrize("V,rows,cfg,T,k,p", DEEP)
def test_deep_sums_band_acceptance(V, rows, cfg, T, k, p):
    check_deep_case(emu_top_p, V, rows, cfg, T, k, p, pmap=threaded)


def test_restatement_rejects_unfiltered_draws_of_the_deep_cases():
    """what makes the band test bite: a sampler that ignored top_p would be refused on a visible share of the draws"""
    for (V, rows, cfg, T, k, p), least in zip(DEEP, (3, 20)):
        lg, _ = case_logits(V, rows, cfg, T, k, p, need=None)
        s, lo, hi, _ = row_sets(lg, cfg, T, k, p)[0]
        out = sum(int(R.sample(lg[:1], temperature=T, top_k=k, seed=99, step=st)[0][0]) not in
                  R.band_tokens(s, lo, hi, 0, 99, st) for st in range(64))
        assert out >= least, out


@pytest.mark.parametrize("which", DECIDABLE)
def test_exactly_decidable_rows(which):
    decidable_rows(emu_top_p, which, pmap=threaded)


@pytest.mark.parametrize("V,rows,cfg,T,k", GRID)
def test_off_is_off(V, rows, cfg, T, k):
    """top_p = 0, 1 and 2 in the struct: the tokens of a call that never sets the field"""
    rng = np.random.default_rng(V * 7 + rows * 131 + int(T * 10) + k)
    lg = _logits(rng, rows, V, neg_inf=0 if cfg else min(5, V // 4))
    seed, step = 0x5EED0000 + V + k, 17 + rows
    base = emu_sample(lg, temperature=T, top_k=k, seed=seed, step=step, cfg=cfg)[0][0]
    for off in (0.0, 1.0, 2.0):
        assert np.array_equal(emu_top_p(lg, temperature=T, top_k=k, top_p=off, seed=seed, step=step, cfg=cfg), base), off


def test_greedy_ignores_top_p():
    lg = _logits(np.random.default_rng(2), 4, 8448)
    assert np.array_equal(emu_top_p(lg, temperature=0.0, top_k=0, top_p=0.5, seed=3), lg.argmax(-1))


def test_validation_on_the_real_library(real_lib):
    L = real_lib
    assert L.lwm_sizeof(4) == C.sizeof(_capi.LwmSampleArgs)
    assert L.lwm_version() >= 590
    buf = (C.c_char * 4096)()
    base = C.addressof(buf)
    base += (-base) % 16
    for bad in (-0.25, -1e-30, float("nan"), float("-inf")):
        a = _capi.LwmSampleArgs()
        a.logits, a.ld, a.rows, a.V = base, 64, 2, 64
        a.temperature, a.top_k, a.top_p = 1.0, 0, bad
        a.tokens, a.copies = base + 2048, 1
        assert L.lwm_sample_tokens(C.byref(a), None) == _capi.LWM_EINVAL, bad
        assert L.lwm_last_error().startswith(b"sample_tokens") and b"top_p" in L.lwm_last_error(), bad


def test_restatement_against_transformers():
    try:
        import torch
        from transformers.generation.logits_process import TopPLogitsWarper
    except Exception as e:                                  # noqa: BLE001
        pytest.skip(f"transformers' TopPLogitsWarper does not import here ({type(e).__name__}: {e})")
    rng = np.random.default_rng(41)
    checked = 0
    for V, scale, p in ((37, 3.0, 0.9), (37, 1.0, 0.5), (300, 3.0, 0.95), (2048, 6.0, 0.5), (8448, 15.0, 0.9),
                        (32000, 12.0, 0.1)):
        for _ in range(6):
            s = (rng.standard_normal(V) * scale).astype(np.float32)
            lo, hi, margin = R.top_p_sets(s, np.ones(V, bool), p, 0.0)
            if margin < 1e-4 or len(np.unique(s)) != V:
                continue
            out = TopPLogitsWarper(top_p=float(np.float32(p)))(None, torch.from_numpy(s)[None].clone())[0].numpy()
            assert np.array_equal(np.isfinite(out), lo), (V, scale, p)
            checked += 1
    assert checked >= 12


def test_python_surfaces_refuse_bad_top_p_without_a_device():
    import torch
    from lwm_amd import ops
    from lwm_amd.vision_llama import VideoLLaMAForCausalLM
    for bad in (0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="top_p"):
            ops.sample_tokens(torch.zeros(1, 8), temperature=1.0, top_k=0, seed=0, top_p=bad)
        with pytest.raises(ValueError, match="top_p"):
            VideoLLaMAForCausalLM.generate(None, None, do_sample=True, top_p=bad)
        with pytest.raises(ValueError, match="top_p"):
            VideoLLaMAForCausalLM.generate_vision(None, None, [1.0], top_p=bad)
    assert ops._check_top_p(None, "x") == 0.0 and ops._check_top_p(1.0, "x") == 0.0 and ops._check_top_p(0.25, "x") == 0.25


def test_lwm_top_p_environment_variable(monkeypatch):
    import torch
    from lwm_amd.cli import _common
    assert _common.parse_top_p("") is None and _common.parse_top_p("0.9") == 0.9 and _common.parse_top_p("1") == 1.0
    model = types.SimpleNamespace(dtype=torch.bfloat16)
    for v in ("LWM_TOP_P", "LWM_PREFILL_CHUNK", "LWM_KV_CACHE", "LWM_DECODE_GRAPH"):
        monkeypatch.delenv(v, raising=False)
    gen = object()
    assert _common.sampler_kwargs(model, 7, gen) == dict(generator=gen)              # unset: the dict as it was
    monkeypatch.setenv("LWM_TOP_P", "")
    assert _common.sampler_kwargs(model, 7, gen) == dict(generator=gen)
    monkeypatch.setenv("LWM_TOP_P", "0.9")
    assert _common.sampler_kwargs(model, 7, gen) == dict(generator=gen, top_p=0.9)
    monkeypatch.setenv("LWM_DECODE_GRAPH", "1")
    monkeypatch.setenv("LWM_KV_CACHE", "fp8")
    assert _common.sampler_kwargs(model, 7, gen) == dict(seed=7, graph=True, kv_dtype="fp8", top_p=0.9)
    for bad in ("0", "1.5", "x", "-0.5", "nan"):
        monkeypatch.setenv("LWM_TOP_P", bad)
        with pytest.raises(SystemExit, match="LWM_TOP_P"):
            _common.sampler_kwargs(model, 7, gen)
