"""Residual and embedding dropout on the MI355X (csrc/dropout.h, llama_ops.dropout_add, the sites of lwm_amd/llama.py): the
device kernels against the numpy restatement of tests/_dropout_ref.py bit for bit; the operator's backward; a block with
dropout on against the composition of its own submodules under masks uploaded from the restatement; and a model's
training step -- the same (seed, step) twice gives the same bits, remat and the chunked MLP regenerate the masks of the
forward, and with the rates at 0, in eval() and under a KV cache not one dropout launch happens."""
import functools

import numpy as np
import pytest

from tests import _dropout_ref as R

pytestmark = pytest.mark.gpu
RULE = dict(key0=0x5EED0001, key1=17, site=3)
THR, INV = R.thr_inv(0.1)
# the shapes of tests/test_emu_dropout.py (33 and 257 vectors a row: the division and the compare path); the last one has more 8-channel vectors than one pass of the device's grid
# (8 blocks x 256 compute units x 256), the last tile cut
SHAPES = [(1, 1, 8), (2, 3, 8), (2, 5, 264), (2, 3, 2056), (2, 1031, 2056)]


def _dev(a):
    import torch
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16).copy()).view(torch.bfloat16).cuda()
    return torch.from_numpy(a.copy()).cuda()


def _host(t):
    import torch
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    return t.cpu().numpy()


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


@functools.lru_cache(maxsize=None)
def _case(shape, f32):
    """inputs and the restatement's results for one shape and dtype, computed once and left alone"""
    rng = np.random.default_rng(shape[1] * 7 + shape[2])
    x, r = (rng.standard_normal(shape).astype(np.float32) for _ in range(2))
    if not f32:
        x, r = R.to_bf16_bits(x), R.to_bf16_bits(r)
    fn = R.dropout_add_f32 if f32 else R.dropout_add_bf16
    kw = dict(thr16=THR, inv=INV, **RULE)
    return x, r, fn(x, r, **kw), fn(x, None, **kw)


def _launch(kind, x, res, *, y=None, thr16=THR, inv=float(INV), s_offset=0, key0, key1, site):
    import torch
    from lwm_amd import dropout as O
    y = torch.full_like(x, float("nan")) if y is None else y
    O._dropout_launch(kind, x, res, y, (thr16, inv, key0, key1, site, s_offset))
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "f32"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_kernel_bits(shape, f32):
    import torch
    if shape == SHAPES[-1]:
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        assert shape[0] * shape[1] * shape[2] // 8 > 8 * cus * 256, "the shape no longer exceeds one pass of the grid"
    x, r, y_ref, d_ref = _case(shape, f32)
    xd, rd = _dev(x), _dev(r)
    assert np.array_equal(_bits(_host(_launch("add", xd, rd, **RULE))), _bits(y_ref))
    assert np.array_equal(_bits(_host(_launch("add", xd, None, **RULE))), _bits(d_ref))
    assert np.array_equal(_bits(_host(_launch("bwd", xd, None, **RULE))), _bits(d_ref))
    # y may alias x or res
    xa = xd.clone()
    assert np.array_equal(_bits(_host(_launch("add", xa, rd, y=xa, **RULE))), _bits(y_ref))
    ra = rd.clone()
    assert np.array_equal(_bits(_host(_launch("add", xd, ra, y=ra, **RULE))), _bits(y_ref))


@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "f32"])
def test_kernel_edges(f32):
    """thr16 = 0 is the plain rounded sum; thr16 = 65535; -0 and subnormal operands; a chunk of rows at its offset"""
    shape = (2, 37, 264)
    n = int(np.prod(shape))
    tiny = np.float32(2.0 ** -133)
    vals = np.array([-0.0, 0.0, tiny, -tiny, 2.0 ** -126, 1.0, -3.5, 0.3, 2.0 ** -149 if f32 else tiny * 3], np.float32)
    rng = np.random.default_rng(3)
    x, r = (vals[rng.integers(0, len(vals), n)].reshape(shape) for _ in range(2))
    fn = R.dropout_add_f32
    if not f32:
        x, r, fn = R.to_bf16_bits(x), R.to_bf16_bits(r), R.dropout_add_bf16
    xd, rd = _dev(x), _dev(r)
    whole = _host(_launch("add", xd, rd, **RULE))
    assert np.array_equal(_bits(whole), _bits(fn(x, r, thr16=THR, inv=INV, **RULE)))
    assert np.array_equal(_bits(_host(_launch("add", xd, None, **RULE))), _bits(fn(x, None, thr16=THR, inv=INV, **RULE)))
    y0 = _launch("add", xd, rd, thr16=0, inv=1.0, **RULE)
    plain = (x + r).astype(np.float32) if f32 else R.to_bf16_bits(R.from_bf16_bits(x) + R.from_bf16_bits(r))
    assert np.array_equal(_bits(_host(y0)), _bits(plain)) and np.array_equal(_bits(plain), _bits(fn(x, r, thr16=0, inv=np.float32(1), **RULE)))
    t, inv = R.thr_inv(65535 / 65536)
    assert np.array_equal(_bits(_host(_launch("add", xd, rd, thr16=t, inv=float(inv), **RULE))), _bits(fn(x, r, thr16=t, inv=inv, **RULE)))
    for s0, s1 in ((0, 13), (13, 30), (30, 37)):
        part = _launch("add", xd[:, s0:s1].contiguous(), rd[:, s0:s1].contiguous(), s_offset=s0, **RULE)
        assert np.array_equal(_bits(_host(part)), _bits(np.ascontiguousarray(whole[:, s0:s1]))), (s0, s1)


@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "f32"])
def test_operator(f32):
    import torch
    from lwm_amd.llama_ops import dropout_add
    shape = (2, 5, 264)
    x, r, y_ref, _ = _case(shape, f32)
    rng = np.random.default_rng(1)
    g = rng.standard_normal(shape).astype(np.float32)
    g = g if f32 else R.to_bf16_bits(g)
    xd, rd, gd = _dev(x).requires_grad_(True), _dev(r).requires_grad_(True), _dev(g)
    y = dropout_add(xd, rd, 0.1, (RULE["key0"], RULE["key1"]), RULE["site"])
    assert np.array_equal(_bits(_host(y.detach())), _bits(y_ref))
    assert y.grad_fn.saved_tensors == ()                    # nothing is saved for the backward: only the scalars
    y.backward(gd)
    dx_ref = (R.dropout_add_f32 if f32 else R.dropout_add_bf16)(g, None, thr16=THR, inv=INV, **RULE)
    assert np.array_equal(_bits(_host(xd.grad)), _bits(dx_ref))
    assert torch.equal(rd.grad, gd)                         # the residual's gradient is g
    # residual None, a chunk at its offset
    y2 = dropout_add(xd.detach()[:, 2:4].contiguous(), None, 0.1, (RULE["key0"], RULE["key1"]), RULE["site"], s_offset=2)
    whole = (R.dropout_add_f32 if f32 else R.dropout_add_bf16)(x, None, thr16=THR, inv=INV, **RULE)
    assert np.array_equal(_bits(_host(y2)), _bits(np.ascontiguousarray(whole[:, 2:4])))


def test_operator_refusals():
    import torch
    from lwm_amd.llama_ops import dropout_add, dropout_threshold
    x = torch.zeros(2, 4, 16, dtype=torch.bfloat16, device="cuda")
    ok = dict(p=0.1, rng=(1, 2), site=0)
    for bad in ((-1, 0), (0, -1), (2 ** 32, 0), (0, 2 ** 32), (1.5, 0), (True, 0), (1,), 7):
        with pytest.raises(ValueError):
            dropout_add(x, None, 0.1, bad, 0)
    for kw in (dict(site=-1), dict(site=2 ** 32), dict(s_offset=-1), dict(s_offset=2 ** 32 - 3), dict(p=1.0), dict(p=-0.1),
               dict(p=0.999999)):
        with pytest.raises(ValueError):
            dropout_add(x, None, **{**ok, **kw})
    for t in (x.cpu(), x.half(), x[:, :, :8], x.transpose(0, 1), x[0], torch.zeros(2, 4, 12, dtype=torch.bfloat16, device="cuda")):
        with pytest.raises(ValueError):
            dropout_add(t, None, **ok)
    for r in (x.float(), x[:1], x.cpu()):
        with pytest.raises(ValueError):
            dropout_add(x, r, **ok)
    assert dropout_threshold(0.1) == (6554, float(np.float32(1.0 / (1.0 - 6554 / 65536.0)))) and dropout_threshold(0.0) == (0, 1.0)
    assert dropout_add(x, None, 0.0, (2 ** 32 - 1, 2 ** 32 - 1), 2 ** 32 - 1).shape == x.shape


# ---------------------------------------------------------------- block level
def _keep(shape, site, rng, dev, p=0.1):
    import torch
    return torch.from_numpy(R.keep_mask(*shape, thr16=R.thr_inv(p)[0], key0=rng[0], key1=rng[1], site=site)).to(dev)


@pytest.mark.parametrize("chunked", [False, True], ids=["plain_mlp", "chunked_mlp"])
@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "f32"])
def test_block_equals_the_composition_of_its_submodules(f32, chunked):
    """hidden 256, 2 heads, S = 192: the block with dropout on == norm, attention, mask * inv, add, norm, MLP, mask * inv, add
    done one by one with the restatement's masks -- the same f32 product, f32 add and one rounding (bf16), so torch.equal;
    in the chunked MLP (chunks of 64 rows) the dropout is rounded inside the chunk and the add is the block's own."""
    import torch
    from lwm_amd.llama import LLaMABlock, LLaMAConfig
    from lwm_amd.llama_ops import precompute_freqs_cis
    dtype = torch.float32 if f32 else torch.bfloat16
    cfg = LLaMAConfig(vocab_size=512, hidden_size=256, intermediate_size=512, num_hidden_layers=1, num_attention_heads=2,
                      max_sequence_length=512, resid_pdrop=0.1, scan_mlp=chunked, scan_mlp_chunk_size=64)
    torch.manual_seed(2)
    blk = LLaMABlock(cfg, dtype).cuda().train()
    blk.layer_index, rng = 3, (7, 11)
    B, S, d = 2, 192, 256
    x = torch.randn(B, S, d, generator=torch.Generator().manual_seed(4)).to(dtype).cuda()
    fc = precompute_freqs_cis(128, 512, device=x.device)
    with pytest.raises(ValueError, match="set_dropout_rng"):
        blk(x, fc)
    blk.set_dropout_rng(*rng)
    with torch.no_grad():
        y = blk(x, fc)
        inv = float(INV)
        zero = torch.zeros((), dtype=torch.float32, device=x.device)
        a = blk.attention(blk.attention_norm(x), fc)
        x1 = (x.float() + torch.where(_keep((B, S, d), 7, rng, x.device), a.float() * inv, zero)).to(dtype)
        f = blk.feed_forward(blk.ffn_norm(x1))
        dm = torch.where(_keep((B, S, d), 8, rng, x.device), f.float() * inv, zero)
        ref = x1 + dm.to(dtype) if chunked else (x1.float() + dm).to(dtype)
    assert not torch.equal(x1, x + a)                       # (something was dropped)
    assert torch.equal(y, ref), float((y.float() - ref.float()).abs().max())
    # the graph-recording forward (the chunk checkpoint on) gives the same bits, and eval() none of this
    assert torch.equal(blk(x.clone().requires_grad_(True), fc).detach(), y)
    blk.eval()
    cfg0 = LLaMAConfig(**{**cfg.to_dict(), "resid_pdrop": 0.0})
    blk0 = LLaMABlock(cfg0, dtype).cuda().train()
    blk0.load_state_dict(blk.state_dict())
    with torch.no_grad():
        assert torch.equal(blk(x, fc), blk0(x, fc))


# ---------------------------------------------------------------- model level
def _cfg(video=False, **kw):
    from lwm_amd.llama import LLaMAConfig
    from lwm_amd.vision_llama import VideoLLaMAConfig
    base = dict(vocab_size=512, hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2,
                max_sequence_length=512, resid_pdrop=0.1, embd_pdrop=0.1, scan_mlp=False)
    return (VideoLLaMAConfig if video else LLaMAConfig)(**{**base, **kw})


def _model(cfg, dtype, seed=3):
    import torch
    from lwm_amd.llama import LLaMAForCausalLM
    from lwm_amd.vision_llama import VideoLLaMAConfig, VideoLLaMAForCausalLM
    torch.manual_seed(seed)
    return (VideoLLaMAForCausalLM if isinstance(cfg, VideoLLaMAConfig) else LLaMAForCausalLM)(cfg, dtype).cuda()


def _tokens(B=2, S=256, vocab=512, seed=5):
    import torch
    return torch.randint(0, vocab, (B, S + 1), generator=torch.Generator().manual_seed(seed)).cuda()


def _step(model, tok, rng=None):
    if rng is not None:
        model.set_dropout_rng(*rng)
    model.zero_grad(set_to_none=True)
    loss = model.loss(tok[:, :-1], tok[:, 1:])[0]
    loss.backward()
    return loss.detach().clone(), {n: p.grad.clone() for n, p in model.named_parameters()}


def _equal(a, b):
    import torch
    return torch.equal(a[0], b[0]) and a[1].keys() == b[1].keys() and all(torch.equal(a[1][n], b[1][n]) for n in a[1])


def _count_launches(monkeypatch):
    from lwm_amd import dropout as O
    real, calls = O._dropout_launch, []
    monkeypatch.setattr(O, "_dropout_launch", lambda kind, *a: (calls.append(kind), real(kind, *a))[1])
    return calls


@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "f32"])
def test_model_step_is_a_function_of_seed_and_step(f32, monkeypatch):
    import torch
    dtype = torch.float32 if f32 else torch.bfloat16
    model, tok = _model(_cfg(), dtype).train(), _tokens()
    with pytest.raises(ValueError, match="set_dropout_rng"):
        model.loss(tok[:, :-1], tok[:, 1:])
    calls = _count_launches(monkeypatch)
    a, b = _step(model, tok, (11, 0)), _step(model, tok, (11, 0))
    # per step: the embedding and two sites per layer, forward and backward
    assert calls.count("add") == 2 * 5 and calls.count("bwd") == 2 * 5
    assert _equal(a, b) and all(torch.isfinite(g).all() for g in a[1].values())
    assert not torch.equal(_step(model, tok, (11, 1))[0], a[0])             # another step
    assert not torch.equal(_step(model, tok, (12, 0))[0], a[0])             # another seed
    # rates 0: the model of before, and not one dropout launch -- in training mode, with no pair ever set
    model0 = _model(_cfg(resid_pdrop=0.0, embd_pdrop=0.0), dtype).train()
    del calls[:]
    z, z2 = _step(model0, tok), _step(model0, tok)
    assert calls == [] and _equal(z, z2)
    assert not torch.equal(z[0], a[0])                                      # dropout changes the loss
    # eval() of the model with rates > 0 IS the rates-0 model
    model.eval()
    e = _step(model, tok)
    model.train()
    assert calls == [] and _equal(e, z)


@pytest.mark.parametrize("scan_mlp", [False, True], ids=["plain_mlp", "chunked_mlp_64"])
@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "f32"])
def test_remat_regenerates_the_masks(f32, scan_mlp):
    """remat on and off: the same loss and gradients bit for bit -- the recompute sees the same (key, site, b, s, c)"""
    import torch
    dtype = torch.float32 if f32 else torch.bfloat16
    model = _model(_cfg(scan_mlp=scan_mlp, scan_mlp_chunk_size=64), dtype).train()
    tok = _tokens()
    model.remat_blocks = False
    off, off2 = _step(model, tok, (11, 3)), _step(model, tok, (11, 3))
    model.remat_blocks = True
    on = _step(model, tok, (11, 3))
    assert _equal(off, off2) and _equal(on, off)
    if scan_mlp:        # the chunked MLP drops what the unchunked one drops: the masks are equal, the roundings are not
        plain = _model(_cfg(scan_mlp=False), dtype).train()
        plain.load_state_dict(model.state_dict())
        p = _step(plain, tok, (11, 3))
        assert abs(float(p[0]) - float(off[0])) < 1e-2 * abs(float(off[0]))


def test_vision_embedding_site_keeps_what_the_restatement_keeps():
    import torch
    model = _model(_cfg(video=True, embd_pdrop=0.5, resid_pdrop=0.0, vision_vocab_size=256), torch.bfloat16).train()
    B, S = 2, 64
    ids = _tokens(B, S - 1, vocab=256)
    vm = torch.zeros(B, S, dtype=torch.bool, device="cuda")
    vm[:, 16:40] = True
    model.set_dropout_rng(5, 9)
    emb = model._embed(ids, vm)
    assert bool((emb != 0).all())
    y = model._embd_dropout(emb, None)
    assert torch.equal(y != 0, _keep((B, S, 256), 0, (5, 9), "cuda", p=0.5))
    assert model._embd_dropout(emb, {"cache": 1}) is emb              # under a KV cache: inert
    # the same through hidden_states: the first block sees the dropped embedding
    seen = []
    h = model.h[0].register_forward_pre_hook(lambda m, args: seen.append(args[0].detach().clone()))
    with torch.no_grad():
        model.hidden_states(ids, vm)
    h.remove()
    assert torch.equal(seen[0], y)


def test_what_is_refused_and_what_is_inert(monkeypatch):
    import torch
    from lwm_amd import llama as M
    tok = _tokens()
    # attn_pdrop > 0 in a training forward
    model = _model(_cfg(attn_pdrop=0.1), torch.bfloat16).train()
    model.set_dropout_rng(1, 2)
    with pytest.raises(NotImplementedError, match="attn_pdrop"):
        model.loss(tok[:, :-1], tok[:, 1:])
    model.eval()
    assert torch.isfinite(model.loss(tok[:, :-1], tok[:, 1:])[0])
    # set_dropout_rng takes two integers in [0, 2^32)
    model = _model(_cfg(), torch.bfloat16).train()
    for bad in ((-1, 0), (0, 2 ** 32), (0.5, 0)):
        with pytest.raises(ValueError):
            model.set_dropout_rng(*bad)
    # a cached generate on a training-mode model with rates > 0 and NO pair set: no dropout launch, no complaint
    calls = _count_launches(monkeypatch)
    out = model.generate(tok[:1, :16], max_new_tokens=4)
    assert out.shape[1] >= 4 and calls == []
    # a sequence ring: the global row of a local row is not wired up
    model.set_dropout_rng(1, 2)
    monkeypatch.setattr(M, "sp_size_rank", lambda axis: (2, 0))
    x = torch.zeros(2, 64, 256, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(NotImplementedError, match="sp > 1"):
        model._embd_dropout(x, None)
    with pytest.raises(NotImplementedError, match="sp > 1"):
        model.h[1](x, model._table(x.device))
    assert calls == []


# ---------------------------------------------------------------- CLI
def test_cli_trains_with_dropout():
    """three steps of the debug config: finite losses, one seed gives the same losses run after run (also with
    --lwm_remat_block, whose first loss and gradients are the un-remat ones), and dropout moves the first loss"""
    from lwm_amd.cli import train

    def run(rates, *extra):
        hist = train.main(["--load_llama_config=debug", "--mesh_dim=1,-1,1,1", "--dtype=bf16", "--tokenizer=synthetic", "--modality=text",
                           "--total_steps=3", "--log_freq=0", "--seed=11",
                           f"--update_llama_config=dict(vocab_size=512,max_sequence_length=512,{rates})",
                           "--train_dataset.json_dataset.seq_length=256", "--train_dataset.json_dataset.batch_size=2",
                           "--optimizer.accumulate_gradient_steps=2", "--optimizer.adamw_optimizer.lr=1e-3",
                           "--optimizer.adamw_optimizer.lr_warmup_steps=1", *extra])
        return [h["loss"] for h in hist]

    on = "resid_pdrop=0.1,embd_pdrop=0.1"
    a, b = run(on), run(on)
    assert len(a) == 3 and all(np.isfinite(a)) and a == b
    assert run("resid_pdrop=0.0,embd_pdrop=0.0")[0] != a[0]
    r = run(on, "--lwm_remat_block", "--lwm_fused_optimizer")
    assert all(np.isfinite(r)) and r[0] == a[0]
