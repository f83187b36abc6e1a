"""Per-block activation recompute (lwm_amd/remat.py, LLaMAForCausalLM.remat_blocks) on the GPU: the same loss and the same
gradients as the un-remat path, bit for bit (the forward runs the same kernels on the same inputs, the backward the same
kernels on a recomputed graph); the attention forward once per layer and step; the MLP twice per chunk, not three times;
and the memory a step holds per layer: remat.saved_bytes, derived from the formula, not measured.

retain_graph: a remat block's kept tensors are autograd's saved tensors, so backward(retain_graph=True) followed by a
second backward() WORKS -- the block is recomputed again, with the same results -- and a second backward() without it is
autograd's own "backward through the graph a second time" RuntimeError."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg(layers=2, video=False, **kw):
    from lwm_amd.llama import LLaMAConfig
    from lwm_amd.vision_llama import VideoLLaMAConfig
    return (VideoLLaMAConfig if video else LLaMAConfig)(vocab_size=4096, hidden_size=512, intermediate_size=1408, num_hidden_layers=layers,
                                                        num_attention_heads=4, max_sequence_length=2048, **kw)


def _model(cfg, dtype=None, seed=3):
    import torch
    from lwm_amd.llama import LLaMAForCausalLM
    from lwm_amd.vision_llama import VideoLLaMAConfig, VideoLLaMAForCausalLM
    torch.manual_seed(seed)
    cls = VideoLLaMAForCausalLM if isinstance(cfg, VideoLLaMAConfig) else LLaMAForCausalLM
    return cls(cfg, dtype or torch.bfloat16).cuda()


def _tokens(B, S, vocab=4096, seed=5):
    import torch
    return torch.randint(0, vocab, (B, S + 1), generator=torch.Generator().manual_seed(seed)).cuda()


def _grads(model):
    return {n: (None if p.grad is None else p.grad.clone()) for n, p in model.named_parameters()}


def _step(model, loss_fn, zero=True):
    if zero:
        model.zero_grad(set_to_none=True)
    loss = loss_fn()
    loss.backward()
    return loss.detach().clone(), _grads(model)


def _same(on, off, off2, what=""):
    """remat against the un-remat step: torch.equal.  The precondition -- the un-remat step run twice gives torch.equal
    results -- is checked first, per tensor; a tensor that fails it is held to twice that path's own run-to-run difference
    and printed."""
    import torch
    (l_on, g_on), (l_off, g_off), (l_off2, g_off2) = on, off, off2
    bad = []
    for n, a, b, c in [("loss", l_on, l_off, l_off2)] + [(n, g_on[n], g_off[n], g_off2[n]) for n in g_off]:
        if a is None or b is None:
            if not (a is None and b is None):
                bad.append((n, "a gradient on one side only"))
        elif torch.equal(b, c):
            if not torch.equal(a, b):
                bad.append((n, float((a.float() - b.float()).abs().max())))
        else:
            rr, d = float((b.float() - c.float()).abs().max()), float((a.float() - b.float()).abs().max())
            print(f"remat {what}: the un-remat step does not reproduce {n}: run-to-run {rr!r}, remat - un-remat {d!r}")
            if d > 2 * rr:
                bad.append((n, d, "run-to-run", rr))
    assert not bad, (what, bad)


def _three(model, loss_fn, what=""):
    model.remat_blocks = False
    off, off2 = _step(model, loss_fn), _step(model, loss_fn)
    model.remat_blocks = True
    on = _step(model, loss_fn)
    model.remat_blocks = False
    _same(on, off, off2, what)
    return on, off


def _spy(monkeypatch, obj, name, counts, static=True):
    real = getattr(obj, name)
    counts[name] = 0

    def wrapped(*a, **kw):
        counts[name] += 1
        return real(*a, **kw)
    monkeypatch.setattr(obj, name, staticmethod(wrapped) if static else wrapped)


@pytest.mark.parametrize("case", ["packed_1536", "b2_1024_plain_mlp", "s1000", "float32_512", "video"])
def test_remat_equals_the_unremat_step(case, monkeypatch):
    import torch
    from lwm_amd import remat
    made = {}
    _spy(monkeypatch, remat, "remat_block", made, static=False)
    if case == "packed_1536":        # three segments and a hole in the key mask: the 9-unit backward; chunked MLP
        S = 1536
        model, tok = _model(_cfg(scan_mlp_chunk_size=256)), _tokens(1, S)
        seg = torch.zeros(1, S, dtype=torch.int32, device="cuda")
        seg[:, S // 3:] = 1
        seg[:, (3 * S) // 4:] = 2
        am = torch.ones(1, S, dtype=torch.int32, device="cuda")
        am[:, 5:9] = 0
        fn = lambda: model.loss(tok[:, :-1], tok[:, 1:], None, am, seg, chunk=1024)[0]
    elif case == "b2_1024_plain_mlp":        # no masks: the dS hand-over backward
        model, tok = _model(_cfg(scan_mlp=False)), _tokens(2, 1024)
        fn = lambda: model.loss(tok[:, :-1], tok[:, 1:], chunk=512)[0]
    elif case == "s1000":
        model, tok = _model(_cfg()), _tokens(1, 1000)
        fn = lambda: model.loss(tok[:, :-1], tok[:, 1:], chunk=512)[0]
    elif case == "float32_512":        # the plain branch of LLaMABlock.forward
        model, tok = _model(_cfg(scan_mlp_chunk_size=256), torch.float32), _tokens(1, 512)
        fn = lambda: model.loss(tok[:, :-1], tok[:, 1:], chunk=512)[0]
    else:        # two embedding tables, two heads, a vision span mid-sequence
        S = 1024
        model, tok = _model(_cfg(video=True, vision_vocab_size=1024, scan_mlp_chunk_size=512)), _tokens(1, S)
        vm = torch.zeros(1, S + 1, dtype=torch.bool, device="cuda")
        vm[:, S // 4: S // 4 + S // 2] = True
        tok = torch.where(vm, tok % 1024, tok)
        fn = lambda: model.loss(tok[:, :-1], vm[:, :-1], tok[:, 1:], vm[:, 1:], chunk=512)[0]
    _three(model, fn, case)
    assert made["remat_block"] == 2          # the remat step took the new path, once per block


def test_launch_counts(monkeypatch):
    """remat on: the attention forward once per layer and step, each backward entry point once per layer, the MLP twice per
    chunk and layer (the no-grad forward and the recompute) -- its own chunk checkpoint does not add a third"""
    from lwm_amd import ring as ring_mod
    from lwm_amd.llama_ops import LLaMAMLP
    S, chunk, layers = 1024, 256, 2
    model, tok = _model(_cfg(scan_mlp_chunk_size=chunk)), _tokens(1, S)
    fn = lambda: model.loss(tok[:, :-1], tok[:, 1:], chunk=512)[0]
    _step(model, fn)
    counts = {}
    for name in ("fwd", "bwd_delta", "bwd_dq", "bwd_dkdv"):
        _spy(monkeypatch, ring_mod.HipBlockOps, name, counts)
    _spy(monkeypatch, LLaMAMLP, "forward", counts, static=False)
    model.remat_blocks = True
    _step(model, fn)
    assert counts == {"fwd": layers, "bwd_delta": layers, "bwd_dq": layers, "bwd_dkdv": layers, "forward": 2 * (S // chunk) * layers}, counts


def test_a_block_whose_input_needs_no_gradient_still_gives_its_parameters_theirs():
    model, tok = _model(_cfg(scan_mlp_chunk_size=512)), _tokens(1, 1024)
    fn = lambda: model.loss(tok[:, :-1], tok[:, 1:], chunk=512)[0]
    model.wte.requires_grad_(False)
    on, off = _three(model, fn, "frozen wte")
    blocks = [n for n in on[1] if n.startswith("h.")]
    assert len(blocks) == 2 * 9 and all(on[1][n] is not None for n in blocks) and on[1]["wte"] is None
    model.h[1].attention.wo.requires_grad_(False)
    on, off = _three(model, fn, "frozen wte and h.1.attention.wo")
    assert on[1]["h.1.attention.wo"] is None and all(on[1][n] is not None for n in blocks if n != "h.1.attention.wo")


def test_two_micro_batches_accumulate_as_without_remat():
    import torch
    model = _model(_cfg(scan_mlp_chunk_size=512))
    toks = [_tokens(1, 1024, seed=s) for s in (5, 6)]

    def run():
        model.zero_grad(set_to_none=True)
        losses = []
        for t in toks:
            losses.append(_step(model, lambda: model.loss(t[:, :-1], t[:, 1:], chunk=512)[0] / 2, zero=False)[0])
        return torch.stack(losses), _grads(model)
    model.remat_blocks = False
    off, off2 = run(), run()
    model.remat_blocks = True
    on = run()
    _same(on, off, off2, "two micro-batches")


def test_retain_graph_and_a_second_backward():
    import torch
    model, tok = _model(_cfg(scan_mlp_chunk_size=512)), _tokens(1, 1024)
    fn = lambda: model.loss(tok[:, :-1], tok[:, 1:], chunk=512)[0]
    off, off2 = _step(model, fn), _step(model, fn)
    model.remat_blocks = True
    model.zero_grad(set_to_none=True)
    loss = fn()
    loss.backward(retain_graph=True)
    first = (loss.detach().clone(), _grads(model))
    model.zero_grad(set_to_none=True)
    loss.backward()
    second = (loss.detach().clone(), _grads(model))
    _same(first, off, off2, "first backward")
    _same(second, off, off2, "second backward")
    with pytest.raises(RuntimeError, match="second time"):
        loss.backward()


def _held_and_peak(layers, on):
    import torch
    model, tok = _model(_cfg(layers)), _tokens(2, 2048)
    model.remat_blocks = on
    fn = lambda: model.loss(tok[:, :-1], tok[:, 1:], chunk=1024)[0]
    fn().backward()
    model.zero_grad(set_to_none=False)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    loss = fn()
    held = torch.cuda.memory_allocated() - base
    loss.backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del loss, model
    torch.cuda.empty_cache()
    return held, peak


def test_memory_held_per_layer_is_the_kept_set():
    """L = 2 and L = 6, B = 2, S = 2048: what a further layer adds to the memory held after the forward, and to the peak of the
    step, is remat.saved_bytes -- x, the attention out, one lse -- within 1.25 (allocator rounding; the smallest tensor that
    could be kept by accident, one (B,S,d) bf16 tensor, is 0.5 of it); without remat a layer holds at least x, q|k|v, out,
    x2 and h2: 7 d against 2 d per token, asserted as >= 3."""
    import torch
    from lwm_amd import remat
    per = remat.saved_bytes(2, 2048, 512, 4, torch.bfloat16)
    h2, p2 = _held_and_peak(2, True)
    h6, p6 = _held_and_peak(6, True)
    o2, _ = _held_and_peak(2, False)
    o6, _ = _held_and_peak(6, False)
    print(f"remat memory: per layer kept {per}; held (6-2)/4 on {(h6 - h2) / 4} off {(o6 - o2) / 4}; peak (6-2)/4 on {(p6 - p2) / 4}")
    assert (h6 - h2) / 4 <= 1.25 * per, ((h6 - h2) / 4, per)
    assert (p6 - p2) / 4 <= 1.25 * per, ((p6 - p2) / 4, per)
    assert (o6 - o2) / 4 >= 3 * per, ((o6 - o2) / 4, per)


def test_inert_in_inference_and_under_no_grad(monkeypatch):
    import torch
    from lwm_amd import remat
    model, tok = _model(_cfg()), _tokens(2, 48)
    made = {}
    _spy(monkeypatch, remat, "remat_block", made, static=False)
    out_off = model.generate(tok[:, :48], max_new_tokens=4, return_logits=True)
    model.remat_blocks = True
    out_on = model.generate(tok[:, :48], max_new_tokens=4, return_logits=True)
    assert torch.equal(out_on[0], out_off[0]) and torch.equal(out_on[1], out_off[1])
    with torch.no_grad():
        model.hidden_states(tok[:, :-1])
    assert made["remat_block"] == 0
    model.hidden_states(tok[:, :-1])           # ... and with autograd recording, the same call is recomputed
    assert made["remat_block"] == 2


def _cli(dump, extra=(), S=1024):
    argv = [sys.executable, "-m", "lwm_amd.cli.train", "--mesh_dim=1,1,1,1", "--dtype=bf16", "--total_steps=1", "--log_freq=1",
            "--load_llama_config=debug", "--seed=11", f"--update_llama_config=dict(vocab_size=512,max_sequence_length={S},theta=1000000)",
            "--train_dataset.type=json", f"--train_dataset.json_dataset.seq_length={S}", "--train_dataset.json_dataset.batch_size=1",
            "--optimizer.adamw_optimizer.lr=1e-4", f"--lwm_dump_grads={dump}", *extra]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "LWM_REMAT_BLOCK")}
    r = subprocess.run(argv, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    return r.stdout + r.stderr


def _dumps_equal(a, b):
    import torch
    assert torch.equal(a["tokens"], b["tokens"]) and a["loss"] == b["loss"], (a["loss"], b["loss"])
    assert set(a["grads"]) == set(b["grads"]) == set(a["params"]) and len(a["grads"]) >= 20
    bad = [n for n in a["grads"] if not torch.equal(a["grads"][n], b["grads"][n])]
    assert not bad, bad


def test_train_cli_with_the_flag_equals_the_run_without(tmp_path):
    import torch
    off_f, on_f = str(tmp_path / "off.pt"), str(tmp_path / "on.pt")
    out_off = _cli(off_f)
    out_on = _cli(on_f, ("--lwm_remat_block",))
    assert "activation recompute" in out_on and "activation recompute" not in out_off
    _dumps_equal(torch.load(on_f), torch.load(off_f))


def test_train_cli_c_ring_driver_replays_under_the_flag(tmp_path):
    """2 ranks on one GPU, the C ring driver over the library's IPC transport (tests/test_gpu_cli_ring.py's arrangement and
    its sequence length): _RingAttentionC under replay -- no forward exchange in the recompute, K/V fetched again by the
    backward -- gives the gradients of the run without the flag"""
    import torch
    from tests.test_gpu_cli_ring import _run
    off_f, on_f = str(tmp_path / "off.pt"), str(tmp_path / "on.pt")
    env = {"LWM_RING_DRIVER": "c"}
    outs_off = _run(2, off_f, env_extra=env, timeout=300)
    outs_on = _run(2, on_f, env_extra=env, extra=("--lwm_remat_block",), timeout=300)
    for outs in (outs_off, outs_on):
        assert "'driver': 'c'" in outs[0] and "'transport': 'ipc'" in outs[0], outs[0][-1500:]
    assert "activation recompute" in outs_on[0]
    _dumps_equal(torch.load(on_f), torch.load(off_f))
