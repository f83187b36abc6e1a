"""Per-block activation recompute (lwm_amd/remat.py) without a GPU: the harness's own module code in float32 with the
operators stood in (tests/test_golden.py: _cpu_operator_stand_ins) and the attention op routed through the product's ring
driver over the oracle block kernels (tests/_standin.OracleBlockOps), as tests/test_golden.py's sequence-ring harness
arranges it.  RoPE is stood in by a differentiable one here, so that wq and wk get gradients to compare."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

B, S, V, D_MODEL, HEADS, LAYERS = 2, 64, 64, 32, 2, 2


def _rope(xq, xk, table, position_ids=None, dtype=None):
    """lwm/llama.py:353-375 in torch: the complex multiply on interleaved pairs, differentiable"""
    Bq, Sq = xq.shape[:2]
    pos = torch.arange(Sq)[None].expand(Bq, Sq) if position_ids is None else position_ids.long()
    fc = torch.view_as_complex(table.float().contiguous())[pos]

    def rot(t):
        tc = torch.view_as_complex(t.float().reshape(*t.shape[:-1], -1, 2))
        return torch.view_as_real(tc * fc[:, :, None, :]).reshape(t.shape)
    return rot(xq), rot(xk)


def _stand_ins(mp_, comm, counts=None):
    """-> the model; `comm`: the ring communicator every attention call uses.  counts["fwd"]: launches of the block forward."""
    from lwm_amd import llama as LM
    from lwm_amd import ringattention as RA
    from lwm_amd.ring import ring_attention
    from tests._standin import OracleBlockOps
    from tests.test_golden import _cpu_operator_stand_ins
    _cpu_operator_stand_ins(mp_)
    mp_.setattr(LM, "apply_rotary_emb", _rope)
    mp_.setattr(LM, "ringattention", RA.ringattention)
    mp_.setattr(RA, "ring_attention", lambda q, k, v, **kw: ring_attention(
        q, k, v, **{**kw, "block_ops": OracleBlockOps, "comm": comm}).float())
    if counts is not None:
        real = OracleBlockOps.fwd
        mp_.setattr(OracleBlockOps, "fwd", staticmethod(lambda *a, **kw: (counts.__setitem__("fwd", counts["fwd"] + 1), real(*a, **kw))[1]))
    torch.manual_seed(3)
    cfg = LM.LLaMAConfig(vocab_size=V, hidden_size=D_MODEL, intermediate_size=48, num_hidden_layers=LAYERS, num_attention_heads=HEADS,
                         max_sequence_length=128, scan_mlp=True, scan_mlp_chunk_size=16, initializer_range=0.2)
    return LM.LLaMAForCausalLM(cfg, torch.float32)


def _batch():
    g = torch.Generator().manual_seed(11)
    tokens = torch.randint(0, V, (B, S + 1), generator=g)
    am = torch.ones(B, S, dtype=torch.int32)
    am[:, 20:24] = 0                                                     # a hole
    seg = torch.bucketize(torch.arange(S), torch.tensor([17, 40]), right=True).to(torch.int32)[None].expand(B, S).contiguous()
    return tokens, am, seg


def _step(model, tokens, am, seg, shard=lambda t: t):
    """one forward + backward of this rank's rows -> (loss, {name: grad or None})"""
    model.zero_grad(set_to_none=True)
    h = model.hidden_states(shard(tokens[:, :-1]), am, seg)
    logits = h @ model.lm_head
    loss = torch.nn.functional.cross_entropy(logits.reshape(-1, V), shard(tokens[:, 1:]).reshape(-1), reduction="sum")
    loss.backward()
    return loss.detach().clone(), {n: (None if p.grad is None else p.grad.clone()) for n, p in model.named_parameters()}


def _same(on, off, off2, what=""):
    """`on` against the un-remat run `off`: torch.equal -- or, for a tensor the un-remat path itself does not reproduce
    (off vs off2), no further away than that path's own run-to-run difference"""
    (l_on, g_on), (l_off, g_off), (l_off2, g_off2) = on, off, off2
    bad = []
    for n, a, b, c in [("loss", l_on, l_off, l_off2)] + [(n, g_on[n], g_off[n], g_off2[n]) for n in g_off]:
        if b is None or a is None:
            if not (a is None and b is None):
                bad.append((n, "grad is None on one side only"))
        elif torch.equal(b, c):
            if not torch.equal(a, b):
                bad.append((n, float((a - b).abs().max())))
        elif float((a - b).abs().max()) > float((b - c).abs().max()):
            bad.append((n, float((a - b).abs().max()), "run-to-run", float((b - c).abs().max())))
    assert not bad, (what, bad)
    assert any(g is not None and bool(g.abs().sum() > 0) for n, g in g_on.items() if n.endswith("attention.wq")), "wq got no gradient"


def test_one_process_equals_the_unremat_path_and_runs_the_attention_forward_once(monkeypatch):
    from lwm_amd import remat
    from lwm_amd.ring import SingleComm
    counts = {"fwd": 0}
    model = _stand_ins(monkeypatch, SingleComm(), counts)
    made = []
    real_apply = remat.remat_block
    monkeypatch.setattr(remat, "remat_block", lambda *a, **kw: (made.append(1), real_apply(*a, **kw))[1])
    batch = _batch()
    off, off2 = _step(model, *batch), _step(model, *batch)
    assert not made
    counts["fwd"] = 0
    model.remat_blocks = True
    on = _step(model, *batch)
    assert len(made) == LAYERS                       # the switch took the new path ...
    assert counts["fwd"] == LAYERS, counts           # ... and the recompute did not run the attention forward again
    _same(on, off, off2)
    # a block whose input needs no gradient still owes its parameters theirs; a frozen parameter stays without one
    model.wte.requires_grad_(False)
    model.h[1].attention.wo.requires_grad_(False)
    model.remat_blocks = False
    off, off2 = _step(model, *batch), _step(model, *batch)
    model.remat_blocks = True
    on = _step(model, *batch)
    _same(on, off, off2, "frozen wte and h.1.attention.wo")
    assert on[1]["h.1.attention.wo"] is None and on[1]["wte"] is None and on[1]["h.0.attention.wq"] is not None
    # inert under no_grad
    made.clear()
    with torch.no_grad():
        model.hidden_states(batch[0][:, :-1], batch[1], batch[2])
    assert not made


def test_an_attention_call_with_nothing_to_replay_is_recomputed(monkeypatch):
    """LM.ringattention as a plain differentiable function: no Function records anything, the recompute runs it again"""
    from lwm_amd import llama as LM
    from lwm_amd.ring import SingleComm
    from lwm_amd.ringattention import key_valid_from_bias
    model = _stand_ins(monkeypatch, SingleComm())
    calls = []

    def plain(q, k, v, attn_bias, segment_ids, axis_name="sp", float32_logits=True, cache_idx=None, blockwise_kwargs=None, layout=None):
        calls.append(torch.is_grad_enabled())
        Sq = q.shape[1]
        vis = torch.ones(Sq, Sq, dtype=torch.bool).tril()[None].expand(q.shape[0], Sq, Sq)
        if segment_ids is not None:
            vis = vis & (segment_ids[:, :, None] == segment_ids[:, None, :])
        if attn_bias is not None:
            vis = vis & (key_valid_from_bias(attn_bias)[:, None, :] != 0)
        s = torch.einsum("bqhd,bkhd->bhqk", q, k) / q.shape[-1] ** 0.5
        p = torch.softmax(s.masked_fill(~vis[:, None], float("-inf")), -1)
        return torch.einsum("bhqk,bkhd->bqhd", p, v)
    monkeypatch.setattr(LM, "ringattention", plain)
    batch = _batch()
    off, off2 = _step(model, *batch), _step(model, *batch)
    calls.clear()
    model.remat_blocks = True
    on = _step(model, *batch)
    assert calls == [False, False, True, True], calls        # the no-grad forwards, then one recompute per layer, last first
    _same(on, off, off2)


def test_saved_bytes_against_hand_computed_values():
    from lwm_amd.remat import saved_bytes
    assert saved_bytes(1, 1, 4096, 32, torch.bfloat16) == 16512                 # 4 d + 4 H per token: 16.1 KB at LWM-7B
    assert saved_bytes(2, 2048, 512, 4, torch.bfloat16) == 2 * 2048 * (4 * 512 + 4 * 4) == 8454144
    assert saved_bytes(1, 8, 16, 2, torch.float32, n_lse=2) == 8 * (2 * 16 * 4 + 4 * 2 * 2) == 1152
    assert saved_bytes(1, 1, 4096, 32, torch.float32) == 2 * 16384 + 128


def test_the_environment_switch(monkeypatch):
    from lwm_amd import llama as LM
    monkeypatch.setattr(LM.LLaMAConfig, "_validate", lambda self: None)
    model = LM.LLaMAForCausalLM(LM.LLaMAConfig(vocab_size=8, hidden_size=8, intermediate_size=8, num_hidden_layers=1,
                                               num_attention_heads=2, max_sequence_length=8), torch.float32)
    monkeypatch.delenv("LWM_REMAT_BLOCK", raising=False)
    assert model.remat_blocks is False
    for text, want in (("1", True), ("0", False), ("", False)):
        monkeypatch.setenv("LWM_REMAT_BLOCK", text)
        assert model.remat_blocks is want
    monkeypatch.setenv("LWM_REMAT_BLOCK", "2")
    with pytest.raises(ValueError, match="LWM_REMAT_BLOCK"):
        model.remat_blocks
    model.remat_blocks = True                         # set on the model: the environment is not read
    assert model.remat_blocks is True
    model.remat_blocks = False
    assert model.remat_blocks is False
    with pytest.raises(ValueError, match="remat_blocks"):
        model.remat_blocks = "yes"
    model.remat_blocks = None
    monkeypatch.setenv("LWM_REMAT_BLOCK", "1")
    assert model.remat_blocks is True


def _ring_worker(rank, world, port, q_out):
    """one rank of a gloo sequence ring (zigzag ownership): the un-remat step twice, then the remat step"""
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from lwm_amd import ring as ring_mod
        from lwm_amd import ringattention as RA
        mp_ = pytest.MonkeyPatch()
        comm = ring_mod.TorchRingComm(None, schedule="mesh")
        sent = {"n": 0, "fwd": 0}
        for name in ("exchange_async", "rotate", "all_gather"):
            real = getattr(ring_mod.TorchRingComm, name)
            mp_.setattr(ring_mod.TorchRingComm, name,
                        (lambda real: lambda self, *a, **kw: (sent.__setitem__("n", sent["n"] + 1), real(self, *a, **kw))[1])(real))
        real_fwd = ring_mod.ring_forward
        mp_.setattr(ring_mod, "ring_forward", lambda *a, **kw: (sent.__setitem__("fwd", sent["fwd"] + 1), real_fwd(*a, **kw))[1])
        model = _stand_ins(mp_, comm)
        RA.set_sp_group(dist.group.WORLD)
        shard = lambda t: RA.sp_shard(t, dim=1)
        batch = _batch()
        runs, exchanges = [], []
        for on in (False, False, True):
            model.remat_blocks = on
            sent["n"] = sent["fwd"] = 0
            runs.append(_step(model, *batch, shard=shard))
            exchanges.append((sent["n"], sent["fwd"]))
        err = None
        try:
            _same(runs[2], runs[0], runs[1], f"rank {rank}")
        except AssertionError as e:
            err = str(e)
        q_out.put((rank, RA.sp_layout("sp", S // world), err, exchanges))
        dist.barrier()
        mp_.undo()
    finally:
        dist.destroy_process_group()


def test_a_gloo_ring_of_two_equals_the_unremat_path_and_replays_without_an_exchange():
    import torch.multiprocessing as mp
    from tests.test_ring_gloo import _free_port
    world = 2
    ctx = mp.get_context("spawn")
    qout, port = ctx.Queue(), _free_port()
    procs = [ctx.Process(target=_ring_worker, args=(r, world, port, qout)) for r in range(world)]
    for p in procs:
        p.start()
    res = [qout.get(timeout=240) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, layout, err, exchanges in res:
        assert layout == "zigzag"
        assert err is None, err
        # (exchange calls of a whole step, ring_forward calls): the remat step posts what the un-remat step posts -- the
        # replayed forward sends nothing -- and runs the ring forward once per layer
        assert exchanges[0][0] > 0 and exchanges[2] == exchanges[0] == exchanges[1], (rank, exchanges)
        assert exchanges[2][1] == LAYERS
