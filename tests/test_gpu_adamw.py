"""The fused AdamW on the device: the kernels through the C ABI against the numpy restatement (tests/_adamw_ref.py, bit for
bit -- the same cases as the host emulation, tests/_adamw_cases.py), then lwm_amd.optim.FusedAdamW under the 2-layer debug
model -- master / working-copy consistency, version counters, the restatement on the captured gradients, no stale weight
cache -- its state_dict round trip, and the --lwm_fused_optimizer switch of the training command line."""
import ast
import copy
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _adamw_cases as K
from tests import _adamw_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 1024


def _run(specs, data, **kw):
    import torch
    from lwm_amd._lib import lib
    return K.run(lib(), K.TorchMem(torch.device("cuda", 0)), specs, data, **kw)


@pytest.mark.parametrize("flavour", ["bf16grad_copy_decay", "f32grad_nocopy_nodecay"])
def test_single_tensors_are_bit_exact(flavour):
    half = flavour.startswith("bf16")
    for numel in K.SIZES:
        specs = [K.Spec(numel, grad_bf16=half, copy=half, decay=half, step=1 if half else 7)]
        data = K.make_data(specs, seed=numel + half)
        got = _run(specs, data, max_norm=1.0)
        K.check_bitwise(specs, data, got, what=flavour)
        K.check_norms(specs, data, got, 1.0, what=f"{flavour} n={numel}")


def test_mixed_list_edges_and_reproducibility():
    specs = K.mixed_list()
    data = K.make_data(specs, seed=5, grad_scale=3e-2)
    got = _run(specs, data, max_norm=1.0)
    assert got["norms"][1] < 1.0
    K.check_bitwise(specs, data, got, what="mixed")
    K.check_norms(specs, data, got, 1.0, what="mixed")
    again = _run(specs, data, max_norm=1.0)                       # two runs: the same bits, norms included
    assert again["norms"].tobytes() == got["norms"].tobytes()
    for k in ("p", "m", "v"):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(again[k], got[k]))
    zeros = K.make_data(specs, seed=6, zero_every=3)              # gradient entries exactly 0 with m = v = 0: v stays 0
    got = _run(specs, zeros, max_norm=1.0)
    K.check_bitwise(specs, zeros, got, what="zeros")
    K.check_norms(specs, zeros, got, 1.0, what="zeros")
    for d in zeros:
        d["g"][:] = 0
    got = _run(specs, zeros, max_norm=1.0)                        # all-zero gradients: norm 0, coefficient 1
    assert got["norms"][0] == 0 and got["norms"][1] == 1
    K.check_bitwise(specs, zeros, got, what="all-zero")
    big = K.make_data(specs, seed=7, grad_scale=3.0)
    got = _run(specs, big, max_norm=-1.0)                         # max_norm <= 0: no clipping
    assert got["norms"][0] > 100 and got["norms"][1] == 1
    K.check_bitwise(specs, big, got, what="max_norm=-1")
    small = K.make_data(specs, seed=8, grad_scale=1e-6)           # a norm below max_norm
    got = _run(specs, small, max_norm=1.0)
    assert got["norms"][0] < 1 and got["norms"][1] == 1
    K.check_bitwise(specs, small, got, what="below")
    K.check_norms(specs, small, got, 1.0, what="below")


def test_wrapper_names_the_offending_tensor():
    import torch
    from lwm_amd import optim as ops
    dev = torch.device("cuda", 0)
    p = torch.zeros(64, device=dev)
    ok = ("w", p, torch.zeros(64, device=dev), torch.zeros(64, device=dev), torch.zeros(64, device=dev), None, True, 1)

    def bad(**kw):
        e = dict(zip(("name", "master", "grad", "m", "v", "copy", "decay", "step"), ok))
        e.update(kw)
        return [tuple(e.values())]

    ops.adamw_tensor_table([ok], 0.9, 0.95)
    for what, entries in (("grad of w", bad(grad=torch.zeros(64))),                                      # a CPU tensor
                          ("exp_avg of w", bad(m=torch.zeros(64, device=dev, dtype=torch.bfloat16))),    # dtype
                          ("exp_avg_sq of w", bad(v=torch.zeros(32, device=dev))),                       # shape
                          ("grad of w", bad(grad=torch.zeros(128, device=dev)[::2])),                    # strides
                          ("master of w", bad(master=torch.zeros(66, device=dev)[2:], grad=torch.zeros(64, device=dev))),
                          ("bf16 copy of w", bad(copy=torch.zeros(64, device=dev)))):
        with pytest.raises(ValueError, match=what):
            ops.adamw_tensor_table(entries, 0.9, 0.95)


# ---------------------------------------------------------------- FusedAdamW under the debug model
HP = dict(lr=1e-2, betas=(0.9, 0.95), eps=1e-8, weight_decay=1e-4)
CLIP = 1.0


def _cfg():
    from lwm_amd.llama import LLaMAConfig
    return LLaMAConfig.load_config("debug").update(dict(vocab_size=512, max_sequence_length=S, theta=1000000))


def _model(dtype, seed=3):
    import torch
    from lwm_amd.llama import LLaMAForCausalLM
    torch.manual_seed(seed)
    with torch.device("cuda:0"):
        return LLaMAForCausalLM(_cfg(), dtype)


def _tokens():
    import torch
    return torch.randint(0, 512, (1, S + 1), generator=torch.Generator().manual_seed(1)).cuda()


def _loss(model, tok):
    return model.loss(tok[:, :-1], tok[:, 1:])[0]


def _bits(t):
    import torch
    return t.detach().contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).cpu().numpy()


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_two_steps_on_the_debug_model(dtype):
    import torch
    from lwm_amd.optim import FusedAdamW
    td = torch.bfloat16 if dtype == "bf16" else torch.float32
    model, tok = _model(td), _tokens()
    params = list(model.parameters())
    assert any(p.dtype == td for p in params)
    opt = FusedAdamW(params, max_grad_norm=CLIP, **HP)
    for step in (1, 2):
        _loss(model, tok).backward()
        grads = [p.grad.detach().float().cpu().numpy().reshape(-1) for p in params]
        # (a bf16 model keeps its norm weights in f32: those are their own masters)
        before = [(opt.state[p]["master"] if step > 1 and p.dtype == torch.bfloat16 else p.detach().float()).cpu().numpy().reshape(-1)
                  for p in params]
        moments = [(opt.state[p]["exp_avg"].cpu().numpy().reshape(-1), opt.state[p]["exp_avg_sq"].cpu().numpy().reshape(-1))
                   if step > 1 else (np.zeros(p.numel(), np.float32), np.zeros(p.numel(), np.float32)) for p in params]
        versions = [p._version for p in params]
        opt.step()
        opt.zero_grad(set_to_none=True)
        gn, coef, pn = float(opt.grad_norm), opt.clip_coef.cpu().numpy(), float(opt.param_norm)
        ref_gn = R.norm64(grads)
        assert abs(gn - ref_gn) <= 2.0 ** -22 * ref_gn, (gn, ref_gn)
        assert coef.view(np.uint32) == R.clip_coef(np.float32(gn), CLIP).view(np.uint32)
        new = []
        for p, g, b, (m, v), ver in zip(params, grads, before, moments, versions):
            assert p._version > ver                                                   # the caches keyed on it see the write
            rp, rm, rv, rw = R.update(b, m, v, g, coef, step, decay=True, **HP)        # the restatement on the captured gradients
            st = opt.state[p]
            assert st["step"] == step
            assert np.array_equal(_bits(st["exp_avg"]).reshape(-1), rm.view(np.int32))
            assert np.array_equal(_bits(st["exp_avg_sq"]).reshape(-1), rv.view(np.int32))
            if p.dtype == torch.bfloat16:
                assert st["master"].dtype == torch.float32
                assert np.array_equal(_bits(st["master"]).reshape(-1), rp.view(np.int32))
                assert torch.equal(p.detach(), st["master"].to(torch.bfloat16))       # the working copy IS bf16(master)
                assert np.array_equal(_bits(p).reshape(-1), rw.view(np.int16))
            else:
                assert "master" not in st
                assert np.array_equal(_bits(p).reshape(-1), rp.view(np.int32))
            new.append(rp)
        ref_pn = R.norm64(new)
        assert abs(pn - ref_pn) <= 2.0 ** -22 * ref_pn, (pn, ref_pn)
        # no stale cache: the next forward's loss is, bitwise, that of a freshly built model holding these parameters
        with torch.no_grad():
            loss = _loss(model, tok)
            fresh = _model(td, seed=99)
            fresh.load_state_dict(model.state_dict())
            assert torch.equal(loss, _loss(fresh, tok)), (step, float(loss))
            del fresh


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_state_dict_resume_is_bit_identical(dtype):
    import torch
    from lwm_amd.optim import FusedAdamW
    td = torch.bfloat16 if dtype == "bf16" else torch.float32
    tok = _tokens()

    def one_step(model, opt):
        _loss(model, tok).backward()
        opt.step()
        opt.zero_grad(set_to_none=True)

    model = _model(td)
    opt = FusedAdamW(model.parameters(), max_grad_norm=CLIP, **HP)
    one_step(model, opt)
    saved_opt = copy.deepcopy(opt.state_dict())
    saved_model = {k: v.clone() for k, v in model.state_dict().items()}
    one_step(model, opt)
    model2 = _model(td, seed=77)
    model2.load_state_dict(saved_model)
    opt2 = FusedAdamW(model2.parameters(), lr=1.0, betas=(0.5, 0.5), eps=1.0, weight_decay=0.5, max_grad_norm=0.0)
    opt2.load_state_dict(saved_opt)
    assert opt2.param_groups[0]["lr"] == HP["lr"] and opt2.param_groups[0]["max_grad_norm"] == CLIP
    for p in model2.parameters():
        st = opt2.state[p]
        assert st["step"] == 1 and st["exp_avg"].dtype == st["exp_avg_sq"].dtype == torch.float32
        assert ("master" in st) == (p.dtype == torch.bfloat16) and (p.dtype != torch.bfloat16 or st["master"].dtype == torch.float32)
    one_step(model2, opt2)
    for (n, a), b in zip(model.named_parameters(), model2.parameters()):
        assert torch.equal(a.detach(), b.detach()), n
        for k in opt.state[a]:
            x, y = opt.state[a][k], opt2.state[b][k]
            assert torch.equal(x, y) if isinstance(x, torch.Tensor) else x == y, (n, k)
    assert torch.equal(opt.grad_norm, opt2.grad_norm) and torch.equal(opt.param_norm, opt2.param_norm)


def test_parameter_without_gradient_keeps_its_own_step_count():
    import torch
    from lwm_amd.optim import FusedAdamW
    dev = torch.device("cuda", 0)
    a = torch.nn.Parameter(torch.full((100,), 0.5, device=dev))
    b = torch.nn.Parameter(torch.full((40,), 0.25, device=dev, dtype=torch.bfloat16))
    opt = FusedAdamW([a, b], max_grad_norm=0.0, decay_mask=[True, False], **HP)
    a.grad = torch.full_like(a, 0.1)
    opt.step()                                                   # b has no gradient: left out, not counted
    assert opt.state[a]["step"] == 1 and b not in opt.state and torch.equal(b.detach(), torch.full_like(b, 0.25))
    a.grad, b.grad = torch.full_like(a, 0.1), torch.full_like(b, 0.1)
    pa, ma, va = (t.cpu().numpy() for t in (a.detach(), opt.state[a]["exp_avg"], opt.state[a]["exp_avg_sq"]))
    opt.step()
    assert opt.state[a]["step"] == 2 and opt.state[b]["step"] == 1
    coef = opt.clip_coef.cpu().numpy()
    ra = R.update(pa, ma, va, np.full(100, 0.1, np.float32), coef, 2, decay=True, **HP)[0]
    g_b = R.from_bf16_bits(R.to_bf16_bits(np.full(40, 0.1, np.float32)))
    rb = R.update(np.full(40, 0.25, np.float32), np.zeros(40, np.float32), np.zeros(40, np.float32), g_b, coef, 1, decay=False, **HP)
    assert np.array_equal(_bits(a), ra.view(np.int32))
    assert np.array_equal(_bits(opt.state[b]["master"]), rb[0].view(np.int32)) and np.array_equal(_bits(b), rb[3].view(np.int16))


def test_train_cli_with_the_fused_optimizer(tmp_path):
    import torch
    dump = str(tmp_path / "dump.pt")
    argv = [sys.executable, "-m", "lwm_amd.cli.train", "--mesh_dim=1,1,1,1", "--dtype=bf16", "--total_steps=2", "--log_freq=1",
            "--load_llama_config=debug", "--seed=11", f"--update_llama_config=dict(vocab_size=512,max_sequence_length={S},theta=1000000)",
            "--train_dataset.type=json", f"--train_dataset.json_dataset.seq_length={S}", "--train_dataset.json_dataset.batch_size=1",
            "--optimizer.adamw_optimizer.lr=1e-4", f"--lwm_dump_grads={dump}", "--lwm_fused_optimizer"]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run(argv, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    recs = [ast.literal_eval(l) for l in r.stdout.splitlines() if l.startswith("{'step'")]
    assert [x["step"] for x in recs] == [0, 1], r.stdout[-2000:]
    for x in recs:
        assert math.isfinite(x["gradient_norm"]) and x["gradient_norm"] > 0 and math.isfinite(x["param_norm"]) and x["param_norm"] > 0
    d = torch.load(dump)
    ref = R.norm64([g.numpy() for g in d["grads"].values()])      # dumped before clipping, the last step's
    print(f"cli: gradient_norm {recs[-1]['gradient_norm']!r}, f64 of the dumped gradients {ref!r}")
    assert abs(recs[-1]["gradient_norm"] - ref) <= 2.0 ** -22 * ref, (recs[-1]["gradient_norm"], ref)
