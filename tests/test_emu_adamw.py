"""The fused AdamW (lwm_adamw_grad_norm + lwm_adamw_step, lwm_amd/csrc/optim.h) in the host emulation, through the C ABI:
bit for bit against the numpy restatement of tests/_adamw_ref.py, the norms against float64, the restatement itself
against torch.optim.AdamW + clip_grad_norm_ in float64 -- and the argument validation on the real library (no GPU:
every bad argument is refused before a launch)."""
import ctypes as C
import os

import numpy as np
import pytest

from lwm_amd import _capi
from tests import _adamw_cases as K
from tests import _adamw_ref as R
from tests import _emu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(specs, data, **kw):
    return K.run(_emu.lib(), K.NumpyMem(), specs, data, **kw)


def test_chunk_constant_and_struct_sizes():
    L = _emu.lib()
    assert L.lwm_adamw_chunk() == K.CH
    assert L.lwm_sizeof(7) == C.sizeof(_capi.LwmAdamWArgs) and L.lwm_sizeof(8) == C.sizeof(_capi.LwmAdamWTensor)
    assert L.lwm_version() >= 540


@pytest.mark.parametrize("numel", K.SIZES)
@pytest.mark.parametrize("flavour", ["bf16grad_copy_decay", "f32grad_nocopy_nodecay"])
def test_single_tensor_is_bit_exact(numel, flavour):
    half = flavour.startswith("bf16")
    specs = [K.Spec(numel, grad_bf16=half, copy=half, decay=half, step=1 if half else 7)]
    data = K.make_data(specs, seed=numel + half)
    got = _run(specs, data, max_norm=1.0)
    K.check_bitwise(specs, data, got, what=flavour)
    K.check_norms(specs, data, got, 1.0, what=f"{flavour} n={numel}")


def test_mixed_list_in_one_call_is_bit_exact():
    specs = K.mixed_list()
    data = K.make_data(specs, seed=5, grad_scale=3e-2)
    got = _run(specs, data, max_norm=1.0)
    assert got["norms"][1] < 1.0                                  # the norm lies above max_norm: the gradients are scaled
    K.check_bitwise(specs, data, got, what="mixed")
    K.check_norms(specs, data, got, 1.0, what="mixed")


def test_edge_inputs():
    specs = K.mixed_list()
    # some gradient entries exactly 0 (and m = v = 0 there): v stays 0, den = eps, the update is 0 / eps = 0
    data = K.make_data(specs, seed=6, zero_every=3)
    got = _run(specs, data, max_norm=1.0)
    K.check_bitwise(specs, data, got, what="zeros")
    K.check_norms(specs, data, got, 1.0, what="zeros")
    assert all((v[::3] == 0).all() for v in got["v"]) and all(np.isfinite(p).all() for p in got["p"])
    # all-zero gradients: norm 0, coefficient 1
    for d in data:
        d["g"][:] = 0
    got = _run(specs, data, max_norm=1.0)
    assert got["norms"][0] == 0 and got["norms"][1] == 1
    K.check_bitwise(specs, data, got, what="all-zero")
    # max_norm <= 0: no clipping whatever the norm
    data = K.make_data(specs, seed=7, grad_scale=3.0)
    for mx in (0.0, -1.0):
        got = _run(specs, data, max_norm=mx)
        assert got["norms"][0] > 100 and got["norms"][1] == 1
        K.check_bitwise(specs, data, got, what=f"max_norm={mx}")
        K.check_norms(specs, data, got, mx, what=f"max_norm={mx}")
    # a norm below max_norm (coefficient exactly 1) and one above it
    small = K.make_data(specs, seed=8, grad_scale=1e-6)
    got = _run(specs, small, max_norm=1.0)
    assert got["norms"][0] < 1 and got["norms"][1] == 1
    K.check_bitwise(specs, small, got, what="below")
    K.check_norms(specs, small, got, 1.0, what="below")
    got = _run(specs, data, max_norm=1.0)
    assert got["norms"][0] > 1 and 0 < got["norms"][1] < 1
    K.check_bitwise(specs, data, got, what="above")
    K.check_norms(specs, data, got, 1.0, what="above")


def test_non_finite_gradients_propagate_without_a_fault():
    specs = [K.Spec(K.CH + 1, grad_bf16=False, copy=True)]
    data = K.make_data(specs, seed=9)
    data[0]["g"][5] = np.inf
    got = _run(specs, data, max_norm=1.0)
    assert np.isinf(got["norms"][0]) and got["norms"][1] == 0 and np.isnan(got["p"][0][5])
    assert np.isfinite(np.delete(got["p"][0], 5)).all()            # inf * 0 is NaN for that entry alone


def test_two_runs_are_bitwise_equal():
    specs = K.mixed_list()
    data = K.make_data(specs, seed=10)
    a, b = _run(specs, data), _run(specs, data)
    assert a["norms"].tobytes() == b["norms"].tobytes()
    for k in ("p", "m", "v"):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a[k], b[k]))


@pytest.mark.parametrize("scale", [1e-6, 1e-3, 3.0])
def test_restatement_matches_torch_adamw_and_clip_in_float64(scale):
    """The anchor of the restatement: torch.optim.AdamW(foreach=False) + clip_grad_norm_ in float64 on the CPU, one step at
    a time FROM THE SAME f32 STATE (what is compared is one step's arithmetic, not four steps' drift).  lr = 1e-2: at LWM's
    8e-5 the f32 quantisation of p alone puts the error of the update at 5e-5 of its maximum.  Bound: 1e-5 of the maximum,
    the project's f32 bound, on the update p_new - p_old, on m and on v."""
    import torch
    n, hp, max_norm = 4099, K.HP, 1.0
    rng = np.random.default_rng(int(scale * 1e6) + 1)
    p = (rng.standard_normal(n) * 0.02).astype(np.float32)
    m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    for step in range(1, 5):
        g = R.from_bf16_bits(R.to_bf16_bits((rng.standard_normal(n) * scale).astype(np.float32)))
        tp = torch.nn.Parameter(torch.from_numpy(p.astype(np.float64)))
        opt = torch.optim.AdamW([tp], lr=hp["lr"], betas=hp["betas"], eps=hp["eps"], weight_decay=hp["weight_decay"], foreach=False)
        opt.state[tp] = dict(step=torch.tensor(float(step - 1)), exp_avg=torch.from_numpy(m.astype(np.float64)),
                             exp_avg_sq=torch.from_numpy(v.astype(np.float64)))
        tp.grad = torch.from_numpy(g.astype(np.float64))
        tnorm = float(torch.nn.utils.clip_grad_norm_([tp], max_norm))
        opt.step()
        norm = np.float32(R.norm64([g]))
        p2, m2, v2, _ = R.update(p, m, v, g, R.clip_coef(norm, max_norm), step, **hp)
        upd_ref = tp.detach().numpy() - p.astype(np.float64)
        upd = p2.astype(np.float64) - p.astype(np.float64)
        errs = {}
        for name, got, ref in (("update", upd, upd_ref), ("m", m2, opt.state[tp]["exp_avg"].numpy()),
                               ("v", v2, opt.state[tp]["exp_avg_sq"].numpy())):
            errs[name] = float(np.abs(got - ref).max() / np.abs(ref).max())
        errs["norm"] = abs(float(norm) - tnorm) / tnorm
        print(f"scale {scale} step {step}: error / max {errs}")
        assert all(e <= 1e-5 for e in errs.values()), (scale, step, errs)
        p, m, v = p2, m2, v2


def test_wrappers_refuse_host_tensors_before_the_library():
    """lwm_amd has no CPU path: well-formed tensors that live on the host are refused by name, nothing is launched"""
    import torch
    from lwm_amd import optim
    z = lambda *a, **k: torch.zeros(*a, **k)
    with pytest.raises(ValueError, match="master of w"):
        optim.adamw_tensor_table([("w", z(64), z(64), z(64), z(64), None, True, 1)], 0.9, 0.95)
    with pytest.raises(ValueError, match="adamw: tensors"):
        optim.adamw_launch(z(0, dtype=torch.uint8), z(0, 2, dtype=torch.int32), 0, lr=1e-3, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.0,
                           max_norm=1.0, grad_partials=z(1, dtype=torch.float64), param_partials=z(1, dtype=torch.float64), norms=z(3))
    with pytest.raises(ValueError, match="parameter 0"):
        optim.FusedAdamW([torch.nn.Parameter(z(8))])


@pytest.fixture(scope="module")
def real_lib():
    so = os.path.join(ROOT, "lwm_amd", "liblwm_hip.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    return _capi.bind(C.CDLL(so))


def test_validation_refuses_bad_arguments_before_any_launch(real_lib):
    L = real_lib
    assert L.lwm_sizeof(7) == C.sizeof(_capi.LwmAdamWArgs) and L.lwm_sizeof(8) == C.sizeof(_capi.LwmAdamWTensor)
    assert L.lwm_version() >= 540 and L.lwm_adamw_chunk() == K.CH
    buf = (C.c_char * 8192)()
    base = C.addressof(buf)
    base += (-base) % 16

    def good():
        a = _capi.LwmAdamWArgs()
        a.tensors, a.chunks, a.n_tensors, a.n_chunks = base, base + 1024, 2, 5
        a.lr, a.beta1, a.beta2, a.eps, a.weight_decay, a.max_norm = 1e-2, 0.9, 0.95, 1e-8, 1e-4, 1.0
        a.grad_partials, a.grad_partials_len = base + 2048, 5
        a.param_partials, a.param_partials_len = base + 4096, 5
        a.norms = base + 6144
        return a

    nan, inf = float("nan"), float("inf")
    cases = [dict(tensors=None), dict(chunks=None), dict(n_tensors=-1), dict(n_chunks=-1), dict(n_tensors=0),
             dict(lr=-1e-3), dict(lr=nan), dict(lr=inf), dict(eps=-1e-8), dict(eps=nan), dict(eps=inf),
             dict(weight_decay=-1.0), dict(weight_decay=nan), dict(beta1=1.0), dict(beta1=-0.1), dict(beta1=nan),
             dict(beta2=1.0), dict(beta2=-0.1), dict(beta2=nan), dict(max_norm=nan),
             dict(grad_partials=None), dict(param_partials=None), dict(norms=None),
             dict(grad_partials_len=4), dict(param_partials_len=4),
             dict(tensors=base + 4), dict(chunks=base + 1026), dict(grad_partials=base + 2052), dict(norms=base + 6146)]
    for entry, prefix in ((L.lwm_adamw_grad_norm, b"adamw_grad_norm"), (L.lwm_adamw_step, b"adamw_step")):
        for fields in cases:
            a = good()
            for f, v in fields.items():
                setattr(a, f, v)
            assert entry(C.byref(a), None) == _capi.LWM_EINVAL, fields
            assert L.lwm_last_error().startswith(prefix), (fields, L.lwm_last_error())
        assert entry(None, None) == _capi.LWM_EINVAL
