"""The cases of the fused AdamW kernels and the harness that drives lwm_adamw_grad_norm + lwm_adamw_step through the C ABI
over guarded buffers -- shared by the host emulation (tests/test_emu_adamw.py: numpy memory) and the device
(tests/test_gpu_adamw.py: torch memory).  A `mem` object places a numpy array in the memory the library under test
reads (`put` -> address) and brings it back (`get`)."""
import ctypes as C

import numpy as np

from lwm_amd import _capi
from lwm_amd.optim import ADAMW_CHUNK, adamw_chunk_table
from tests import _adamw_ref as R

CH = ADAMW_CHUNK
SIZES = (1, 3, 8, CH - 1, CH, CH + 1, 2 * CH + 5)
HP = dict(lr=1e-2, betas=(0.9, 0.95), eps=1e-8, weight_decay=1e-4)
GUARD = 64                       # elements on either side of every buffer (a multiple of 8: the data stays 16-byte aligned)
SENT32, SENT16 = 0x7FC5A5A5, 0x7FA5     # NaN patterns: a guard that is read poisons the result, one that is written changes


class Spec:
    def __init__(self, numel, grad_bf16=True, copy=True, decay=True, step=1):
        self.numel, self.grad_bf16, self.copy, self.decay, self.step = numel, grad_bf16, copy, decay, step

    def __repr__(self):
        return f"Spec({self.numel}, grad_bf16={self.grad_bf16}, copy={self.copy}, decay={self.decay}, step={self.step})"


def mixed_list():
    """every size in ONE call: bf16-grad / copy / decay-on beside f32-grad / no-copy / decay-off, step counts that differ"""
    out = []
    for i, n in enumerate(SIZES):
        out.append(Spec(n, grad_bf16=i % 2 == 0, copy=i % 2 == 0, decay=i % 2 == 0, step=1 + i))
    out.append(Spec(CH + 9, grad_bf16=True, copy=False, decay=False, step=3))
    out.append(Spec(13, grad_bf16=False, copy=True, decay=True, step=40))
    return out


def make_data(specs, seed, grad_scale=1e-2, zero_every=0):
    """per tensor: p ~ 0.02 * N(0,1), m and v as after a few steps (v >= 0), g ~ grad_scale * N(0,1) (rounded to bf16 where
    the gradient is bf16; every zero_every-th entry exactly 0)"""
    rng = np.random.default_rng(seed)
    data = []
    for s in specs:
        n = s.numel
        g = (rng.standard_normal(n) * grad_scale).astype(np.float32)
        if zero_every:
            g[::zero_every] = 0.0
        if s.grad_bf16:
            g = R.from_bf16_bits(R.to_bf16_bits(g))
        first = s.step == 1
        m = np.zeros(n, np.float32) if first else (rng.standard_normal(n) * grad_scale * 0.3).astype(np.float32)
        v = np.zeros(n, np.float32) if first else ((rng.standard_normal(n) * grad_scale) ** 2 * 0.1).astype(np.float32)
        if zero_every and not first:
            v[::zero_every] = 0.0
            m[::zero_every] = 0.0
        data.append(dict(p=(rng.standard_normal(n) * 0.02).astype(np.float32), m=m, v=v, g=g))
    return data


class NumpyMem:
    """host memory: the emulated library reads numpy buffers in place"""

    def __init__(self):
        from tests import _emu
        self._aligned = _emu.aligned
        self.bufs = []

    def put(self, arr):
        a = self._aligned(arr.shape, arr.dtype)
        a[...] = arr
        self.bufs.append(a)
        return len(self.bufs) - 1, a.ctypes.data

    def get(self, i):
        return self.bufs[i]

    def stream(self):
        return None

    def sync(self):
        pass


class TorchMem:
    """device memory: arrays travel as raw bytes (no dtype is reinterpreted by torch)"""

    def __init__(self, device):
        import torch
        self.torch, self.dev, self.bufs = torch, device, []

    def put(self, arr):
        t = self.torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1).copy()).to(self.dev)
        assert t.data_ptr() % 16 == 0
        self.bufs.append((t, arr.dtype, arr.shape))
        return len(self.bufs) - 1, t.data_ptr()

    def get(self, i):
        t, dtype, shape = self.bufs[i]
        return t.cpu().numpy().view(dtype).reshape(shape)

    def stream(self):
        return C.c_void_p(self.torch.cuda.current_stream().cuda_stream)

    def sync(self):
        self.torch.cuda.synchronize()


def _guarded(x, sent):
    out = np.full(x.size + 2 * GUARD, sent, dtype={4: np.uint32, 2: np.uint16}[x.dtype.itemsize])
    out[GUARD:GUARD + x.size] = x.view(out.dtype)
    return out


def run(L, mem, specs, data, hp=HP, max_norm=1.0):
    """One lwm_adamw_grad_norm + lwm_adamw_step over the list.  -> dict(p, m, v: lists of f32 arrays; w: list of bf16 bit
    arrays or None; norms: f32[3]).  Asserts that every guard -- around each tensor buffer, the norms and the partials --
    came back untouched and that the gradients were not written."""
    held = []            # (handle, kind, tensor, dtype, numel)
    tab = (_capi.LwmAdamWTensor * len(specs))()
    isz = lambda dt: np.dtype(dt).itemsize

    def place(kind, i, x):
        sent = SENT32 if x.dtype.itemsize == 4 else SENT16
        h, ptr = mem.put(_guarded(x, sent))
        held.append((h, kind, i, x.dtype, x.size, sent))
        return ptr + GUARD * isz(x.dtype)

    for i, (s, d) in enumerate(zip(specs, data)):
        e = tab[i]
        e.master, e.exp_avg, e.exp_avg_sq = place("p", i, d["p"]), place("m", i, d["m"]), place("v", i, d["v"])
        e.grad = place("g", i, R.to_bf16_bits(d["g"]) if s.grad_bf16 else d["g"])
        e.copy_bf16 = place("w", i, np.full(s.numel, 0x1234, np.uint16)) if s.copy else None
        e.numel, e.grad_bf16, e.decay = s.numel, int(s.grad_bf16), int(s.decay)
        e.bias_corr1, e.sqrt_bias_corr2 = R.bias_corrections(s.step, *hp["betas"])
    chunks = adamw_chunk_table([s.numel for s in specs], CH)
    nc = chunks.shape[0]
    _, tab_ptr = mem.put(np.frombuffer(bytes(tab), dtype=np.uint8).copy())
    _, ch_ptr = mem.put(chunks.reshape(-1))
    a = _capi.LwmAdamWArgs()
    a.tensors, a.chunks, a.n_tensors, a.n_chunks = tab_ptr, ch_ptr, len(specs), nc
    a.lr, (a.beta1, a.beta2), a.eps, a.weight_decay, a.max_norm = hp["lr"], hp["betas"], hp["eps"], hp["weight_decay"], max_norm
    # the f64 workspaces and the norms sit between guards too (as u32 words)
    gp = place("gpart", -1, np.zeros(2 * nc, np.uint32))
    pp = place("ppart", -1, np.zeros(2 * nc, np.uint32))
    nr = place("norms", -1, np.zeros(3, np.float32).view(np.uint32))
    a.grad_partials, a.grad_partials_len, a.param_partials, a.param_partials_len, a.norms = gp, nc, pp, nc, nr
    st = mem.stream()
    _capi.check(L, L.lwm_adamw_grad_norm(C.byref(a), st), "lwm_adamw_grad_norm")
    _capi.check(L, L.lwm_adamw_step(C.byref(a), st), "lwm_adamw_step")
    mem.sync()
    out = dict(p=[None] * len(specs), m=[None] * len(specs), v=[None] * len(specs), w=[None] * len(specs), norms=None)
    for h, kind, i, dtype, n, sent in held:
        raw = mem.get(h)
        assert (raw[:GUARD] == sent).all() and (raw[GUARD + n:] == sent).all(), f"guard of {kind}[{i}] was written"
        body = raw[GUARD:GUARD + n].copy()
        if kind in ("p", "m", "v"):
            out[kind][i] = body.view(np.float32)
        elif kind == "w":
            out["w"][i] = body
        elif kind == "g":
            ref = R.to_bf16_bits(data[i]["g"]) if specs[i].grad_bf16 else data[i]["g"].view(np.uint32)
            assert np.array_equal(body, ref), f"gradient {i} was written"
        elif kind == "norms":
            out["norms"] = body.view(np.float32)
    return out


def check_bitwise(specs, data, got, hp=HP, what=""):
    """master, exp_avg, exp_avg_sq and the bf16 copy BITWISE against the restatement fed the kernel's own coefficient"""
    coef = got["norms"][1]
    for i, (s, d) in enumerate(zip(specs, data)):
        p, m, v, w = R.update(d["p"], d["m"], d["v"], d["g"], coef, s.step, decay=s.decay, **hp)
        for name, ref, out in (("master", p, got["p"][i]), ("exp_avg", m, got["m"][i]), ("exp_avg_sq", v, got["v"][i])):
            bad = np.flatnonzero(ref.view(np.uint32) != out.view(np.uint32))
            assert bad.size == 0, (what, s, name, bad[:5], ref[bad[:5]], out[bad[:5]])
        if s.copy:
            bad = np.flatnonzero(w != got["w"][i])
            assert bad.size == 0, (what, s, "bf16 copy", bad[:5])
        else:
            assert got["w"][i] is None


def check_norms(specs, data, got, max_norm, what=""):
    """norms[0] and norms[2] within 2^-22 relative of the float64 values; the coefficient is the f32 formula of norms[0]"""
    gn = R.norm64([d["g"] for d in data])
    pn = R.norm64(got["p"])
    n = got["norms"]
    print(f"{what}: grad norm {n[0]!r} (f64 {gn!r}, rel {abs(float(n[0]) - gn) / max(gn, 1e-300):.3e}), coef {n[1]!r}, "
          f"param norm {n[2]!r} (f64 {pn!r}, rel {abs(float(n[2]) - pn) / max(pn, 1e-300):.3e})")
    assert abs(float(n[0]) - gn) <= 2.0 ** -22 * gn, (what, n[0], gn)
    assert abs(float(n[2]) - pn) <= 2.0 ** -22 * pn, (what, n[2], pn)
    assert n[1].view(np.uint32) == R.clip_coef(n[0], max_norm).view(np.uint32), (what, n[1], R.clip_coef(n[0], max_norm))
