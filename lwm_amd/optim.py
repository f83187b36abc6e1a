"""FusedAdamW -- gradient clipping by the global norm and AdamW in four launches of hand-written HIP (csrc/optim.h,
lwm_adamw_grad_norm + lwm_adamw_step), on f32 master weights.

What it replaces in a training step: torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW -- a dozen library passes over
every parameter and a norm pass of their own -- and, for bf16 parameters, their arithmetic: torch keeps bf16 moments and
adds the update into the bf16 weight, where an update of lr * u below half an ulp of the weight (1.2e-4 at |w| = 0.02) is
rounded away.  The reference keeps parameters in f32 and casts them for compute (param_dtype=jnp.float32,
lwm/llama.py:324,381): here a bf16 parameter has an f32 `master` in the optimizer state, the moments are f32, and the
bf16 tensor the model computes with is the rounded copy of the master, rewritten by the update kernel in the same pass.
An f32 parameter is its own master.

The norms the reference logs every step (lwm/train.py:216-222) come out of the same passes: `grad_norm` (before
clipping), `clip_coef` and `param_norm` (after the update, over the parameters this step updated) are 0-d device tensors
-- reading one is a host synchronisation, so read them only when logging.

Memory: 12 bytes of f32 state per bf16 parameter (master + two moments) against torch's 4 (two bf16 moments) -- 81 GB
against 27 GB at LWM-7B's 6.74e9 parameters.  Hence opt-in.
"""
import ctypes as C
import math

import torch

from . import _capi
from ._lib import lib
from .ops import _stream_ptr


# ---------------------------------------------------------------- the C entry points (lwm_adamw_*, csrc/optim.h)
ADAMW_CHUNK = 8192      # lwm_adamw_chunk(): checked against the library by adamw_launch


def adamw_chunk_table(numels, chunk=ADAMW_CHUNK):
    """The chunk table of a list of tensors of `numels` elements: an int32 numpy array (n_chunks, 2) of (tensor, chunk of
    that tensor), every chunk of every tensor once, tensor by tensor.  Host arithmetic only."""
    import numpy as np
    rows = []
    for t, n in enumerate(numels):
        k = np.arange((int(n) + chunk - 1) // chunk, dtype=np.int32)
        rows.append(np.stack([np.full_like(k, t), k], 1))
    return np.concatenate(rows, 0) if rows else np.zeros((0, 2), np.int32)


def adamw_bias_corrections(step, beta1, beta2):
    """(1 - beta1^step, sqrt(1 - beta2^step)) in double -- rounded to f32 when stored in the tensor table"""
    return 1.0 - beta1 ** step, math.sqrt(1.0 - beta2 ** step)


def adamw_tensor_table(entries, beta1, beta2):
    """The tensor table of the fused AdamW as a CPU uint8 tensor (one LwmAdamWTensor per entry), ready to be copied to
    the device.  entries: (name, master, grad, exp_avg, exp_avg_sq, copy or None, decay, step) -- master and moments
    f32, grad bf16 or f32, copy bf16; all contiguous device tensors of one shape on one device with 16-byte aligned
    bases; step >= 1 is the count of updates of that tensor INCLUDING this one."""
    tab = (_capi.LwmAdamWTensor * max(len(entries), 1))()
    dev = None
    for i, (name, master, grad, m, v, copy, decay, step) in enumerate(entries):
        dev = master.device if dev is None else dev
        for what, t, dtypes in (("master", master, (torch.float32,)), ("grad", grad, (torch.bfloat16, torch.float32)),
                                ("exp_avg", m, (torch.float32,)), ("exp_avg_sq", v, (torch.float32,)),
                                ("bf16 copy", copy, (torch.bfloat16,))):
            if t is None and what == "bf16 copy":
                continue
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise ValueError(f"adamw: {what} of {name}: expected a ROCm device tensor (lwm_amd has no CPU path)")
            if t.device != dev:
                raise ValueError(f"adamw: {what} of {name}: on {t.device}, the list is on {dev}")
            if t.dtype not in dtypes:
                raise ValueError(f"adamw: {what} of {name}: dtype {t.dtype}, expected {' or '.join(str(d) for d in dtypes)}")
            if tuple(t.shape) != tuple(master.shape):
                raise ValueError(f"adamw: {what} of {name}: shape {tuple(t.shape)}, the parameter has {tuple(master.shape)}")
            if not t.is_contiguous():
                raise ValueError(f"adamw: {what} of {name}: not contiguous (strides {t.stride()})")
            if t.data_ptr() % 16:
                raise ValueError(f"adamw: {what} of {name}: base {t.data_ptr():#x} is not 16-byte aligned")
        if int(step) < 1:
            raise ValueError(f"adamw: {name}: step {step} (the count of updates including this one, >= 1)")
        bc1, sbc2 = adamw_bias_corrections(int(step), beta1, beta2)
        e = tab[i]
        e.master, e.grad, e.exp_avg, e.exp_avg_sq = master.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr()
        e.copy_bf16 = None if copy is None else copy.data_ptr()
        e.numel, e.grad_bf16, e.decay = master.numel(), int(grad.dtype == torch.bfloat16), int(bool(decay))
        e.bias_corr1, e.sqrt_bias_corr2 = bc1, sbc2
    n = len(entries) * C.sizeof(_capi.LwmAdamWTensor)
    return torch.frombuffer(bytearray(bytes(tab)[:n]), dtype=torch.uint8) if n else torch.zeros(0, dtype=torch.uint8)


def adamw_launch(tensors, chunks, n_tensors, *, lr, betas, eps, weight_decay, max_norm, grad_partials, param_partials, norms):
    """Gradient norm + clipping coefficient, then the AdamW update and the parameter norm: four launches on the current
    stream, no host synchronisation.  tensors: the device copy of adamw_tensor_table's bytes; chunks: (n_chunks, 2) int32
    device tensor (adamw_chunk_table); grad_partials / param_partials: f64 device workspaces of at least n_chunks elements;
    norms: (3,) f32 device tensor -> gradient norm, clipping coefficient, parameter norm after the update."""
    dev = norms.device if isinstance(norms, torch.Tensor) else None
    n_chunks = chunks.shape[0] if isinstance(chunks, torch.Tensor) and chunks.dim() == 2 else -1
    for name, t, dtype, ok in (("tensors", tensors, torch.uint8, lambda t: t.numel() == n_tensors * C.sizeof(_capi.LwmAdamWTensor)),
                               ("chunks", chunks, torch.int32, lambda t: t.dim() == 2 and t.shape[1] == 2),
                               ("grad_partials", grad_partials, torch.float64, lambda t: t.numel() >= n_chunks),
                               ("param_partials", param_partials, torch.float64, lambda t: t.numel() >= n_chunks),
                               ("norms", norms, torch.float32, lambda t: t.numel() == 3)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != dev or t.dtype != dtype or not t.is_contiguous() or not ok(t):
            raise ValueError(f"adamw: {name} must be a contiguous {dtype} tensor on {dev} of the documented size, got "
                             f"{getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))} on {getattr(t, 'device', None)}")
    L = lib()
    if L.lwm_adamw_chunk() != ADAMW_CHUNK:
        raise RuntimeError(f"adamw: the library cuts chunks of {L.lwm_adamw_chunk()} elements, lwm_amd.optim of {ADAMW_CHUNK}")
    a = _capi.LwmAdamWArgs()
    a.tensors, a.chunks, a.n_tensors, a.n_chunks = tensors.data_ptr(), chunks.data_ptr(), n_tensors, n_chunks
    a.lr, a.beta1, a.beta2, a.eps, a.weight_decay = float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay)
    a.max_norm = float(max_norm) if max_norm is not None else 0.0
    a.grad_partials, a.grad_partials_len = grad_partials.data_ptr(), grad_partials.numel()
    a.param_partials, a.param_partials_len = param_partials.data_ptr(), param_partials.numel()
    a.norms = norms.data_ptr()
    s = _stream_ptr()
    _capi.check(L, L.lwm_adamw_grad_norm(C.byref(a), s), "lwm_adamw_grad_norm")
    _capi.check(L, L.lwm_adamw_step(C.byref(a), s), "lwm_adamw_step")


class FusedAdamW(torch.optim.Optimizer):
    """AdamW with decoupled weight decay (torch.optim.AdamW's update, per-parameter step counts included) preceded by
    clip_grad_norm_(max_grad_norm) -- max_grad_norm <= 0 or None: no clipping.  One param group.  decay_mask: one bool per
    parameter, False = no weight decay for it (None: every parameter decays)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=0.0, decay_mask=None):
        params = list(params)
        if params and isinstance(params[0], dict):
            raise ValueError("FusedAdamW: one param group (pass the parameters, not a list of groups)")
        if not (lr >= 0.0) or not (eps >= 0.0) or not (weight_decay >= 0.0):
            raise ValueError(f"FusedAdamW: lr {lr}, eps {eps}, weight_decay {weight_decay} must be >= 0")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"FusedAdamW: betas {betas} must lie in [0, 1)")
        if decay_mask is not None:
            decay_mask = [bool(d) for d in decay_mask]
            if len(decay_mask) != len(params):
                raise ValueError(f"FusedAdamW: decay_mask has {len(decay_mask)} entries for {len(params)} parameters")
        for i, p in enumerate(params):
            if p.dtype not in (torch.bfloat16, torch.float32) or not p.is_cuda or not p.is_contiguous():
                raise ValueError(f"FusedAdamW: parameter {i}: expected a contiguous bf16 / f32 ROCm device tensor, got {p.dtype} "
                                 f"on {p.device}, strides {p.stride()}")
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay,
                                      max_grad_norm=0.0 if max_grad_norm is None else float(max_grad_norm), decay_mask=decay_mask))
        dev = params[0].device
        self._norms = torch.zeros(3, dtype=torch.float32, device=dev)
        self.grad_norm, self.clip_coef, self.param_norm = self._norms[0], self._norms[1], self._norms[2]
        self._chunks = (None, None)          # (numels of the listed tensors, device chunk table)
        self._partials = None                # (2, n_chunks) f64
        self._table = None                   # device tensor table

    def _state_of(self, p):
        st = self.state[p]
        if not st:
            st["step"] = 0
            if p.dtype == torch.bfloat16:
                st["master"] = p.detach().float()
            st["exp_avg"] = torch.zeros_like(p, dtype=torch.float32)
            st["exp_avg_sq"] = torch.zeros_like(p, dtype=torch.float32)
        return st

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        g = self.param_groups[0]
        mask = g["decay_mask"]
        entries, written = [], []
        for i, p in enumerate(g["params"]):
            if p.grad is None:
                continue
            st = self._state_of(p)
            st["step"] += 1
            half = p.dtype == torch.bfloat16
            entries.append((f"parameter {i}", st["master"] if half else p.detach(), p.grad, st["exp_avg"], st["exp_avg_sq"],
                            p.detach() if half else None, True if mask is None else mask[i], st["step"]))
            written.append(p)
        if not entries:
            return loss
        dev = self._norms.device
        # the table is rebuilt every step: zero_grad(set_to_none=True) gives the next gradients new addresses.  A fresh host
        # buffer per step, copied (pageable: the call returns when the bytes are staged) to the device buffer the launches
        # of this step read -- launches of the previous step have read theirs by then, in stream order.
        host = adamw_tensor_table(entries, g["betas"][0], g["betas"][1])
        if self._table is None or self._table.numel() != host.numel():
            self._table = torch.empty(host.numel(), dtype=torch.uint8, device=dev)
        self._table.copy_(host)
        numels = tuple(e[1].numel() for e in entries)
        if self._chunks[0] != numels:
            self._chunks = (numels, torch.from_numpy(adamw_chunk_table(numels)).to(dev))
            self._partials = torch.empty((2, max(self._chunks[1].shape[0], 1)), dtype=torch.float64, device=dev)
        adamw_launch(self._table, self._chunks[1], len(entries), lr=g["lr"], betas=g["betas"], eps=g["eps"],
                         weight_decay=g["weight_decay"], max_norm=g["max_grad_norm"], grad_partials=self._partials[0],
                         param_partials=self._partials[1], norms=self._norms)
        # the kernels wrote behind autograd: bump the version counters the weight caches are keyed on (the bf16 casts, the
        # re-laid GEMM operands, the norm weights), as torch's own fused optimizers do, and end the re-layout epoch
        for p in written:
            torch._C._increment_version(p)
        from . import llama_ops
        llama_ops.weights_changed()
        return loss

    def load_state_dict(self, state_dict):
        """Restores step counts, f32 moments and f32 masters as they were saved (torch's loader would cast the state of a
        bf16 parameter to bf16), then rewrites every bf16 parameter from its master."""
        groups = state_dict["param_groups"]
        mine = self.param_groups[0]
        if len(groups) != 1 or len(groups[0]["params"]) != len(mine["params"]):
            raise ValueError("FusedAdamW.load_state_dict: the state is of another parameter list")
        mine.update({k: v for k, v in groups[0].items() if k != "params"})
        mine["betas"] = tuple(mine["betas"])
        self.state.clear()
        with torch.no_grad():
            for pid, p in zip(groups[0]["params"], mine["params"]):
                src = state_dict["state"].get(pid)
                if src is None:
                    continue
                st = self.state[p]
                st["step"] = int(src["step"])
                for k in ("master", "exp_avg", "exp_avg_sq"):
                    if k in src:
                        if tuple(src[k].shape) != tuple(p.shape):
                            raise ValueError(f"FusedAdamW.load_state_dict: {k} of parameter {pid} has shape {tuple(src[k].shape)}, "
                                             f"the parameter {tuple(p.shape)}")
                        st[k] = src[k].detach().to(device=p.device, dtype=torch.float32, copy=True).contiguous()
                if (p.dtype == torch.bfloat16) != ("master" in st):
                    raise ValueError(f"FusedAdamW.load_state_dict: parameter {pid} is {p.dtype}, its saved state "
                                     f"{'has' if 'master' in st else 'lacks'} an f32 master")
                if "master" in st:
                    p.copy_(st["master"])
        from . import llama_ops
        llama_ops.weights_changed()
