"""The specification of the fused AdamW update (lwm_amd/csrc/optim.h, phase B) as numpy float32 arithmetic -- every
operation on float32 arrays and float32 scalars, so every operation is rounded once, in the kernel's order -- plus the
norms in float64.  The emulated and the device kernels are held to this BITWISE; test_emu_adamw.py anchors it to
torch.optim.AdamW + clip_grad_norm_ evaluated in float64."""
import math

import numpy as np

from oracle.attention_ref import from_bf16_bits, to_bf16_bits  # noqa: F401  (re-exported for the tests)

f32 = np.float32


def scalars(lr, beta1, beta2, eps, weight_decay):
    """what the C entry rounds to f32 once, from doubles"""
    return dict(lr=f32(lr), beta1=f32(beta1), om_beta1=f32(1.0 - beta1), beta2=f32(beta2), om_beta2=f32(1.0 - beta2),
                eps=f32(eps), decay=f32(1.0 - lr * weight_decay))


def bias_corrections(step, beta1, beta2):
    """the per-tensor table entries: computed in double from the tensor's own step count, stored as f32"""
    return f32(1.0 - beta1 ** step), f32(math.sqrt(1.0 - beta2 ** step))


def norm64(arrays):
    """sqrt(sum x^2) over a list of arrays, in float64"""
    return math.sqrt(sum(float(np.sum(np.asarray(a, dtype=np.float64) ** 2)) for a in arrays))


def clip_coef(norm, max_norm):
    """the finalize kernel's coefficient, from ITS f32 norm: min(1, max_norm / (norm + 1e-6)) in f32; 1 when max_norm <= 0"""
    if not max_norm > 0:
        return f32(1.0)
    c = f32(max_norm) / (f32(norm) + f32(1e-6))
    return f32(1.0) if c > f32(1.0) else c


def update(p, m, v, g, coef, step, *, lr, betas, eps, weight_decay, decay=True):
    """One tensor's update.  p, m, v: float32 arrays; g: float32 array (a bf16 gradient widened -- exact); coef: the f32
    clipping coefficient; step: this tensor's count of updates including this one.  -> (p, m, v, bf16 bits of p)"""
    s = scalars(lr, betas[0], betas[1], eps, weight_decay)
    bc1, sbc2 = bias_corrections(step, betas[0], betas[1])
    p, m, v, g = (np.asarray(a, dtype=f32) for a in (p, m, v, g))
    with np.errstate(all="ignore"):
        g = g * f32(coef)
        m = m * s["beta1"] + g * s["om_beta1"]
        v = v * s["beta2"] + (g * g) * s["om_beta2"]
        den = np.sqrt(v) / sbc2 + s["eps"]
        if decay:
            p = p * s["decay"]
        p = p - (s["lr"] / bc1) * (m / den)
    assert p.dtype == m.dtype == v.dtype == f32
    return p, m, v, to_bf16_bits(p)
