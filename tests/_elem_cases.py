"""The kernels either side of attention -- RoPE, RMSNorm forward / backward (folded residual, dW reduction), the SwiGLU
gate, the fused softmax cross entropy, the decode GEMV family -- at the shapes and values the rest of the suite does not
feed them: case builders, float64 references WITH THEIR MAGNITUDES, and the shared verdict.  The cases run twice, on the
host emulator (tests/test_emu_elem_edges.py) and on the device (tests/test_gpu_elem_edges.py), in both dtype flavours.
TEST INFRASTRUCTURE ONLY.

The verdict is per element.  For every output element the reference returns its value ref_i and a magnitude mag_i, the
sum of the absolute values of the terms that are added or subtracted to form ref_i (each output's OWN terms: the
imaginary output of a RoPE pair is x0 s + x1 c, so its magnitude is |x0 s| + |x1 c|).  A max-norm bound hides a missing
term wherever that term is small against the tensor's largest element; a bound scaled by mag_i does not.

  bf16 outputs       |got - ref| <= 2^-7 mag_i + 2^-126.  Round-to-nearest-even into bf16 costs at most 2^-8 relative;
                     the bound doubles that, which leaves 2^-8 mag for the f32 evaluation.  The floor is the smallest
                     normal f32: underflowed products may flush.
  rounded twice      (RMSNorm forward bf16(bf16(x r) w)): against the rounding-faithful oracle.  Every element equals
                     bf16(c w) for c the oracle's bf16(x r) or one of its two bf16 neighbours, and fewer than 5e-3 of
                     the elements differ from the oracle's own at all (check_twice_rounded says why "one ulp of the
                     result" cannot be kept).  The folded-residual dx, bf16(bf16(dx) + res), likewise with c around the
                     oracle's bf16(dx).
  GEMV f32 output    |got - ref| <= 64 2^-24 mag_i: no product passes more than 64 roundings on its way out (32 FMAs, 3 wave
                     adds, at most 12 partials, 3 shuffles).
  f32 flavour        the allowance is measured, per case, on the REFERENCE side: the same formulas evaluated in numpy
                     float32, that run's worst |err| / mag_i against fp64, times 8 (hardware exp / reciprocal / square
                     root of ~1 ulp in place of correctly rounded ones, another summation order).  No kernel output is
                     in it.  A case whose allowance exceeds 1e-4 is badly conditioned and fails before any kernel is
                     judged.  The 2^-126 floor applies as above.
  scalars            rstd within 1e-6 relative of fp64, nll within 1e-6 max(1, |ref|), `correct` equal to the argmax
                     (first maximum wins).
"""
import numpy as np

from oracle import llama_ops_ref as R
from oracle.attention_ref import round_bf16, to_bf16_bits

FLOOR = 2.0 ** -126
BF16_TOL = 2.0 ** -7
GEMV_F32_TOL = 64 * 2.0 ** -24
F32_FACTOR = 8.0
F32_CAP = 1e-4
LOG2E = np.float32(1.4426950408889634)
BF16_MAX = float(np.float32(3.3895313892515355e38))

FIGURES = {}      # "<backend> <flavour> <case>.<output>" -> dict(worst=, bound=, np32=): what a run measured, for the record


class VerdictError(AssertionError):
    pass


def _f64(a):
    return np.asarray(a, np.float64)


def worst_ratio(got, ref, mag):
    """max_i max(|got_i - ref_i| - 2^-126, 0) / mag_i (inf where mag_i is 0 and the error is not)"""
    got, ref, mag = _f64(got), _f64(ref), _f64(mag)
    if got.shape != ref.shape or mag.shape != ref.shape:
        raise VerdictError(f"shapes differ: got {got.shape}, ref {ref.shape}, mag {mag.shape}")
    if got.size == 0:
        return 0.0
    if not np.isfinite(got).all():
        return float("inf")
    excess = np.maximum(np.abs(got - ref) - FLOOR, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(excess > 0, excess / mag, 0.0)
    return float(ratio.max())


def check(name, got, ref, mag, tol, np32=None):
    w = worst_ratio(got, ref, mag)
    FIGURES[name] = dict(worst=w, bound=tol, np32=np32)
    extra = "" if np32 is None else f", numpy-f32 {np32:.3e}"
    print(f"{name}: worst |err| / mag = {w:.3e} (bound {tol:.3e}{extra})")
    if not w <= tol:
        raise VerdictError(f"{name}: worst |err| / mag = {w:.3e} > {tol:.3e}")


def f32_allowance(name, np32, ref, mag):
    """8 x the worst |err| / mag of the numpy-float32 evaluation of the same formulas"""
    fig = worst_ratio(np32, ref, mag)
    allow = F32_FACTOR * fig
    if not allow <= F32_CAP:
        raise VerdictError(f"{name}: the case is badly conditioned, numpy float32 itself errs by {fig:.3e} of mag: rebuild it")
    return fig, allow


class Verdict:
    """verdict of one backend ("emu" / "gpu") and flavour; v(case.output, got, ref, mag, np32=the numpy-f32 evaluation)"""

    def __init__(self, backend, f32):
        self.tag, self.f32 = f"{backend} {'f32' if f32 else 'bf16'}", f32

    def __call__(self, name, got, ref, mag, np32=None):
        name = f"{self.tag} {name}"
        if not self.f32:
            return check(name, got, ref, mag, BF16_TOL)
        fig, allow = f32_allowance(name, np32, ref, mag)
        check(name, got, ref, mag, allow, np32=fig)

    def gemv_f32(self, name, got, ref, mag):
        check(f"{self.tag} {name}", got, ref, mag, GEMV_F32_TOL)


def _ord(x):
    b = to_bf16_bits(np.asarray(x, np.float32)).astype(np.int32)
    return np.where(b & 0x8000, -(b & 0x7fff), b)


def check_twice_rounded(name, got, inner, outer, share=5e-3):
    """An output that rounds twice, bf16(outer(bf16(inner))), against the rounding-faithful oracle.  `inner` is the oracle's
    value BEFORE the first rounding.  The f32 evaluation may land the first rounding on the neighbouring bf16 value where
    `inner` lies next to a tie, and no more than that: every element must equal outer(c) for c the oracle's first
    rounding or one of its two bf16 neighbours, and fewer than `share` of the elements may differ from the oracle's own
    at all.  (One ulp of the FIRST rounding is up to 2^-7 relative, which is up to two ulps of the result where the
    product's mantissa is near 2: "one ulp of the result" is not a bound this arithmetic can keep.)"""
    from oracle.attention_ref import from_bf16_bits
    got = np.asarray(got, np.float32)
    assert np.isfinite(got).all(), f"{name}: non-finite output"
    b = to_bf16_bits(round_bf16(np.asarray(inner, np.float32))).astype(np.uint16)
    zero = (b & 0x7fff) == 0
    cands = [b, np.where(zero, b, b + 1).astype(np.uint16), np.where(zero, b, b - 1).astype(np.uint16)]
    outs = [to_bf16_bits(np.asarray(outer(from_bf16_bits(c)), np.float32)) for c in cands]
    gb = to_bf16_bits(got)
    hit = (gb == outs[0]) | (gb == outs[1]) | (gb == outs[2]) | ((got == 0) & (outs[0] & 0x7fff == 0))
    frac = float((gb != outs[0]).mean()) if gb.size else 0.0
    FIGURES[name] = dict(worst=float((~hit).sum()), bound=0.0, share=frac)
    print(f"{name}: elements no first-rounding neighbour explains = {int((~hit).sum())}, share differing from the faithful "
          f"oracle = {frac:.2e} (< {share})")
    if gb.size and ((~hit).any() or not frac < share):
        raise VerdictError(f"{name}: {int((~hit).sum())} unexplained elements, share {frac:.3e}")


def check_rel(name, got, ref, tol, floor=0.0):
    got, ref = _f64(got), _f64(ref)
    assert got.shape == ref.shape and np.isfinite(got).all(), f"{name}: shape or non-finite"
    w = float((np.abs(got - ref) / np.maximum(np.abs(ref), floor)).max()) if got.size else 0.0
    FIGURES[name] = dict(worst=w, bound=tol, np32=None)
    print(f"{name}: worst relative error = {w:.3e} (bound {tol:.1e})")
    if not w <= tol:
        raise VerdictError(f"{name}: {w:.3e} > {tol:.1e}")


def _rng(seed):
    return np.random.default_rng(seed)


def _prep(f32, *ts):
    """bf16 flavours round the operands first"""
    return tuple(np.asarray(t, np.float32) if f32 else round_bf16(np.asarray(t, np.float32)) for t in ts)


# ================================================================ RoPE
def rope_table(D, max_pos, theta):
    """the product's host table (lwm_amd.llama_ops.precompute_freqs_cis) restated: f32 (max_pos, D/2, 2) = (cos, sin)"""
    fc = R.precompute_freqs_cis(D, max_pos, theta)
    return np.ascontiguousarray(np.stack((fc.real, fc.imag), axis=-1).astype(np.float32))


class RopeCase:
    def __init__(self, D, theta, max_pos, seed, broadcast=False):
        self.name = f"rope_D{D}_theta{theta:g}_pos{max_pos}{'_bcast' if broadcast else ''}"
        self.D, self.theta, self.max_pos, self.broadcast = D, theta, max_pos, broadcast
        self.B, self.S, self.H = 2, 37, 3
        g = _rng(seed)
        self._x = g.standard_normal((self.B, self.S, self.H, D)).astype(np.float32)
        pos = g.integers(0, max_pos, (1 if broadcast else self.B, self.S)).astype(np.int32)
        pos[0, 0], pos[0, 1] = 0, max_pos - 1                 # both ends of the table planted
        self.pos_arg = pos                                    # what the Python surface is handed: (1, S) or (B, S)
        self.pos = np.ascontiguousarray(np.broadcast_to(pos, (self.B, self.S)))
        self._tab = None

    @property
    def table(self):
        if self._tab is None:
            self._tab = rope_table(self.D, self.max_pos, self.theta)
        return self._tab

    def x(self, f32):
        return _prep(f32, self._x)[0]

    def __repr__(self):
        return self.name


def rope_cases():
    return [RopeCase(8, 5e7, 1 << 20, 11), RopeCase(64, 1e4, 4096, 12), RopeCase(128, 5e7, 1 << 16, 13),
            RopeCase(128, 1e4, 4096, 14, broadcast=True), RopeCase(8, 1e4, 64, 15, broadcast=True)]


def _rope_terms(x, table, pos, conj, dt):
    x = np.asarray(x, dt)
    cs = table[pos].astype(dt)                                # (B,S,D/2,2)
    c, s = cs[:, :, None, :, 0], cs[:, :, None, :, 1]
    if conj:
        s = -s
    xr = x.reshape(x.shape[:-1] + (-1, 2))
    return xr[..., 0], xr[..., 1], c, s


def rope_ref(x, table, pos, conj=False):
    """-> (ref, mag) float64"""
    x0, x1, c, s = _rope_terms(x, table, pos, conj, np.float64)
    ref = np.stack((x0 * c - x1 * s, x0 * s + x1 * c), axis=-1).reshape(x.shape)
    mag = np.stack((np.abs(x0 * c) + np.abs(x1 * s), np.abs(x0 * s) + np.abs(x1 * c)), axis=-1).reshape(x.shape)
    return ref, mag


def rope_np32(x, table, pos, conj=False):
    x0, x1, c, s = _rope_terms(x, table, pos, conj, np.float32)
    return np.stack((x0 * c - x1 * s, x0 * s + x1 * c), axis=-1).reshape(x.shape)


def verify_rope(case, got, conj, v, x=None):
    x = case.x(v.f32) if x is None else x
    ref, mag = rope_ref(x, case.table, case.pos, conj)
    v(f"{case.name}.{'conj' if conj else 'fwd'}", got, ref, mag, np32=rope_np32(x, case.table, case.pos, conj))


# ================================================================ RMSNorm
EPS = 1e-6


class RmsCase:
    def __init__(self, rows, C, seed, fwd_only=False):
        self.name, self.rows, self.C, self.fwd_only = f"rms_{rows}x{C}", rows, C, fwd_only
        g = _rng(seed)
        x = (g.standard_normal((rows, C)) * 2).astype(np.float32)
        if rows >= 7:
            x[1] = 0.0                    # r = eps^-1/2
            x[2] *= 1e15
            x[3] *= 1e-15
        self._x = x
        self._w = (g.standard_normal(C) * 3 + 0.5).astype(np.float32)         # far from 1, both signs
        # (the upstream gradient leans towards x w: mean(dy xhat) keeps a definite part, it does not sit where chance
        # cancelled it -- there float32 itself loses the projection term, numpy float32 5.8e-5 of mag at 300 x 264)
        self._g = (g.standard_normal((rows, C)) + 0.25 * np.sign(x * self._w)).astype(np.float32)
        self._res = g.standard_normal((rows, C)).astype(np.float32)

    def ops(self, f32):
        """(x, w, g, res)"""
        return _prep(f32, self._x, self._w, self._g, self._res)

    def __repr__(self):
        return self.name


def rms_shapes(f32, device=False):
    """(rows, C, fwd_only).  C: one vector, a partial first slot, a partial second slot, all four slots full (f32: C % 4)"""
    Cs = (8, 264, 2056, 8192) + ((4, 1000) if f32 else ())
    out = [(rows, C, False) for C in Cs for rows in (1, 7, 300)]
    out.append((2049, 64, False))                 # the second trip of the backward's grid-stride loop; dW: main loop + tail
    if device:                                    # (a fiber per lane: 65539 workgroups cost the host emulator minutes)
        out.append((65539, 8, True))              # past the forward's grid cap
    return out


def rms_case(rows, C, fwd_only=False):
    return RmsCase(rows, C, 1000 + 7 * C + rows, fwd_only)


def rms_ref(x, w, g):
    """float64: dict of (ref, mag) pairs + rstd"""
    x, w, g = _f64(x), _f64(w), _f64(g)
    C = x.shape[-1]
    r = 1.0 / np.sqrt(np.mean(x * x, axis=-1, keepdims=True) + EPS)
    xh = x * r
    dy = g * w
    mean = np.sum(dy * xh, axis=-1, keepdims=True) / C
    return dict(rstd=r[:, 0], y=(xh * w, np.abs(xh * w)), dx=(r * (dy - xh * mean), r * (np.abs(dy) + np.abs(xh * mean))),
                dw=((g * xh).sum(0), np.abs(g * xh).sum(0)))


def rms_np32(x, w, g):
    x, w, g = (np.asarray(t, np.float32) for t in (x, w, g))
    C = np.float32(x.shape[-1])
    r = (np.float32(1) / np.sqrt(np.sum(x * x, axis=-1, keepdims=True, dtype=np.float32) / C + np.float32(EPS))).astype(np.float32)
    xh = x * r
    dy = g * w
    mean = np.sum(dy * xh, axis=-1, keepdims=True, dtype=np.float32) / C
    return dict(y=xh * w, dx=r * (dy - xh * mean), dw=np.sum(g * xh, axis=0, dtype=np.float32))


def verify_rms(case, got, v):
    """got: dict(y, rstd[, dx, dw[, dx_res, dw_res]]) float arrays"""
    x, w, g, res = case.ops(v.f32)
    ref = rms_ref(x, w, g)
    n32 = rms_np32(x, w, g) if v.f32 else {}
    check_rel(f"{v.tag} {case.name}.rstd", got["rstd"], ref["rstd"], 1e-6)
    if v.f32:
        v(f"{case.name}.y", got["y"], *ref["y"], np32=n32["y"])
    else:
        # lwm/llama.py:339-341: bf16(bf16(x r) w)
        check_twice_rounded(f"{v.tag} {case.name}.y", got["y"], (_f64(x) * ref["rstd"][:, None]).astype(np.float32),
                            lambda y0: round_bf16(y0 * w))
    if case.fwd_only:
        return
    v(f"{case.name}.dx", got["dx"], *ref["dx"], np32=n32.get("dx"))
    v(f"{case.name}.dw", got["dw"], *ref["dw"], np32=n32.get("dw"))
    if "dx_res" in got:
        # the folded residual rounds twice: bf16(bf16(dx) + res), the roundings of autograd's separate bf16 add
        check_twice_rounded(f"{v.tag} {case.name}.dx_res", got["dx_res"], ref["dx"][0].astype(np.float32),
                            lambda d0: round_bf16(d0 + res))
        assert np.array_equal(np.asarray(got["dw_res"], np.float32), np.asarray(got["dw"], np.float32)), \
            f"{case.name}: dw changes with the residual"


# ================================================================ SwiGLU
SWIGLU_SPECIALS = (0.0, 20.0, 30.0, 50.0, 88.0, 100.0, 1e4, 1e-20)


class SwigluCase:
    def __init__(self, n, seed, name=None, shape=None):
        self.name, self.n, self.shape = name or f"swiglu_n{n}", n, shape or (n,)
        g = _rng(seed)
        a = (g.standard_normal(n) * 2).astype(np.float32)
        sp = np.array([s * v for v in SWIGLU_SPECIALS for s in (1.0, -1.0)], np.float32)       # +-0 included
        if n >= sp.size:
            a[g.choice(n, sp.size, replace=False)] = sp
        else:                                   # the smallest case: specials only, as many as fit (n = 8: +-20, +-88, +-1e4, +-1e-20)
            a[:] = np.array([20, -20, 88, -88, 1e4, -1e4, 1e-20, -1e-20], np.float32)[:n]
        self._a = a
        self._b = (g.standard_normal(n) * 2).astype(np.float32)
        self._g = g.standard_normal(n).astype(np.float32)

    def ops(self, f32):
        """(a, b, g)"""
        return tuple(t.reshape(self.shape) for t in _prep(f32, self._a, self._b, self._g))

    def __repr__(self):
        return self.name


def swiglu_cases():
    # the second small case carries the specials that do not fit into eight elements
    return [SwigluCase(8, 41), SwigluCase(64, 42), SwigluCase(8 * 4001, 43)]


def swiglu_halves_cases():
    return [SwigluCase(rows * F, 50 + rows + F, name=f"swiglu_halves_{rows}x{F}", shape=(rows, F)) for rows in (1, 5) for F in (8, 1376)]


def swiglu_ref(a, b, g):
    a, b, g = _f64(a), _f64(b), _f64(g)
    with np.errstate(over="ignore"):
        sg = 1.0 / (1.0 + np.exp(-a))
    y = a * sg * b
    t1, t2 = g * b * sg, g * b * sg * a * (1.0 - sg)
    db = g * a * sg
    return dict(y=(y, np.abs(y)), da=(t1 + t2, np.abs(t1) + np.abs(t2)), db=(db, np.abs(db)))


def swiglu_np32(a, b, g):
    a, b, g = (np.asarray(t, np.float32) for t in (a, b, g))
    one = np.float32(1)
    with np.errstate(over="ignore", under="ignore"):
        sg = one / (one + np.exp2(-a * LOG2E))            # (the kernels' sigmoid: the product rounds at ulp(|a| log2 e))
        return dict(y=a * sg * b, da=g * b * sg * (one + a * (one - sg)), db=g * a * sg)


def verify_swiglu(case, got, v):
    """got: dict(y, da, db)"""
    a, b, g = case.ops(v.f32)
    ref = swiglu_ref(a, b, g)
    n32 = swiglu_np32(a, b, g) if v.f32 else {}
    for n in ("y", "da", "db"):
        assert not np.isnan(np.asarray(got[n])).any(), f"{case.name}: NaN in {n}"
        v(f"{case.name}.{n}", got[n], *ref[n], np32=n32.get(n))


# ================================================================ softmax cross entropy
class CeCase:
    def __init__(self, name, logits, target, weight):
        self.name, self._l, self.target, self.weight = name, logits, np.asarray(target, np.int32), np.asarray(weight, np.float32)

    def logits(self, f32):
        return _prep(f32, self._l)[0]

    def __repr__(self):
        return self.name


CE_WEIGHTS = (1.0, 0.5, 1.0 / 3.0, 0.0, 1e-3, 1.0)


def _ce_plain(V, seed):
    """six rows: targets at 0, at V - 1, on an odd column and at the argmax; weights {1, 1/2, 1/3, 0, 1e-3}; scales 3 and 10"""
    g = _rng(seed)
    x = g.standard_normal((6, V)).astype(np.float32) * np.array([3, 10, 3, 10, 3, 10], np.float32)[:, None]
    odd = (int(g.integers(0, V // 2)) * 2 + 1) % V
    t = [0, V - 1, odd, int(g.integers(0, V)), 0, 0]
    for r in (4, 5):
        t[r] = int(round_bf16(x[r]).argmax())
    return CeCase(f"ce_V{V}", x, t, CE_WEIGHTS)


def _ce_special(V, seed, f32):
    """an all-equal row; an argmax tie in two threads and in two waves of the kernel (the lower index wins); a row with the
    largest and the most negative finite bf16"""
    g = _rng(seed)
    x = (g.standard_normal((6, V)) * 3).astype(np.float32)
    vw = 4 if f32 else 8                                      # columns per thread and vector slot
    TIE = 16.0                                                # above every N(0, 9) draw (max ~ 13), near enough to leave the other p_i a say
    t = [0] * 6
    x[0] = 1.5                                                # uniform p, argmax 0
    lo, hi = vw * 1 + 1, vw * 5 + 2                           # two threads of wave 0
    if hi >= V:
        lo, hi = 1, V - 2                                     # (a row of one vector: one thread)
    x[1, [lo, hi]] = TIE
    t[1] = lo                                                 # correct
    x[2, [lo, hi]] = TIE
    t[2] = hi                                                 # the later maximum is NOT the argmax
    wl, wh = vw * 3 + 1, vw * 64 + vw // 2                    # thread 3 of wave 0, thread 64 = wave 1
    if wh >= V:
        wl, wh = lo, hi
    x[3, [wl, wh]] = TIE
    t[3] = wl
    c = g.choice(V, 3, replace=False)
    x[4, c[0]], x[4, c[1]] = BF16_MAX, -BF16_MAX
    t[4] = int(c[2])
    t[5] = int(g.integers(0, V))
    return CeCase(f"ce_V{V}_special", x, t, (1.0, 0.5, 1.0 / 3.0, 1e-3, 1.0, 0.25))


def ce_names(f32, device=False):
    Vs = ((4,) if f32 else ()) + (8, 520, 8448, 32000, 32768)
    return [f"ce_V{V}{sfx}" for V in Vs for sfx in ("", "_special")] + (["ce_65539x8"] if device else [])


def ce_case(name, f32):
    if name == "ce_65539x8":                      # past the grid cap: three rows ride a second trip
        g, rows = _rng(77), 65539
        return CeCase(name, (g.standard_normal((rows, 8)) * 3).astype(np.float32), g.integers(0, 8, rows),
                      np.resize(np.array(CE_WEIGHTS[:5], np.float32), rows))
    V = int(name.split("_")[1][1:])
    return _ce_special(V, 700 + V, f32) if name.endswith("_special") else _ce_plain(V, 600 + V)


def ce_ref(logits, target, weight):
    x, w = _f64(logits), _f64(weight)
    rows, V = x.shape
    m = x.max(axis=-1, keepdims=True)
    with np.errstate(under="ignore"):
        e = np.exp(x - m)
    tot = e.sum(-1, keepdims=True)
    p = e / tot
    onehot = np.zeros_like(p)
    onehot[np.arange(rows), target] = 1.0
    nll = (m[:, 0] + np.log(tot[:, 0])) - x[np.arange(rows), target]
    return dict(nll=nll, correct=(x.argmax(-1) == target).astype(np.int32), dl=((p - onehot) * w[:, None], (p + onehot) * w[:, None]))


def ce_np32(logits, target, weight):
    x, w = np.asarray(logits, np.float32), np.asarray(weight, np.float32)
    rows = x.shape[0]
    with np.errstate(under="ignore", over="ignore"):
        e = np.exp2((x - x.max(axis=-1, keepdims=True)) * LOG2E)
        tot = np.sum(e, axis=-1, keepdims=True, dtype=np.float32)
        dl = e * (w[:, None] / tot)
    dl[np.arange(rows), target] -= w
    return dl


def verify_ce(case, got, v):
    """got: (nll, correct, dl)"""
    x = case.logits(v.f32)
    ref = ce_ref(x, case.target, case.weight)
    nll, cor, dl = got
    check_rel(f"{v.tag} {case.name}.nll", nll, ref["nll"], 1e-6, floor=1.0)
    assert np.array_equal(np.asarray(cor, np.int32), ref["correct"]), f"{case.name}: `correct` differs from the oracle's argmax"
    v(f"{case.name}.dlogits", dl, *ref["dl"], np32=ce_np32(x, case.target, case.weight) if v.f32 else None)
    dead = case.weight == 0
    assert not np.asarray(dl)[dead].any(), f"{case.name}: a row of weight 0 must get an exact 0 gradient"


def ce_public_case(V, seed, poison=None):
    """(logits (2,3,V) f32, tokens, valid) for the public entry points; poison = a value planted into the logits of the one
    row with valid == 0"""
    g = _rng(seed)
    x = (g.standard_normal((2, 3, V)) * 3).astype(np.float32)
    tok = g.integers(0, V, (2, 3))
    tok[0, 0] = int(round_bf16(x[0, 0]).argmax())
    valid = np.array([[1, 1, 0], [1, 1, 1]], np.float32)
    if poison is not None:
        x[0, 2, :: 3] = poison
    return x, tok, valid


POISONS = (float("nan"), float("inf"), float("-inf"))


# ================================================================ GEMV
GEMV_SHAPES = [(1, 32, 8), (2, 96, 40), (4, 160, 1032), (3, 12288, 520), (2, 4128, 264)]


def gemv_ops(rows, K, N, seed=0):
    g = _rng(900 + rows + K + N + seed)
    return round_bf16(g.standard_normal((rows, K)).astype(np.float32)), round_bf16((g.standard_normal((K, N)) * 0.1).astype(np.float32))


def gemv_ref(x, w):
    x, w = _f64(x), _f64(w)
    return x @ w, np.abs(x) @ np.abs(w)


def verify_gemv(name, y_bf16, y_f32, x, w, v):
    ref, mag = gemv_ref(x, w)
    v.gemv_f32(f"{name}.y_f32", y_f32, ref, mag)
    assert np.array_equal(to_bf16_bits(np.asarray(y_bf16, np.float32)), to_bf16_bits(round_bf16(np.asarray(y_f32, np.float32)))), \
        f"{name}: the bf16 output is not the rounded f32 output"


# ================================================================ mutants: the verdict must fail a reference with one term damaged
def mutants():
    """-> [(name, got (a damaged float64 reference), ref, mag, old-style max-norm figure and bound)]: numpy arrays only, no
    kernel is made to misbehave.  Each on the smallest case of its operator."""
    out = []
    # CE: the softmax term zeroed on one aligned group of 8 columns
    c = _ce_plain(8, 608)
    x = c.logits(False)
    ref, mag = ce_ref(x, c.target, c.weight)["dl"]
    bad = ref.copy()
    onehot = np.zeros_like(ref)
    onehot[np.arange(6), c.target] = 1.0
    bad[0, 0:8] = (-onehot * _f64(c.weight)[:, None])[0, 0:8]
    out.append(("ce_dlogits_softmax_term_zeroed_on_8_columns", bad, ref, mag, 2.0 ** -7))
    # RMSNorm: dx without the projection term; dW with one row's contribution missing
    rc = rms_case(7, 8)
    x, w, g, _ = rc.ops(False)
    rr = rms_ref(x, w, g)
    x64, w64, g64 = _f64(x), _f64(w), _f64(g)
    out.append(("rmsnorm_dx_without_projection", rr["rstd"][:, None] * g64 * w64, *rr["dx"], 1e-2))
    out.append(("rmsnorm_dw_one_row_missing", rr["dw"][0] - g64[0] * x64[0] * rr["rstd"][0], *rr["dw"], 1e-2))
    # SwiGLU: da without the a (1 - sigma) term
    sc = SwigluCase(8, 41)
    a, b, g = sc.ops(False)
    sr = swiglu_ref(a, b, g)
    with np.errstate(over="ignore"):
        sg = 1.0 / (1.0 + np.exp(-_f64(a)))
    out.append(("swiglu_da_without_a_one_minus_sigma", _f64(g) * _f64(b) * sg, *sr["da"], 2.0 ** -6))
    # RoPE: the sine's sign flipped on one pair
    pc = RopeCase(8, 1e4, 64, 15, broadcast=True)
    xr = pc.x(False)
    ref, mag = rope_ref(xr, pc.table, pc.pos)
    flipped, _ = rope_ref(xr, pc.table, pc.pos, conj=True)
    bad = ref.copy()
    bad[1, 5, 2, 2:4] = flipped[1, 5, 2, 2:4]
    out.append(("rope_sine_sign_flipped_on_one_pair", bad, ref, mag, 2.0 ** -7))
    # GEMV: the last row of W left out
    xg, wg = gemv_ops(1, 32, 8)
    ref, mag = gemv_ref(xg, wg)
    out.append(("gemv_last_row_of_W_left_out", _f64(xg[:, :-1]) @ _f64(wg[:-1]), ref, mag, 2e-6 * np.sqrt(32)))
    return out


def max_norm(got, ref):
    return float(np.abs(_f64(got) - ref).max() / max(np.abs(ref).max(), 1e-30))
