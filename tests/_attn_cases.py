"""Attention at the inputs the rest of the suite does not feed it: case builders and the shared verdict, run twice --
on the host emulator (tests/test_emu_attn_edges.py) and on the device (tests/test_gpu_attn_edges.py).
TEST INFRASTRUCTURE ONLY.

A Case holds float32 operands (the bf16 flavour rounds them, the f32 flavour takes them as they are), the mask /
offset / scale keywords that the kernels and the fp64 oracle (oracle/attention_ref.py) both take, and the number of
query rows with no visible key the case is built to produce (checked on the oracle's mask: a case that lost its point
fails before any kernel is judged).

Bounds are the project's own, per flavour and backend (tests/_parity.py; TOL of tests/test_gpu_f32.py; the 1e-2 / 1e-4 of
tests/test_emu_kernels.py; the 1e-5 of tests/test_emu_attn_f32.py)."""
import numpy as np

from oracle import attention_ref as R
from tests import _kv8_ref as K8, _parity

D = 128


class Bounds:
    def __init__(self, name, tol, lse_tol, parity=False):
        self.name, self.tol, self.lse_tol, self.parity = name, tol, lse_tol, parity

    @staticmethod
    def rel(got, ref):
        return float(np.abs(np.asarray(got, np.float64) - ref).max() / max(np.abs(ref).max(), 1e-30))

    def check(self, name, got, ref, row_tol=_parity.ROW_TOL):
        print(f"[{self.name}] {name}: max|err| / max|ref| = {self.rel(got, ref):.3e} (bound {self.tol})")
        if self.parity:
            _parity.check(name, got, ref, row_tol=row_tol)
        else:
            assert self.rel(got, ref) < self.tol, f"{name}: {self.rel(got, ref):.3e} >= {self.tol}"

    def check_dq(self, name, got, dq_saved, dq_exact):
        print(f"[{self.name}] {name}: max|err| / max|ref| = {self.rel(got, dq_exact):.3e} (bound {self.tol})")
        if self.parity:
            _parity.check_dq(name, got, dq_saved, dq_exact)
        else:
            assert self.rel(got, dq_exact) < self.tol, f"{name}: {self.rel(got, dq_exact):.3e} >= {self.tol}"

    def check_lse(self, name, got, ref):
        fin = np.isfinite(ref)
        assert np.array_equal(np.isfinite(got), fin), f"{name}: isfinite(lse) differs from the oracle's"
        assert not np.isnan(got).any(), f"{name}: NaN in lse"
        err = float(np.abs(got[fin] - ref[fin]).max()) if fin.any() else 0.0
        print(f"[{self.name}] {name}: max|lse err| = {err:.3e} (bound {self.lse_tol}), max|lse| = "
              f"{float(np.abs(ref[fin]).max()) if fin.any() else 0.0:.1f}")
        assert err <= self.lse_tol if self.parity else err < self.lse_tol, f"{name}: lse error {err:.3e} > {self.lse_tol}"


EMU_BF16 = Bounds("emu bf16", 1e-2, 1e-4)
EMU_F32 = Bounds("emu f32", 1e-5, 1e-5)
GPU_BF16 = Bounds("gpu bf16", _parity.TOL, 2e-3, parity=True)
GPU_F32 = Bounds("gpu f32", 1e-5, 1e-5)


class Case:
    def __init__(self, name, q, k, v, do, kw, empty_rows=None, scale_guard=False, min_abs_lse=None):
        self.name, self.kw, self.empty_rows, self.scale_guard, self.min_abs_lse = name, kw, empty_rows, scale_guard, min_abs_lse
        self._ops = (q, k, v, do)

    def operands(self, f32):
        """(q, k, v, dout) float32: as they are for the f32 flavour, rounded to bf16 values for the bf16 one"""
        return self._ops if f32 else tuple(R.round_bf16(t) for t in self._ops)

    @property
    def has_segments(self):
        return self.kw.get("seg_q") is not None

    def __repr__(self):
        return self.name


def _rnd(shape, seed, mag=1.0):
    return (np.random.default_rng(seed).standard_normal(shape) * mag).astype(np.float32)


def _qkvdo(B, Sq, Sk, H, seed, qk_mag=1.0):
    return (_rnd((B, Sq, H, D), seed, qk_mag), _rnd((B, Sk, H, D), seed + 1, qk_mag), _rnd((B, Sk, H, D), seed + 2),
            _rnd((B, Sq, H, D), seed + 3))


def _sparse_valid(B, Sk, seed, p=0.1):
    kv = (np.random.default_rng(seed).random((B, Sk)) > p).astype(np.uint8)
    kv[:, 0] = 1
    return kv


# ---------------------------------------------------------------- B1: scale
SCALES = (0.01, 0.25, 0.5)


def scale_cases():
    """plain = the kernels without key meta (no mask source but causality, Sk a multiple of every key tile); meta = the
    `_meta` variants (csrc/api.inc: a key_valid pointer selects them in the forward, dQ and dK/dV alike)"""
    out = []
    for s in SCALES:
        B, S, H = 1, 256, 2
        out.append(Case(f"scale{s}_plain", *_qkvdo(B, S, S, H, 100), dict(causal=True, scale=s), empty_rows=0, scale_guard=True))
        out.append(Case(f"scale{s}_meta", *_qkvdo(B, 192, 320, H, 110),
                        dict(causal=True, q_start=128, key_valid=_sparse_valid(B, 320, 7), scale=s), empty_rows=0, scale_guard=True))
    return out


def infer_case(scale, Sq, seed=120):
    """dense-mask inference operands: (q, k, v bf16 values, mask u8 (B,Sq,Sk), scale) -- Sq = 1 is the decode kernel"""
    B, Sk, H = 2, 300, 2
    q, k, v, _ = (R.round_bf16(t) for t in _qkvdo(B, Sq, Sk, H, seed))
    rng = np.random.default_rng(seed + 9)
    mask = (rng.random((B, Sq, Sk)) > 0.1).astype(np.uint8)
    mask[:, :, 270:] = 0                         # the empty tail of a cache
    mask[:, :, 5] = 1
    return q, k, v, mask, scale


# ---------------------------------------------------------------- B3: mask structure
def _segments(B, S, cuts=None, runs=None):
    s = np.zeros((B, S), np.int32)
    if cuts is not None:
        for c in cuts:
            s[:, c:] += 1
    else:
        s[:] = np.repeat(np.asarray(runs[0], np.int32), runs[1])[None]
    return s


def mask_cases():
    out = []
    # (a) whole tiles of invalid keys at the head of the sequence: the running max stays -inf across tiles
    B, S, H = 2, 768, 2
    kv = np.ones((B, S), np.uint8)
    kv[0, :300] = 0
    kv[1, :256] = 0
    out.append(Case("b3a_left_pad", *_qkvdo(B, S, S, H, 200), dict(causal=True, key_valid=kv), empty_rows=1112))
    # (b) non-causal, holes that cover whole tiles
    B, Sq, Sk, H = 1, 200, 768, 2
    kv = np.ones((B, Sk), np.uint8)
    kv[:, :128] = 0
    kv[:, 384:640] = 0
    out.append(Case("b3b_holes", *_qkvdo(B, Sq, Sk, H, 210), dict(causal=False, key_valid=kv), empty_rows=0))
    # (c) segment cuts on tile boundaries and one past them
    B, S, H = 1, 768, 2
    seg = _segments(B, S, cuts=(64, 128, 129, 255, 256, 512, 513))
    out.append(Case("b3c_cuts", *_qkvdo(B, S, S, H, 220), dict(causal=True, seg_q=seg, seg_k=seg), empty_rows=0))
    # (d) a ring step: queries 512.. of a 1024-token row against keys 0..511; the document that starts at 700 has no key here
    B, S, H = 1, 512, 2
    full = _segments(B, 1024, cuts=(300, 700))
    out.append(Case("b3d_ring_step", *_qkvdo(B, S, S, H, 230),
                    dict(causal=True, q_start=512, k_start=0, seg_q=full[:, 512:].copy(), seg_k=full[:, :512].copy()), empty_rows=648))
    # (e) non-monotone segment ids together with key_valid
    B, S, H = 1, 768, 2
    seg = _segments(B, S, runs=([3, 1, 3, 2, 1, 0], 128))
    kv = np.ones((B, S), np.uint8)
    kv[:, 96:160] = 0
    kv[:, 700:768] = 0
    out.append(Case("b3e_non_monotone", *_qkvdo(B, S, S, H, 240), dict(causal=True, seg_q=seg, seg_k=seg, key_valid=kv), empty_rows=64))
    return out


# ---------------------------------------------------------------- B4: large logits
def large_logit_cases():
    """q and k scaled by 3 and by 6: |score| reaches tens and beyond a hundred, the softmax is next to one-hot.  Causal
    with position offsets that are no multiple of a tile; plain and `_meta` kernels."""
    out = []
    for f, lo in ((3, 25.0), (6, 100.0)):
        B, Sq, Sk, H = 1, 192, 256, 2
        out.append(Case(f"logits_x{f}_plain", *_qkvdo(B, Sq, Sk, H, 300, f), dict(causal=True, q_start=165, k_start=37),
                        empty_rows=0, min_abs_lse=lo))
        out.append(Case(f"logits_x{f}_meta", *_qkvdo(B, Sq, 290, H, 310, f),
                        dict(causal=True, q_start=165, k_start=37, key_valid=_sparse_valid(B, 290, 9)), empty_rows=0, min_abs_lse=lo))
    return out


# ---------------------------------------------------------------- the verdict
def _row_rel(got, ref):
    """the per-row figure of tests/_parity.py::check"""
    gmax = max(np.abs(ref).max(), 1e-9)
    return float((np.abs(got - ref).max(axis=-1) / np.maximum(np.abs(ref).max(axis=-1), _parity.ROW_FLOOR * gmax)).max())


def contract_dk(case):
    """dk of the fp64 oracle under the arithmetic CONTRACT of the bf16 backward, nothing of the kernels' in it: delta =
    rowsum(dO * O) from the output as it is saved (the oracle's own, rounded to bf16 -- the reference saves `out` cast to
    v.dtype too), dS = P (dP - delta) scale rounded to bf16 where the kernels round it for the
    dS^T Q product; everything else in fp64."""
    q, k, v, do = (t.astype(np.float64) for t in case.operands(False))
    kw = dict(case.kw)
    scale = kw.pop("scale", None) or 1.0 / np.sqrt(D)
    B, Sq = q.shape[:2]
    ro, rl = R.dense_attention(q, k, v, scale=scale, **kw)
    vis = R.visible_mask(Sq, k.shape[1], B=B, **kw)[:, None]
    fin = np.isfinite(rl)[..., None]
    p = np.where(vis & fin, np.exp(np.where(vis, R._scores(q, k) * scale, 0.0) - np.where(fin, rl[..., None], 0.0)), 0.0)
    delta = np.einsum("bqhd,bqhd->bhq", do, R.round_bf16(ro).astype(np.float64))[..., None]
    ds = R.round_bf16(p * (R._scores(do, v) - delta) * scale).astype(np.float64)
    return R._apply_t(ds, q)


def dk_row_bound(case, rk):
    """The per-row bound of dk.  tests/_parity.py explains why a dq row cannot be held to its own scale against the
    exact gradient: dS = P (dP - delta) cancels almost completely where the softmax is next to one-hot, and what is left
    is the bf16 rounding of the SAVED output inside delta.  dK = dS^T Q carries the same residual into the rows of keys
    that few queries attend -- unnoticed at unit-variance inputs and the default scale, the whole row error at scale 0.5
    or at logits scaled by 3 and 6 (reference-side figures 0.07 .. 0.35 of the row's own scale, against 0.003 .. 0.008
    without the rounding of the saved output; the emulated kernels land on the same figures to two or three digits).
    Where the contract alone (contract_dk: the fp64 oracle, no kernel output) misses the project's 2.5e-2, the case's
    row bound is TWICE that reference-side figure; everywhere else it is the project's.  The global bound and the
    cosine stay the project's in every case."""
    fig = _row_rel(contract_dk(case), rk)
    print(f"{case.name}.dk: reference-side row figure of the arithmetic contract = {fig:.3e}")
    return 2 * fig if fig > _parity.ROW_TOL else _parity.ROW_TOL


def visibility(case, Sq, Sk, B):
    kw = {k: v for k, v in case.kw.items() if k != "scale"}
    return R.visible_mask(Sq, Sk, B=B, **kw)


def verify(case, got, bounds, f32):
    """got: dict(out, lse, dq, dk, dv) of float arrays from the kernels under test"""
    q, k, v, do = case.operands(f32)
    B, Sq, H, _ = q.shape
    Sk = k.shape[1]
    vis = visibility(case, Sq, Sk, B)
    empty_q, dead_k = ~vis.any(axis=2), ~vis.any(axis=1)                # (B,Sq), (B,Sk)
    if case.empty_rows is not None:
        assert int(empty_q.sum()) * H == case.empty_rows, (case.name, int(empty_q.sum()) * H)
    for n, t in got.items():
        assert not np.isnan(t).any(), f"{case.name}: NaN in {n}"
    ro, rl = R.dense_attention(q, k, v, **case.kw)
    rq_saved, rk, rv, rq = R.dense_attention_bwd(q, k, v, do, out_saved=got["out"], **case.kw)
    if case.min_abs_lse is not None:
        assert np.abs(rl[np.isfinite(rl)]).max() > case.min_abs_lse, "the case no longer produces large logits"
    if case.scale_guard:
        # a case that cannot tell its scale from the default one tests nothing
        kw0 = dict(case.kw, scale=None)
        o0, _ = R.dense_attention(q, k, v, **kw0)
        g0 = R.dense_attention_bwd(q, k, v, do, **kw0)
        for n, a, b in (("out", ro, o0), ("dq", rq, g0[0]), ("dk", rk, g0[1]), ("dv", rv, g0[2])):
            assert Bounds.rel(a, b) > 10 * bounds.tol, f"{case.name}: {n} at this scale is within 10 x tol of the default scale's"
    bounds.check(f"{case.name}.out", got["out"], ro)
    bounds.check_lse(f"{case.name}.lse", got["lse"], rl)
    bounds.check_dq(f"{case.name}.dq", got["dq"], rq_saved, rq)
    bounds.check(f"{case.name}.dk", got["dk"], rk, **(dict(row_tol=dk_row_bound(case, rk)) if bounds.parity and not f32 else {}))
    bounds.check(f"{case.name}.dv", got["dv"], rv)
    # exact zeros: rows with no visible key, keys no query sees
    assert not got["out"][empty_q].any() and not got["dq"][empty_q].any(), f"{case.name}: rows with no visible key must be 0"
    assert np.isneginf(got["lse"].transpose(0, 2, 1)[empty_q]).all()
    assert not got["dk"][dead_k].any() and not got["dv"][dead_k].any(), f"{case.name}: keys masked for every query must get 0"


# ---------------------------------------------------------------- B2: strided operands with poisoned gaps
PAD = 8          # elements between the rows of neighbouring heads: every stride differs from the dense one
POISON = 0xFF    # every byte outside the views (as bf16 and as f32 that is a NaN)


def strided_cases():
    """B = 2, Sq != Sk; plain and `_meta` kernels"""
    B, Sq, Sk, H = 2, 128, 256, 2
    return [Case("strided_plain", *_qkvdo(B, Sq, Sk, H, 400), dict(causal=True, q_start=Sk - Sq), empty_rows=0),
            Case("strided_meta", *_qkvdo(B, Sq, Sk, H, 410), dict(causal=True, q_start=Sk - Sq, key_valid=_sparse_valid(B, Sk, 11)),
                 empty_rows=0)]


def slots_np(B, S, n, H, dtype):
    """-> (buf (B,S,n,H,D+PAD) of poison, [n views (B,S,H,D)]): slot i of one larger buffer, the layout _QKVRope hands
    q / k / v in, with a gap behind every head row on top"""
    from tests import _emu
    buf = _emu.aligned((B, S, n, H, D + PAD), dtype)
    buf.view(np.uint8)[...] = POISON
    return buf, [buf[:, :, i, :, :D] for i in range(n)]


def gaps_intact_np(buf):
    return bool((buf[..., D:].view(np.uint8) == POISON).all())


# ---------------------------------------------------------------- B5: FP8 decode with heterogeneous scales
def kv8_case(seed=500):
    """-> (q (B,1,H,128) bf16 values scaled by 0.5, K bytes, K scales, V bytes, V scales, mask (B,1,Sk), splits): rows whose
    power-of-two scales differ from row to row and head to head by up to 2^5 (K) and 2^23 (V)"""
    B, Sk, H, splits = 2, 200, 3, 3
    rng = np.random.default_rng(seed)
    q = R.round_bf16(_rnd((B, 1, H, D), seed + 1) * 0.5)
    k = R.round_bf16(_rnd((B, Sk, H, D), seed + 2, 1.5) * (2.0 ** rng.integers(-3, 3, (B, Sk, H, 1))).astype(np.float32))
    v = R.round_bf16(_rnd((B, Sk, H, D), seed + 3, 0.7) * (2.0 ** rng.integers(-12, 12, (B, Sk, H, 1))).astype(np.float32))
    kq, ks = K8.quantise(k)
    vq, vs = K8.quantise(v)
    mask = np.ones((B, 1, Sk), np.uint8)
    mask[:, :, 170:] = 0                      # a masked tail: the last piece sees a few keys only
    mask[0, :, :9] = 0
    return q, kq, ks, vq, vs, mask, splits


def kv8_reference(q, kq, ks, vq, vs, mask, scale=None, tol=2e-2):
    """the oracle on the DEQUANTISED cache (as test_decode_kv8_vs_oracle), and the guard: scales read one row or one head
    off move the oracle's output by more than ten times the tolerance"""
    ref = lambda ks_, vs_: R.dense_attention(q, K8.dequant(kq, ks_), K8.dequant(vq, vs_), causal=False, dense_mask=mask, scale=scale)
    ro, rl = ref(ks, vs)
    for axis in (1, 2):
        for which in ("k", "v"):
            o2, _ = ref(np.roll(ks, 1, axis) if which == "k" else ks, np.roll(vs, 1, axis) if which == "v" else vs)
            moved = np.abs(o2 - ro).max() / np.abs(ro).max()
            assert moved > 10 * tol, f"rolling the {which} scales along axis {axis} moves the oracle by {moved:.3e} only"
    return ro, rl
