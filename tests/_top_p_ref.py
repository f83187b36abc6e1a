"""fp64 restatement of the nucleus (top-p) filter of the token sampler (the rule of include/lwm_hip.h; the kernel is in
lwm_amd/csrc/sample.h), beside tests/_sample_ref.py, whose Philox / Gumbel / guidance pieces it uses: the reference the
emulated and the device kernel are held to.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

from tests._sample_ref import gumbel, mixed_logits, philox4x32_10
from tests._sample_ref import sample as _sample_without_top_p

# The relative band of the top-p threshold that the kernel's arithmetic is held to -- the one number the tests use.
# include/lwm_hip.h derives it: every weight within delta = 1.25 * 2^-22 of exp(s - max) (a 2-ulp f32 exponential of the
# rounded difference, corrected by the rounding's remainder in f64, kept as an f32), sums and the product top_p * Z in
# f64 (< 2^-33 for any V); M and Z each move by delta, so every entry outside 2 * delta = 0.625 * 2^-20 is decided as in
# exact arithmetic, and eps rounds that up to a power of two.
TOP_P_EPS = 2.0 ** -20


def top_k_keep(s, top_k):
    """s (V,) f32 = logit / T -> the entries the top-k filter keeps (ties at the k-th value all stay)"""
    V = len(s)
    if 0 < top_k < V:
        return s >= np.sort(s)[V - top_k]
    return np.ones(V, bool)


def top_p_sets(s, keep, top_p, eps=TOP_P_EPS):
    """The nucleus rule of include/lwm_hip.h in fp64 from the f32 s (V,), over the top-k survivors `keep` (V,) bool:
    w = exp(s - max_K s), Z = sum_K w, M(j) = mass of K strictly above j; j stays iff M(j) < top_p * Z (top_p as the f32
    the C struct carries).  -> (S_minus, S_plus, margin): S(+-) = {j in K: M(j) < top_p * Z * (1 +- eps)} as bool masks,
    margin = min_j |M(j) - top_p * Z| / Z."""
    s = np.asarray(s, np.float32)
    p = float(np.float32(top_p))
    idx = np.flatnonzero(keep)
    sk = s[idx].astype(np.float64)
    with np.errstate(invalid="ignore"):
        w = np.exp(sk - sk.max())
    Z = float(w.sum())
    if not (np.isfinite(Z) and Z > 0):                     # no finite maximum: nothing to normalise by, K stays whole
        return keep.copy(), keep.copy(), np.inf
    order = np.argsort(-sk, kind="stable")
    so = sk[order]
    csum = np.cumsum(w[order])
    first = np.searchsorted(-so, -so, side="left")         # the first member of each group of equal s
    M = np.full(len(s), np.inf)
    M[idx[order]] = np.where(first > 0, csum[np.maximum(first, 1) - 1], 0.0)
    lo = keep & (M < p * Z * (1.0 - eps))
    hi = keep & (M < p * Z * (1.0 + eps))
    return lo, hi, float(np.abs(M[idx] - p * Z).min() / Z)


def scores(s, b, seed, step):
    """s (V,) f32 -> (s + g in f32, g): g the Gumbel noise of (seed, entry, row b, step)"""
    V = len(s)
    j = np.arange(V)
    ctr = np.stack([j // 4, np.full(V, b), np.full(V, step & 0xFFFFFFFF), np.zeros(V, np.int64)], -1)
    g = gumbel(philox4x32_10(ctr, seed)[j, j % 4])
    return (s + g).astype(np.float32), g


def band_tokens(s, lo, hi, b, seed, step):
    """the tokens a kernel may emit whose keep set is a prefix of the descending order between lo and hi: the
    Gumbel-argmax (lowest index on ties) of lo plus each run of whole tie groups of hi minus lo, from the top"""
    s = np.asarray(s, np.float32)
    z = scores(s, b, seed, step)[0]
    pick = lambda m: int(np.flatnonzero(m)[np.argmax(z[m])])
    out = {pick(lo)} if lo.any() else set()
    cur = lo.copy()
    for v in sorted(set(s[hi & ~lo].tolist()), reverse=True):
        cur = cur | (hi & (s == np.float32(v)))
        out.add(pick(cur))
    return out


def sample(logits, *, temperature, top_k, seed, step, cfg=None, top_p=None, near_tol=1e-6):
    """tests._sample_ref.sample with the nucleus filter after top-k, exactly as top_p_sets states it (eps = 0).
    -> (tokens (B,) int64, None, number of near-tie draws) -- the same triple, the same near-tie measure.  top_p None or
    >= 1, or greedy: that function itself."""
    if top_p is None or not 0 < top_p < 1 or not temperature > 0:
        return _sample_without_top_p(logits, temperature=temperature, top_k=top_k, seed=seed, step=step, cfg=cfg,
                                     near_tol=near_tol)
    lg = mixed_logits(logits, cfg)
    toks = np.empty(lg.shape[0], np.int64)
    near = 0
    for b, row in enumerate(lg):
        s = (row / np.float32(temperature)).astype(np.float32)
        keep = top_p_sets(s, top_k_keep(s, top_k), top_p, 0.0)[0]
        z, g = scores(s, b, seed, step)
        idx = np.flatnonzero(keep)
        zz = z[idx]
        toks[b] = idx[np.argmax(zz)]
        if len(idx) > 1:
            o = np.argsort(-zz.astype(np.float64), kind="stable")[:2]
            z1, z2 = float(zz[o[0]]), float(zz[o[1]])
            if np.isfinite(z1) and np.isfinite(z2):
                scale = max(1.0, abs(z1), abs(z2), abs(float(g[idx[o[0]]])), abs(float(g[idx[o[1]]])))
                near += abs(z1 - z2) <= near_tol * scale
    return toks, None, near
