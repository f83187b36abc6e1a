"""numpy restatement of the token sampler (lwm_amd/csrc/sample.h; lwm_sample_tokens in include/lwm_hip.h): the reference
the emulated and the device kernel are held to, token for token.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_M32 = np.uint64(0xFFFFFFFF)

# Philox4x32-10 known answers: (seed, counter, output words), from rocRAND's host implementation
# (rocrand_device::philox4x32_10_engine(seed, subsequence = c2 | c3 << 32, offset = 4 * (c0 | c1 << 32)).next4()).
# The first is Random123's published answer for a zero key and counter.
PHILOX_KAT = [
    (0x0000000000000000, (0, 0, 0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    (0x0123456789abcdef, (0, 0, 0, 0), (0xb850222e, 0xc58cb04b, 0x14a7a020, 0x7a84fff9)),
    (0x0000000001352898, (5, 1, 257, 0), (0x941f6d10, 0x4c939979, 0x1fa33e3e, 0x5ee6d9f8)),
    (0xffffffffffffffff, (4294967295, 3, 2147483647, 0), (0xe2d667d4, 0xe294e5e2, 0x28a715d3, 0xa81f0810)),
    (0x000000000000002a, (7999, 3, 513, 0), (0x591e31fe, 0xfc7dc37c, 0x38f318d3, 0x72665db0)),
]


def philox4x32_10(ctr, seed):
    """ctr (..., 4) integer array of 32-bit words -> (..., 4) uint32 (key = the 64-bit seed)"""
    ctr = np.asarray(ctr, dtype=np.uint64)
    c = [ctr[..., i] & _M32 for i in range(4)]
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    for r in range(10):
        if r:
            k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & _M32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & _M32]
    return np.stack(c, -1).astype(np.uint32)


def uniform(x):
    """((x >> 9) + 0.5) * 2^-23 in f32: exact, inside (0, 1)"""
    return ((np.asarray(x, np.uint32) >> 9).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -23)


def gumbel(x):
    """-log(-log(u)) with each log rounded to f32 once (the double log, rounded)"""
    a = np.log(uniform(x).astype(np.float64)).astype(np.float32)
    return -np.log((-a).astype(np.float64)).astype(np.float32)


def mixed_logits(logits, cfg=None):
    """u + s * (c - u) in f32, three roundings (lwm_amd/vision_llama.py's eager order)"""
    logits = np.asarray(logits, np.float32)
    if cfg is None:
        return logits
    B = logits.shape[0] // 2
    c, u = logits[:B], logits[B:]
    s = np.asarray(cfg, np.float32).reshape(B, 1)
    return u + s * (c - u)


def sample(logits, *, temperature, top_k, seed, step, cfg=None, force_period=0, force_token=0, done=None, eos=-1, pad=0,
           near_tol=1e-6):
    """-> (tokens (B,) int64, updated done or None, number of near-tie draws).  A draw is a near tie when its two best
    perturbed scores lie within near_tol of each other relative to their magnitude (a log ulp could swap them)."""
    lg = mixed_logits(logits, cfg)
    B, V = lg.shape
    toks = np.empty(B, np.int64)
    done = None if done is None else np.array(done, np.uint8)
    near = 0
    j = np.arange(V)
    for b in range(B):
        row = lg[b]
        if not temperature > 0:
            t = int(np.argmax(row))
        else:
            s = (row / np.float32(temperature)).astype(np.float32)
            keep = np.ones(V, bool)
            if 0 < top_k < V:
                keep = s >= np.sort(s)[V - top_k]
            ctr = np.stack([j // 4, np.full(V, b), np.full(V, step & 0xFFFFFFFF), np.zeros(V, np.int64)], -1)
            g = gumbel(philox4x32_10(ctr, seed)[j, j % 4])
            z = (s + g).astype(np.float32)
            idx = np.flatnonzero(keep)
            zz = z[idx]
            t = int(idx[np.argmax(zz)])
            if len(idx) > 1:
                o = np.argsort(-zz.astype(np.float64), kind="stable")[:2]
                z1, z2 = float(zz[o[0]]), float(zz[o[1]])
                if np.isfinite(z1) and np.isfinite(z2):
                    scale = max(1.0, abs(z1), abs(z2), abs(float(g[idx[o[0]]])), abs(float(g[idx[o[1]]])))
                    near += abs(z1 - z2) <= near_tol * scale
        if force_period > 0 and (step + 1) % force_period == 0:
            t = force_token
        if done is not None:
            if done[b]:
                t = pad
            if eos >= 0 and t == eos:
                done[b] = 1
        toks[b] = t
    return toks, done, near
