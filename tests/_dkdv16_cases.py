"""The dK/dV kernel at the smallest shapes that reach each of its paths: case table and verdict shared by the host
emulator (tests/test_emu_dkdv16.py) and the device (tests/test_gpu_dkdv16.py).  TEST INFRASTRUCTURE ONLY.

The kernel walks the queries in steps of 64, last step first (two units of 32 queries x the wave's 32 keys, each unit cut
into 16 x 16 tiles for v_mfma_f32_16x16x32_bf16); a workgroup holds 128 keys, a wave 32.  Sq = 32 .. 320 gives walks of
1, 1, 2, 3 and 5 steps: the short-walk branch (fewer than three steps, nothing pipelined), the first piped step, the
steady loop, the two unpiped last steps and the drain; Sq = 32 and 100 have a ragged top step; segment ids or key_valid
select the `_meta` kernel.

Cases are tests/_attn_cases.py's Case objects (its builders, and its strided pair as the B = 2 instance).  The bound is
the one tests/test_gpu_attention.py::test_fwd_bwd_vs_oracle holds dk and dv to: tests/_parity.py::check against the fp64
oracle's gradients for the saved (bf16) output; every element of dk and dv takes part."""
import functools

import numpy as np

from oracle import attention_ref as R
from tests import _attn_cases as A, _parity

Case, _qkvdo = A.Case, A._qkvdo


def _walk_cases():
    out = []
    for Sq in (32, 64, 128, 192, 320):
        # every query sees every key: the whole walk, no mask code
        out.append(Case(f"walk_sq{Sq}", *_qkvdo(1, Sq, 128, 2, 1900 + Sq), dict(causal=False)))
    for S in (128, 320):
        # the diagonal: the units that need the causal mask, key blocks whose walk ends early
        out.append(Case(f"causal_s{S}", *_qkvdo(1, S, S, 2, 1950 + S), dict(causal=True)))
    return out


def _shape_cases():
    out = []
    # a ragged top step (Sq % 64 = 36: its own staging offsets, padded statistics), bare and below the diagonal
    out.append(Case("ragged_sq100", *_qkvdo(1, 100, 128, 2, 2000), dict(causal=False)))
    out.append(Case("ragged_sq100_causal", *_qkvdo(1, 100, 128, 2, 2001), dict(causal=True, q_start=36)))
    out.append(Case("ragged_sq228_causal", *_qkvdo(1, 228, 128, 2, 2002), dict(causal=True, q_start=20)))     # n = 4, ragged top of a piped walk
    # a wave past the end of the keys (Sk = 40: wave 1 holds 8 keys, waves 2 and 3 none)
    out.append(Case("sk40", *_qkvdo(1, 128, 40, 2, 2010), dict(causal=True, k_start=60)))
    # an off-diagonal block of a ring: position offsets on both sides
    out.append(Case("offdiag_causal", *_qkvdo(1, 160, 128, 2, 2020), dict(causal=True, q_start=512, k_start=256)))
    out.append(Case("offdiag_full", *_qkvdo(1, 160, 128, 2, 2021), dict(causal=False, q_start=512, k_start=256)))
    out.append(Case("offdiag_crossing", *_qkvdo(1, 160, 128, 2, 2022), dict(causal=True, q_start=3, k_start=70)))
    return out


def _mask_cases():
    out = []
    # packed documents: queries 0..63 are one document (a segment-uniform step), the cuts at 100 and 200 fall inside steps
    seg = A._segments(1, 256, cuts=(64, 100, 200))
    out.append(Case("segments", *_qkvdo(1, 256, 256, 2, 2030), dict(causal=True, seg_q=seg, seg_k=seg)))
    out.append(Case("key_valid", *_qkvdo(1, 192, 128, 2, 2040), dict(causal=False, key_valid=A._sparse_valid(1, 128, 13, p=0.3))))
    # keys no query sees: the last 32 keys lie behind every query
    out.append(Case("dead_keys", *_qkvdo(1, 64, 64, 2, 2050), dict(causal=True, q_start=0, k_start=32)))
    kv = np.ones((1, 128), np.uint8)
    kv[:, 40:90] = 0
    out.append(Case("dead_keys_meta", *_qkvdo(1, 128, 128, 2, 2051), dict(causal=True, key_valid=kv)))
    return out


def _map_cases():
    # the two branches of the block -> (key block, head, batch) map: B * H a multiple of 8 or not; more than one key block
    return [Case("map_h8", *_qkvdo(1, 128, 256, 8, 2060), dict(causal=True, q_start=128)),
            Case("map_h2", *_qkvdo(1, 128, 256, 2, 2061), dict(causal=True, q_start=128))] + A.strided_cases()       # (B = 2)


CASES = _walk_cases() + _shape_cases() + _mask_cases() + _map_cases()
CARRY_CASE = next(c for c in CASES if c.name == "walk_sq192")
DEAD_KEYS = {"dead_keys": 32 * 1, "dead_keys_meta": 50 * 1, "sk40": 0}      # keys (per batch row) that no query sees


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (out saved as bf16 values, lse, dk and dv for the saved output, keys no query sees): computed once"""
    case = next(c for c in CASES if c.name == name)
    q, k, v, do = case.operands(False)
    ro, rl = R.dense_attention(q, k, v, **case.kw)
    out_saved = R.round_bf16(ro.astype(np.float32))
    _, rk, rv, _ = R.dense_attention_bwd(q, k, v, do, out_saved=out_saved, **case.kw)
    dead = ~A.visibility(case, q.shape[1], k.shape[1], q.shape[0]).any(axis=1)
    if name in DEAD_KEYS:
        assert int(dead.sum()) == DEAD_KEYS[name], (name, int(dead.sum()))
    for a in (out_saved, rk, rv):
        a.setflags(write=False)
    return out_saved, rl.astype(np.float32), rk, rv, dead


def verify_dkdv(case, dk, dv, offset=None):
    """dk, dv: what the kernel wrote, float; offset: (dk, dv) it was asked to add onto (the f32 carries)"""
    _, _, rk, rv, dead = reference(case.name)
    for n, got, ref, off in (("dk", dk, rk, None if offset is None else offset[0]), ("dv", dv, rv, None if offset is None else offset[1])):
        got = np.asarray(got, np.float64)
        assert not np.isnan(got).any(), f"{case.name}: NaN in {n}"
        if off is not None:
            ref = ref + off
        elif dead.any():
            assert not got[dead].any(), f"{case.name}: {n} of keys that no query sees must be 0"
        g = np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-9)
        print(f"{case.name}.{n}: max|err| / max|ref| = {g:.3e} (bound {_parity.TOL})")
        _parity.check(f"{case.name}.{n}", got, ref)
