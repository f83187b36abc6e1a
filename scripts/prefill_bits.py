"""Bit identity of the block-attention kernels between two builds (profiles/r25_prefill_refactor.md, section 1): the same
seeded inputs through the C ABI of one library, every output byte into one .npz; two such files are then compared.

  python scripts/prefill_bits.py dump LIB OUT.npz [--gpu]    LIB: a liblwm_emu.so (host buffers) or, with --gpu, a liblwm_hip.so
  python scripts/prefill_bits.py cmp A.npz B.npz             exit status 1 and the names that differ, if any do

Calls, at every shape of the prefill CASES of tests/test_emu_kv8_prefill.py, with the case's key_valid (all ones where
the case has none) and without one: lwm_attn_prefill_kv8, lwm_attn_prefill_kv6, lwm_attn_fwd in its partials form
(final_out = 0, k_splits >= 2, on the dequantised 8-bit cache as bf16) -- and lwm_attn_fwd once with a dense_mask.  The
outputs are filled with NaN before each call, so an element a build does not write shows as a difference too."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lwm_amd import _capi                                           # noqa: E402
from oracle.attention_ref import round_bf16, to_bf16_bits           # noqa: E402
from tests import _kv6_ref as K6, _kv8_ref as K8                    # noqa: E402
from tests.test_emu_kv8_prefill import CASES                        # noqa: E402


class Host:
    """numpy buffers, 16-byte aligned: the emulated library"""
    def put(self, a):
        raw = np.zeros(a.nbytes + 16, np.uint8)
        off = (-raw.ctypes.data) % 16
        b = raw[off:off + a.nbytes].view(a.dtype).reshape(a.shape)
        b[...] = a
        return b, b.ctypes.data

    def get(self, b):
        return np.array(b)


class Device:
    """torch buffers on the GPU: the product library, default stream"""
    def put(self, a):
        import torch
        t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
        return t, t.data_ptr()

    def get(self, t):
        import torch
        torch.cuda.synchronize()
        return t.cpu().numpy()


def _rnd(shape, seed, mag=1.0):
    return round_bf16((np.random.default_rng(seed).standard_normal(shape) * mag).astype(np.float32))


def _t4(ptr, shape):
    B, S, H, D = shape
    return _capi.LwmTensor4(ptr, S * H * D, H * D, D)


def dump(L, mem, out):
    nan = lambda shape: mem.put(np.full(shape, np.nan, np.float32))
    res = {}

    def call(name, fn, a, P, B, Sq, H):
        (op, a.out_acc), (lp, a.lse_acc) = nan((P, B, Sq, H, 128)), nan((P, B, H, Sq))
        _capi.check(L, getattr(L, fn)(C.byref(a), None), fn)
        res[name + " out"], res[name + " lse"] = mem.get(op).view(np.uint32), mem.get(lp).view(np.uint32)

    for i, (B, Q, idx, rows, H, n, pad) in enumerate(CASES):
        Sk = idx + Q
        q = _rnd((B, Q, H, 128), 100 + i)
        k, v = _rnd((B, rows, H, 128), 200 + i, 1.5), _rnd((B, rows, H, 128), 300 + i, 0.7)
        kv = np.ones((B, rows), np.uint8)
        kv[0, :pad or 0] = 0
        qb, qp = mem.put(to_bf16_bits(q))
        kvb, kvp = mem.put(kv)
        (k8, s8k), (v8, s8v) = K8.quantise(k), K8.quantise(v)
        kd, vd = to_bf16_bits(K8.dequant(k8, s8k)[:, :Sk]), to_bf16_bits(K8.dequant(v8, s8v)[:, :Sk])
        quant = {"kv8": (_capi.LwmKv8PrefillArgs, 128, k8, s8k, v8, s8v), "kv6": (_capi.LwmKv6PrefillArgs, 96) + K6.quantise(k) + K6.quantise(v)}
        for valid in (True, False):
            tag = f"case {i} {'key_valid' if valid else 'no key_valid'}:"
            for fmt, (args, hb, kq, ks, vq, vs) in quant.items():
                keep = [mem.put(np.ascontiguousarray(t)) for t in (kq, ks, vq, vs)]
                a = args()
                a.q = _t4(qp, q.shape)
                a.k, a.k_scale, a.v, a.v_scale = (p for _, p in keep)
                a.k_stride_b, a.k_stride_s, a.k_stride_h = a.v_stride_b, a.v_stride_s, a.v_stride_h = rows * H * hb, H * hb, hb
                per_head = ks.size // (B * rows * H)         # scale strides in elements of the scale tensor
                a.k_scale_stride_b, a.k_scale_stride_s = a.v_scale_stride_b, a.v_scale_stride_s = rows * H * per_head, H * per_head
                if valid:
                    a.key_valid, a.key_valid_stride_b = kvp, rows
                a.B, a.Sq, a.Sk, a.H, a.D, a.q_start, a.scale, a.k_splits = B, Q, Sk, H, 128, idx, 1.0 / np.sqrt(128), n
                call(f"{tag} lwm_attn_prefill_{fmt}", f"lwm_attn_prefill_{fmt}", a, max(1, n), B, Q, H)
            # the bf16 kernel on a bf16 copy of the first Sk rows; its key_valid rows are Sk apart
            (kb, kp), (vb, vp), (fb, fp) = mem.put(kd), mem.put(vd), mem.put(np.ascontiguousarray(kv[:, :Sk]))
            a = _capi.LwmAttnArgs()
            a.q, a.k, a.v = _t4(qp, q.shape), _t4(kp, kd.shape), _t4(vp, vd.shape)
            a.B, a.H, a.Sq, a.Sk, a.D, a.q_start, a.scale, a.causal, a.k_splits = B, H, Q, Sk, 128, idx, 1.0 / np.sqrt(128), 1, max(2, n)
            if valid:
                a.key_valid = fp
            call(f"{tag} lwm_attn_fwd partials", "lwm_attn_fwd", a, max(2, n), B, Q, H)
            if i == 1 and valid:                         # ... and once its dense-mask path: a random mask, not causal
                m = (np.random.default_rng(7).random((B, Q, Sk)) < 0.7).astype(np.uint8)
                m[:, 5] = 0                              # a query that sees nothing
                mb, mp = mem.put(m)
                a.causal, a.key_valid, a.dense_mask, a.mask_stride_b, a.mask_stride_q = 0, None, mp, Q * Sk, Sk
                call(f"{tag} lwm_attn_fwd dense_mask", "lwm_attn_fwd", a, max(2, n), B, Q, H)
    np.savez(out, **res)
    print(f"{len(res)} arrays -> {out}")


def cmp(a, b):
    A, B = np.load(a), np.load(b)
    assert sorted(A.files) == sorted(B.files), "the two files hold different calls"
    bad = [n for n in A.files if not np.array_equal(A[n], B[n])]
    for n in bad:
        print(f"DIFFERS: {n}: {int((A[n] != B[n]).sum())} of {A[n].size} words")
    print(f"{len(A.files) - len(bad)} of {len(A.files)} arrays bit-equal")
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1] == "cmp":
        sys.exit(cmp(sys.argv[2], sys.argv[3]))
    gpu = "--gpu" in sys.argv
    if gpu:
        import torch                                     # noqa: F401  (its HIP runtime first: lwm_amd/_lib.py)
    dump(_capi.bind(C.CDLL(os.path.abspath(sys.argv[2]))), Device() if gpu else Host(), sys.argv[3])
