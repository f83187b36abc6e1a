"""Bit identity of the three decode-weight quantisers between two builds (profiles/r28_decode_packs.md, section 1; the method
of scripts/prefill_bits.py): the same seeded kernels through the C ABI of one library, every output word into one .npz; two
such files are then compared.

  python scripts/quantise_bits.py dump LIB OUT.npz [--gpu]    LIB: a liblwm_emu.so (host buffers) or, with --gpu, a liblwm_hip.so
  python scripts/quantise_bits.py cmp A.npz B.npz             exit status 1 and the names that differ, if any do

Calls: lwm_w8_quantise, lwm_w6_quantise, lwm_w4_quantise at the quantiser cases of each format's tests (tests/_w8_ref.py,
_w6_ref.py, _w4_ref.py) and at 4096 x 11008 and 11008 x 4096, each once into a `rounded` of its own and once in place.  q,
scale and rounded are filled with NaN patterns before each call, so a word a build does not write shows as a difference."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lwm_amd import _capi                                           # noqa: E402
from oracle.attention_ref import round_bf16, to_bf16_bits           # noqa: E402
from scripts.prefill_bits import Device, Host, cmp                  # noqa: E402
from tests import _w4_ref as W4, _w6_ref as W6, _w8_ref as W8       # noqa: E402

# tag -> (the test cases, bytes of q per (K, N), bytes of scale per (K, N))
FORMATS = {"w8": (W8, lambda K, N: K * N, lambda K, N: (K + 127) // 128 * N * 4),
           "w6": (W6, lambda K, N: K * N * 3 // 4, lambda K, N: K // 32 * N),
           "w4": (W4, lambda K, N: K * N // 2, lambda K, N: K // 32 * N)}
BIG = [(4096, 11008), (11008, 4096)]


def dump(L, mem, out):
    res = {}
    for tag, (ref, q_bytes, s_bytes) in FORMATS.items():
        cases = [(name, to_bf16_bits(w)) for name, w in ref.quantiser_cases()]
        for i, (K, N) in enumerate(BIG):
            w = np.random.default_rng(40 + i).standard_normal((K, N)).astype(np.float32) * 0.02
            cases.append((f"{K}x{N}", to_bf16_bits(round_bf16(w))))
        for name, bits in cases:
            K, N = bits.shape
            for in_place in (False, True):
                wb, wp = mem.put(bits)
                qb, qp = mem.put(np.full(q_bytes(K, N), 0xc1, np.uint8))
                sb, sp = mem.put(np.full(s_bytes(K, N), 0xff, np.uint8))
                rb, rp = (wb, wp) if in_place else mem.put(np.full((K, N), 0x7fc1, np.uint16))
                fn = f"lwm_{tag}_quantise"
                _capi.check(L, getattr(L, fn)(wp, qp, sp, rp, K, N, None), fn)
                key = f"{fn} {name} {'in place' if in_place else 'apart'}:"
                res[key + " q"], res[key + " scale"], res[key + " rounded"] = mem.get(qb), mem.get(sb), mem.get(rb)
    np.savez(out, **res)
    print(f"{len(res)} arrays, {sum(a.nbytes for a in res.values()) // 4} words -> {out}")


if __name__ == "__main__":
    if sys.argv[1] == "cmp":
        sys.exit(cmp(sys.argv[2], sys.argv[3]))
    gpu = "--gpu" in sys.argv
    if gpu:
        import torch                                     # noqa: F401  (its HIP runtime first: lwm_amd/_lib.py)
    dump(_capi.bind(C.CDLL(os.path.abspath(sys.argv[2]))), Device() if gpu else Host(), sys.argv[3])
