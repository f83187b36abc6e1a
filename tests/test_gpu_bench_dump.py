"""bench.py --dump-outputs hands over what its timed path computed: the files of a short run equal, bit for bit, what
the same writer makes of one layer of ring_forward / ring_backward on the benchmark's own seeded inputs (the layers of a
step all see the same q, k, v, dO, and the attention kernels are deterministic).  The writer itself is checked without a
GPU in tests/test_bench_contract.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("out", "lse", "dq", "dk", "dv")


@pytest.mark.gpu
def test_bench_dump_is_the_timed_paths_last_layer(tmp_path):
    S = 4096
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--seq", str(S), "--layers", "2",
                        "--steps", "2", "--warmup", "0", "--dump-outputs", str(tmp_path / "bench")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 2 and line["ms_per_step"] > 0

    import torch
    sys.path.insert(0, ROOT)
    import bench
    from lwm_amd.ring import HipBlockOps, SeqLayout, SingleComm, ring_backward, ring_forward
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1234)          # bench.py's inputs: rank 0, in the order q, k, v, dO
    mk = lambda: torch.randn(1, S, bench.N_HEADS, bench.HEAD_DIM, generator=g, device=dev,
                             dtype=torch.float32).to(torch.bfloat16)
    q, k, v, do = mk(), mk(), mk(), mk()
    lay = SeqLayout("zigzag", 1, S)
    out, lses = ring_forward(HipBlockOps, SingleComm(), q, k, v, layout=lay, causal=True)
    grads = ring_backward(HipBlockOps, SingleComm(), q, k, v, out, lses, do, layout=lay, causal=True)
    torch.cuda.synchronize()
    bench.dump_outputs(torch, str(tmp_path / "direct"), (out, lses, grads), 0, 1)
    for n in NAMES:
        a, b = np.load(tmp_path / "bench" / f"{n}.npy"), np.load(tmp_path / "direct" / f"{n}.npy")
        assert a.dtype == np.float32 and a.shape == b.shape and np.isfinite(a).all(), n
        assert np.array_equal(a, b), (n, float(np.abs(a - b).max()))
