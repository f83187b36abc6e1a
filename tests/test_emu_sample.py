"""The token sampler (lwm_sample_tokens, lwm_amd/csrc/sample.h) in the host emulation, through the C ABI, against the
numpy restatement of tests/_sample_ref.py -- token for token -- and its argument validation on the real library (no
GPU: every bad argument is refused before a launch)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from lwm_amd import _capi
from tests import _emu
from tests import _sample_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_philox_known_answers(tmp_path):
    """the header's Philox4x32-10 (compiled for the host) and the numpy restatement against rocRAND's words"""
    src = tmp_path / "philox.cpp"
    src.write_text(r'''
#include "emu/wave_ops.h"
#include "sample.h"
#include <stdio.h>
#include <stdlib.h>
int main(int argc, char** argv) {
    const unsigned long long seed = strtoull(argv[1], 0, 0);
    uint32_t c[4];
    for (int i = 0; i < 4; ++i) c[i] = (uint32_t)strtoul(argv[2 + i], 0, 0);
    lwm::philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    printf("%u %u %u %u\n", c[0], c[1], c[2], c[3]);
    return 0;
}
''')
    exe = tmp_path / "philox"
    subprocess.run([_emu.CLANG, "-O1", "-std=c++17", "-I", os.path.join(ROOT, "tests"), "-I", os.path.join(ROOT, "lwm_amd", "csrc"),
                    str(src), "-o", str(exe), "-lpthread"], check=True)
    for seed, ctr, words in R.PHILOX_KAT:
        out = subprocess.run([str(exe), str(seed)] + [str(c) for c in ctr], capture_output=True, text=True, check=True)
        assert tuple(int(w) for w in out.stdout.split()) == words, (seed, ctr)
        assert tuple(int(w) for w in R.philox4x32_10(np.array(ctr), seed)) == words, (seed, ctr)


def emu_sample(logits, *, temperature, top_k, seed, step=0, step_dev=None, step_base=0, cfg=None, force_period=0,
               force_token=0, done=None, eos=-1, pad=0, copies=1, seq_cols=0, ld_pad=3):
    """lwm_sample_tokens on the emulated kernel.  The logits rows sit ld_pad NaN columns apart (the kernel must not read
    past V).  -> (tokens (copies, B), done or None, seq (B, seq_cols) or None)"""
    L = _emu.lib()
    rows, V = logits.shape
    B = rows // 2 if cfg is not None else rows
    buf = _emu.aligned((rows, V + ld_pad), np.float32)
    buf[:] = np.nan
    buf[:, :V] = logits
    keep = []
    a = _capi.LwmSampleArgs()
    a.logits, a.ld, a.rows, a.V = buf.ctypes.data, V + ld_pad, rows, V
    if cfg is not None:
        cf = _emu.aligned((B,), np.float32)
        cf[:] = cfg
        keep.append(cf)
        a.cfg_scale = cf.ctypes.data
    a.temperature, a.top_k, a.seed = temperature, top_k, seed
    if step_dev is not None:
        sd = _emu.aligned((1,), np.int32)
        sd[0] = step_dev
        keep.append(sd)
        a.step_dev = sd.ctypes.data
    a.step_base, a.step = step_base, step
    a.force_period, a.force_token = force_period, force_token
    dn = None
    if done is not None:
        dn = _emu.aligned((B,), np.uint8)
        dn[:] = done
        a.done = dn.ctypes.data
    a.eos, a.pad = eos, pad
    toks = _emu.aligned((copies, B), np.int64)
    toks[:] = -1
    a.tokens, a.copies = toks.ctypes.data, copies
    seq = None
    if seq_cols:
        seq = _emu.aligned((B, seq_cols), np.int64)
        seq[:] = -7
        a.seq, a.seq_ld, a.seq_cols = seq.ctypes.data, seq_cols, seq_cols
    _capi.check(L, L.lwm_sample_tokens(C.byref(a), None), "lwm_sample_tokens")
    return toks, dn, seq


def _logits(rng, rows, V, scale=3.0, neg_inf=0):
    lg = (rng.standard_normal((rows, V)) * scale).astype(np.float32)
    if neg_inf:
        lg[:, rng.choice(V, neg_inf, replace=False)] = -np.inf
    return lg


# (V, rows, cfg scales or None, T, k): covers V in {37, 8448, 32000} (and 40000: entries past the register-held ones),
# rows 1 / 2 / 4, guidance off and on with distinct per-row scales, T in {0, 0.2, 1, 3}, k in {0, 1, 50, 1000, 8192, >= V}
GRID = [(V, rows, cfg, T, k)
        for V in (37, 8448, 32000)
        for rows, cfg, T, k in ((1, None, 0.0, 0), (2, (1.0,), 0.2, 0), (4, (5.0, 0.5), 1.0, 50), (2, None, 3.0, 1000),
                                (1, None, 1.0, 1), (4, None, 0.2, 8192), (2, (3.0,), 1.0, V), (4, (1.5, 7.0), 3.0, 0),
                                (2, None, 0.0, 50))] + [(40000, 1, None, 1.0, 100), (40000, 2, (2.0,), 0.2, 0)]


@pytest.mark.parametrize("V,rows,cfg,T,k", GRID)
def test_kernel_matches_numpy_reference(V, rows, cfg, T, k):
    rng = np.random.default_rng(V * 7 + rows * 131 + int(T * 10) + k)
    lg = _logits(rng, rows, V, neg_inf=0 if cfg else min(5, V // 4))      # (-inf - -inf: NaN under guidance)
    seed, step = 0x5EED0000 + V + k, 17 + rows
    toks, _, _ = emu_sample(lg, temperature=T, top_k=k, seed=seed, step=step, cfg=cfg)
    ref, _, near = R.sample(lg, temperature=T, top_k=k, seed=seed, step=step, cfg=cfg)
    assert near == 0
    assert np.array_equal(toks[0], ref), (toks[0], ref)


def test_ties_at_the_kth_value_and_neg_inf_entries():
    """k-th value shared by several entries: all of them stay in the draw; -inf entries are never drawn"""
    rng = np.random.default_rng(3)
    V = 8448
    lg = np.full((2, V), -np.inf, np.float32)
    lg[:, :600] = rng.standard_normal((2, 600)).astype(np.float32)
    lg[:, 600:700] = 2.5                                   # 100 entries tied at the 50th-largest value
    lg[:, :600][lg[:, :600] > 2.5] = 0.0
    lg[0, 5:40] = 3.0 + np.arange(35, dtype=np.float32) / 64   # 35 above the tie: k = 50 lands inside it
    lg[1, 5:40] = 3.0 + np.arange(35, dtype=np.float32) / 64
    seen = set()
    for step in range(40):
        toks, _, _ = emu_sample(lg, temperature=1.0, top_k=50, seed=11, step=step)
        ref, _, near = R.sample(lg, temperature=1.0, top_k=50, seed=11, step=step)
        assert near == 0 and np.array_equal(toks[0], ref)
        seen |= set(toks[0].tolist())
    assert all(5 <= t < 40 or 600 <= t < 700 for t in seen)
    assert any(600 <= t < 700 for t in seen)                 # the tied entries are drawn too
    # nothing finite but one entry: it is the token whatever the filter
    one = np.full((1, 37), -np.inf, np.float32)
    one[0, 29] = -1e30
    for k in (0, 1, 5):
        assert emu_sample(one, temperature=1.0, top_k=k, seed=1)[0][0, 0] == 29


def test_done_rows_emit_pad_and_eos_latches():
    rng = np.random.default_rng(5)
    V, B = 37, 4
    lg = _logits(rng, B, V)
    eos = int(np.argmax(lg[2]))                            # greedy: row 2 emits eos now
    done = np.array([0, 1, 0, 0], np.uint8)
    toks, dn, _ = emu_sample(lg, temperature=0.0, top_k=0, seed=0, done=done, eos=eos, pad=33)
    ref, rdone, _ = R.sample(lg, temperature=0.0, top_k=0, seed=0, step=0, done=done, eos=eos, pad=33)
    assert np.array_equal(toks[0], ref) and np.array_equal(dn, rdone)
    assert toks[0, 1] == 33 and toks[0, 2] == eos and dn.tolist() == [int(np.argmax(lg[0]) == eos), 1, 1,
                                                                        int(np.argmax(lg[3]) == eos)]
    toks2, dn2, _ = emu_sample(lg, temperature=0.0, top_k=0, seed=0, done=dn, eos=eos, pad=33)
    assert toks2[0, 2] == 33 and np.array_equal(dn2, dn)


def test_force_period_copies_seq_column_and_device_step():
    rng = np.random.default_rng(9)
    V, B = 8448, 2
    lg = _logits(rng, 2 * B, V)
    cfg = (5.0, 1.0)
    base = dict(temperature=1.0, top_k=8192, seed=1234, cfg=cfg, force_period=257, force_token=8192, copies=2, seq_cols=600)
    for step in (255, 256, 513):                           # missed, hit (257th token), hit (514th)
        toks, _, seq = emu_sample(lg, step=step, **base)
        ref, _, near = R.sample(lg, temperature=1.0, top_k=8192, seed=1234, step=step, cfg=cfg, force_period=257,
                                force_token=8192)
        assert near == 0 and np.array_equal(toks[0], ref) and np.array_equal(toks[1], ref)
        assert ((ref == 8192).all()) == ((step + 1) % 257 == 0)
        assert np.array_equal(seq[:, step], ref) and (np.delete(seq, step, 1) == -7).all()
        # the same step read from device memory: *step_dev - step_base
        toks_d, _, seq_d = emu_sample(lg, step=0, step_dev=step + 1000, step_base=1000, **base)
        assert np.array_equal(toks_d, toks) and np.array_equal(seq_d, seq)
    # a column outside the sequence is not written
    _, _, seq = emu_sample(lg, step=600, **base)
    assert (seq == -7).all()


def test_draws_differ_by_row_step_and_seed():
    lg = np.zeros((4, 8448), np.float32)                   # uniform: every entry equally likely
    a = emu_sample(lg, temperature=1.0, top_k=0, seed=1, step=0)[0][0]
    assert len(set(a.tolist())) == 4                       # rows draw from their own counters
    assert not np.array_equal(a, emu_sample(lg, temperature=1.0, top_k=0, seed=1, step=1)[0][0])
    assert not np.array_equal(a, emu_sample(lg, temperature=1.0, top_k=0, seed=2, step=0)[0][0])
    assert np.array_equal(a, R.sample(lg, temperature=1.0, top_k=0, seed=1, step=0)[0])


@pytest.fixture(scope="module")
def real_lib():
    so = os.path.join(ROOT, "lwm_amd", "liblwm_hip.so")
    if not os.path.exists(so):
        import __graft_entry__ as g
        g.build()
    return _capi.bind(C.CDLL(so))


def test_validation_refuses_bad_arguments_before_any_launch(real_lib):
    L = real_lib
    assert L.lwm_sizeof(4) == C.sizeof(_capi.LwmSampleArgs)
    assert L.lwm_version() >= 510
    buf = (C.c_char * 4096)()
    base = C.addressof(buf)
    base += (-base) % 16

    def good():
        a = _capi.LwmSampleArgs()
        a.logits, a.ld, a.rows, a.V = base, 64, 2, 64
        a.temperature, a.top_k = 1.0, 0
        a.tokens, a.copies = base + 2048, 1
        return a

    cases = [("logits", dict(logits=None)), ("V", dict(V=0)), ("ld", dict(ld=10)), ("rows", dict(rows=0)),
             ("top_k", dict(top_k=-1)), ("temperature", dict(temperature=-0.5)), ("temperature", dict(temperature=float("nan"))),
             ("odd", dict(rows=3, cfg_scale=base + 1024)), ("no output", dict(tokens=None)), ("copies", dict(copies=0)),
             ("misaligned", dict(logits=base + 2)), ("misaligned", dict(tokens=base + 2052)),
             ("misaligned", dict(cfg_scale=base + 1025)), ("misaligned", dict(step_dev=base + 3)),
             ("force_period", dict(force_period=-1)), ("seq", dict(seq=base + 3072, seq_cols=8, seq_ld=4))]
    for what, fields in cases:
        a = good()
        for f, v in fields.items():
            setattr(a, f, v)
        assert L.lwm_sample_tokens(C.byref(a), None) == _capi.LWM_EINVAL, what
        assert L.lwm_last_error().startswith(b"sample_tokens"), what
    assert L.lwm_sample_tokens(None, None) == _capi.LWM_EINVAL
