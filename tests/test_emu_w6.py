"""The 6-bit (MXFP6) decode weights on the CPU: the numpy restatement of the format (tests/_w6_ref.py) checked against its
own definition, and the kernels of csrc/gemv_w6.h and the 6-bit body of csrc/gemm_rows.h host-emulated through the C ABI --
the quantiser bitwise against the restatement, the GEMV and the rows entry bitwise (outputs AND workspace partials)
against lwm_gemv_fused_bf16 / lwm_gemm_rows_fused_bf16 on the dequantised weights -- the refusals, and the ABI mirror.  The
checks live in tests/_w6_cases.py and run unchanged on the device (tests/test_gpu_w6.py).  Every check is exact."""
import ctypes as C

import numpy as np
import pytest

from lwm_amd import _capi
from tests import _kv4_ref as K4, _kv6_ref as K6, _rows_cases as RC, _w4_ref as W4, _w6_cases as WC, _w6_ref as W6, _w8_ref as W8

B = RC.HostBackend()
ids = lambda v: str(v).replace(" ", "")


# ---------------------------------------------------------------- the restatement itself
def test_restatement_against_its_definition():
    table = K6.E2M3_MAG
    for name, w in W6.quantiser_cases():
        K, N = w.shape
        q, e = W6.quantise(w)
        assert q.shape == (K // 4, N // 8, 24) and q.dtype == np.uint8 and e.shape == (K // 32, N) and e.dtype == np.uint8, name
        assert W6.check_layout(q, (K, N)), name                                          # address formula == the 192-bit integer
        s = np.repeat(2.0 ** (e.astype(np.float64) - 127), 32, axis=0)
        y = w.astype(np.float64) / s
        assert np.abs(y).max() <= 7.5, name                                               # nothing saturates
        codes = W6.unpack_codes(q, (K, N))
        assert np.array_equal(W6.pack_codes(codes), q), name                              # the two statements of the layout agree
        # nearest magnitude, ties to the even code, the sign of zero kept
        d = np.abs(np.abs(y)[..., None] - table)
        assert (np.abs(table[codes & 31] - np.abs(y)) == d.min(-1)).all(), name
        tie = d.min(-1) == np.sort(d, -1)[..., 1]
        assert (codes[tie] % 2 == 0).all(), name
        assert np.array_equal(codes >> 5, np.signbit(w).astype(np.uint8)), name
        # the smallest power of two: half of it no longer fits (except at the lower clamp and for all-zero blocks)
        amax = np.abs(w.astype(np.float64)).reshape(K // 32, 32, N).max(1)
        sb = 2.0 ** (e.astype(np.float64) - 127)
        free = (amax > 0) & (e > 1)
        assert (amax[free] / (sb[free] / 2.0) > 7.5).all() and (amax / sb <= 7.5).all(), name
        assert (e[amax == 0] == 127).all() and e.min() >= 1 and e.max() <= 254, name
        deq = W6.dequant(q, e, (K, N))
        assert np.array_equal(deq, K6.e2m3_decode(codes) * s) and np.isfinite(deq).all(), name
        assert np.array_equal(W6.rounded(q, e, (K, N)).astype(np.float64), deq), name      # every rounded value IS a bf16 number


def test_the_mantissa_threshold_the_clamp_and_the_top():
    (_, w), = [c for c in W6.quantiser_cases() if c[0].startswith("threshold")]
    q, e = W6.quantise(w)
    for c, ex in enumerate((-100, -20, 0, 1, 40, 100)):
        assert e[0, c] == 127 + ex - 2 and e[1, c] == 127 + ex - 1       # 1.875 * 2^e fits 2^(e-2); its bf16 successor does not
    codes = W6.unpack_codes(q, w.shape)
    assert e[0, 9] == 127 and codes[5, 9] == 32                           # an all-zero block; -0 keeps its sign
    assert e[0, 10] == 1                                                  # the lower clamp
    d = W6.dequant(q, e, w.shape)
    assert d[0, 10] == 2.0 ** -127 and d[4, 10] == 3 * 2.0 ** -126 and d[6, 10] == 0 and np.signbit(d[6, 10]) and d[7, 10] == -(2.0 ** -128)
    assert e[1, 11] == 253 and d[33, 11] == 3.75 * 2.0 ** 126 and d[34, 11] == -1.875 * 2.0 ** 127        # the top of bf16
    # ... and the stated limit is where it breaks: 3.875 s is a tie that goes up to the even code, 4 s = 2^128
    assert K6.e2m3_decode(K6.e2m3_encode(np.array([W6.LIMIT / 2.0 ** 126])))[0] * 2.0 ** 126 == 2.0 ** 128


def test_format_properties():
    from oracle.attention_ref import round_bf16
    for name, w in W6.quantiser_cases()[:2]:
        K, N = w.shape
        q, e = W6.quantise(w)
        r = W6.rounded(q, e, w.shape)
        amax = np.repeat(np.abs(w.astype(np.float64)).reshape(K // 32, 32, N).max(1), 32, axis=0)
        free = np.repeat(e > 1, 32, axis=0) & (amax > 0)
        err6 = np.abs(w.astype(np.float64) - r)
        assert (err6[free] < amax[free] / 15).all(), name                                # |w - q s| < amax / 15 off the clamp
        q2, e2 = W6.quantise(r)                                                          # a second quantisation: the same values
        assert np.array_equal(round_bf16(W6.rounded(q2, e2, w.shape)).view(np.uint32), r.view(np.uint32)), name
        ok = np.repeat(np.abs(w).reshape(K // 32, 32, N).max(1) <= 3.5 * 2.0 ** 126, 32, axis=0)      # (the 4-bit format's own limit)
        w4 = np.where(ok, w, 0).astype(np.float32)
        q4, e4 = W4.quantise(w4)
        err4 = np.abs(w4.astype(np.float64) - W4.dequant(q4, e4, w.shape))
        assert (err6[ok] <= err4[ok]).all(), name                                        # element by element no worse than 4 bits
    assert K4 is not None


# ---------------------------------------------------------------- quantiser kernel
@pytest.mark.parametrize("case", W6.quantiser_cases(), ids=lambda c: c[0])
def test_quantiser_equals_the_restatement(case):
    WC.check_quantiser(B, case[1])


def test_quantiser_refusals_touch_nothing():
    WC.check_quantiser_refusals(B)


# ---------------------------------------------------------------- GEMV
@pytest.mark.parametrize("rows", [1, 2, 3, 4])
@pytest.mark.parametrize("K,Ns", W8.GEMV_SHAPES, ids=ids)
def test_gemv_equals_the_bf16_gemv_on_the_rounded_weights(rows, K, Ns):
    WC.check_gemv(B, rows, K, Ns)


@pytest.mark.parametrize("rows", [1, 4])
@pytest.mark.parametrize("K,N", [(160, 48), (416, 2064)])
def test_gemv_norm_on_load(rows, K, N):
    WC.check_gemv_norm(B, rows, K, N)


@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("K,N", [(160, 128), (416, 1152)])
def test_gemv_residual_and_ss_out(rows, K, N):
    WC.check_gemv_residual_ss(B, rows, K, N)


def test_both_entries_through_the_quantiser_kernel():
    WC.check_through_the_quantiser(B)


# ---------------------------------------------------------------- the 5-32-row body
@pytest.mark.parametrize("rows", WC.ROWS_ROWS)
@pytest.mark.parametrize("K,Ns", WC.ROWS_SHAPES, ids=ids)
def test_rows_entry_equals_the_bf16_rows_entry_on_the_rounded_weights(rows, K, Ns):
    WC.check_rows(B, rows, K, Ns)


@pytest.mark.parametrize("rows", [5, 32])
def test_rows_entry_norm_residual_and_ss_out(rows):
    WC.check_rows_residual_ss(B, rows)


def test_a_row_has_the_same_bits_in_a_batch_of_5_and_of_32():
    WC.check_row_independence(B)


# ---------------------------------------------------------------- validation
@pytest.mark.parametrize("name", WC.refusal_names("gemv"))
def test_gemv_refusals_touch_nothing(name):
    WC.check_refusal(B, "gemv", name)


@pytest.mark.parametrize("name", WC.refusal_names("rows"))
def test_rows_refusals_touch_nothing(name):
    WC.check_refusal(B, "rows", name)


@pytest.mark.parametrize("entry", ["gemv", "rows"])
def test_the_unedited_arguments_are_accepted(entry):
    WC.check_accepted(B, entry)


# ---------------------------------------------------------------- ABI
def test_abi_mirror():
    L = B.lib()
    assert L.lwm_version() >= 640
    assert L.lwm_sizeof(15) == C.sizeof(_capi.LwmGemvW6Args)
    assert C.sizeof(_capi.LwmGemvW6Args) == C.sizeof(_capi.LwmGemvArgs) + 3 * C.sizeof(C.c_void_p)
