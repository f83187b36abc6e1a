"""lwm_gemm_rows_fused_bf16 / lwm_gemm_rows_fused_w8 (csrc/gemm_rows.h) on the CPU: the kernels host-emulated through the C
ABI, every buffer guarded and poison-filled.  The checks themselves live in tests/_rows_cases.py and run unchanged on the
device (tests/test_gpu_rows.py).  The emulated matrix instruction adds its 32 products in k order, the device's in its own
order: only the exact cases and the comparisons of the new entries with each other are bitwise, everything else is held to
a bound derived from f32 accumulation."""
import ctypes as C

import pytest

from lwm_amd import _capi
from tests import _rows_cases as RC

B = RC.HostBackend()
ids = lambda v: str(v).replace(" ", "")


@pytest.mark.parametrize("rows", RC.ROWS)
@pytest.mark.parametrize("Ns", RC.NSETS, ids=ids)
@pytest.mark.parametrize("K", RC.KS_)
def test_exact_cases(K, Ns, rows):
    RC.check_exact(B, rows, K, Ns)


@pytest.mark.parametrize("rows", RC.ROWS)
@pytest.mark.parametrize("Ns", RC.SS_NS, ids=ids)
@pytest.mark.parametrize("K", RC.KS_)
def test_exact_residual_and_ss_out(K, Ns, rows):
    RC.check_exact_residual_ss(B, rows, K, Ns)


@pytest.mark.parametrize("rows", RC.ROWS)
@pytest.mark.parametrize("Ns", RC.NSETS, ids=ids)
@pytest.mark.parametrize("K", RC.KS_)
def test_random_data_against_fp64(K, Ns, rows):
    RC.check_random(B, rows, K, Ns)


@pytest.mark.parametrize("n_ss", [1, 32, 64])
@pytest.mark.parametrize("rows", [5, 17, 32])
@pytest.mark.parametrize("K,Ns", [(160, (520,)), (384, (64, 1032))], ids=ids)
def test_norm_on_load(K, Ns, rows, n_ss):
    RC.check_norm(B, rows, K, Ns, n_ss)


@pytest.mark.parametrize("rows", RC.ROWS)
@pytest.mark.parametrize("Ns", RC.NSETS + RC.SS_NS, ids=ids)
@pytest.mark.parametrize("K", RC.KS_)
def test_packs_equal_the_bf16_entry_on_the_rounded_weights(K, Ns, rows):
    RC.check_packs(B, rows, K, Ns)


@pytest.mark.parametrize("K,Ns,fused", [(160, (520,), False), (384, (64, 1032), False), (384, (384,), True)], ids=ids)
def test_row_independence(K, Ns, fused):
    RC.check_row_independence(B, K, Ns, fused)


@pytest.mark.parametrize("w8", [False, True], ids=["bf16", "w8"])
@pytest.mark.parametrize("name", list(RC.REFUSALS))
def test_refusals_touch_nothing(name, w8):
    RC.check_refusal(B, w8, name)


@pytest.mark.parametrize("name", list(RC.W8_REFUSALS))
def test_w8_refusals_touch_nothing(name):
    RC.check_refusal(B, True, name)


@pytest.mark.parametrize("w8", [False, True], ids=["bf16", "w8"])
def test_the_unedited_arguments_are_accepted(w8):
    RC.check_accepted(B, w8)


# ---------------------------------------------------------------- the same table against lwm_gemv_fused_bf16 / _w8
@pytest.mark.parametrize("w8", [False, True], ids=["bf16", "w8"])
@pytest.mark.parametrize("name", list(RC.GEMV_REFUSALS))
def test_gemv_refusals_touch_nothing(name, w8):
    RC.check_refusal(B, w8, name, entry="gemv")


@pytest.mark.parametrize("name", list(RC.W8_REFUSALS))
def test_gemv_w8_refusals_touch_nothing(name):
    RC.check_refusal(B, True, name, entry="gemv")


@pytest.mark.parametrize("w8", [False, True], ids=["bf16", "w8"])
@pytest.mark.parametrize("name", ("rows 0",) + RC.GEMV_ACCEPTS)
def test_gemv_accepts_what_the_rows_entries_refuse(name, w8):
    RC.check_gemv_accepts(B, w8, name)


@pytest.mark.parametrize("w8", [False, True], ids=["bf16", "w8"])
def test_gemv_unedited_arguments_are_accepted(w8):
    RC.check_accepted(B, w8, entry="gemv")


def test_abi_mirror():
    L = B.lib()
    assert L.lwm_version() >= 560
    assert L.lwm_sizeof(3) == C.sizeof(_capi.LwmGemvArgs) and L.lwm_sizeof(9) == C.sizeof(_capi.LwmGemvW8Args)
