"""No tensor reaches the C library unchecked (the CPU half; tests/test_gpu_op_boundary.py is the device half).

The C entry points check null pointers, alignment and strides; shape, device and dtype are the Python wrappers' job.
Every wrapper of lwm_amd.llama_ops / lwm_amd.ops that hands a `data_ptr()` to the library is one row of
tests/_boundary.py.  Here every row is called with WELL-FORMED tensors that live on the host, under the tripwire library:
the wrapper must refuse them with ValueError (lwm_amd has no CPU path) and must not touch the library -- a wrapper that
forgets one device check hands a host pointer to a kernel.

The `data_ptr()` hand-offs of lwm_amd/*.py that are NOT behind a row of the table, and why:
  * llama_ops: y / rstd / nll / correct / dl / ws / dx / dw / da / db / qkv / g / d13 / out / ss_out / ys and every `_GEMV_WS`,
    `_WGRAD_WS` buffer -- allocated by the wrapper itself from the checked operands' shape and device;
    the saved tensors and `g.contiguous()` of every autograd backward -- handed over by autograd from a checked forward;
    `_as_dtype`, `_relayout`: `k.data_ptr()` is a cache KEY there, never dereferenced;
    dense / dense_multi / dense_fused / LLaMAMLP: plain torch GEMMs, except through gemv_multi (a row).
  * ops: `_cached_segment_blocks` -> segment_blocks on tensors `_base` has just checked (a row of its own too);
    o_parts / lse_parts / out / lse / delta / dq / dk / dv / *_acc when the wrapper allocates them; `_keep` hint tables.
  * ring_c: `_workspace` and `kv_keep_buffer` buffers are the ring's own; `_args` checks q / k / v / out / dout / lse /
    segment_ids / key_valid like ops._base does, but a CRing needs a process group -- tests/test_gpu_ring_c.py runs it.
  * llama.py: `w.data_ptr()` in `_norm_weight_bf16` is a cache key."""
import pytest
import torch

from tests import _boundary as Bd, _emu

ROWS = Bd.table()


@pytest.fixture()
def wire():
    # (the host emulator exports the same ABI: it answers the *_bytes / version queries the tripwire lets through)
    with Bd.tripwire(_emu.lib()) as w:
        yield w


@pytest.mark.parametrize("row", ROWS, ids=[r.name for r in ROWS])
def test_host_tensors_never_reach_the_library(row, wire):
    kw = row.make("cpu")
    if row.cpu == "torch":
        row.call(kw)                        # a torch expression: a result, and no library call
    else:
        with pytest.raises(ValueError):
            row.call(kw)
    assert wire.reached == []


def test_the_tripwire_trips_and_forwards_host_queries(wire):
    from lwm_amd import llama_ops, ops
    assert ops.lib() is wire and llama_ops.lib() is wire
    assert wire.lwm_version() >= 520 and wire.lwm_gemv_workspace_bytes(1, 256, 256) > 0
    with pytest.raises(AssertionError, match="reached the C library: lwm_rope_bf16"):
        wire.lwm_rope_bf16
    assert wire.reached == ["lwm_rope_bf16"]


def test_the_table_covers_every_public_wrapper_that_launches():
    """every public function of ops / llama_ops whose source mentions lib() is a row (or listed here with its reason)"""
    import inspect
    from lwm_amd import llama_ops, ops
    covered = {r.fn.__name__ for r in ROWS} | {r.name.split(" ")[0] for r in ROWS}      # (the norms go through adapters)
    exempt = {"use_tuned_gemms", "weights_changed", "precompute_freqs_cis",      # no tensors in
              "dense", "dense_multi", "dense_fused", "fused_dense_ok",           # torch GEMMs / gemv_multi (a row)
              "vision_text_loss",                                                # cross_entropy_loss_and_accuracy twice (a row)
              "kv8_dequant", "bwd_stats_shape"}                                  # torch expressions
    missing = []
    for mod in (ops, llama_ops):
        for name, f in vars(mod).items():
            if name.startswith("_") or not inspect.isfunction(f) or f.__module__ != mod.__name__ or name == "lib":
                continue
            if name not in covered and name not in exempt:
                missing.append(f"{mod.__name__}.{name}")
    assert missing == []
    assert {"RMSNorm", "rmsnorm_residual"} <= {r.name for r in ROWS}


def test_positions_broadcast_like_the_reference_gather():
    """_positions: (1,S) and (B,1) expand to (B,S) as jnp.take(freqs_cis, position_ids) broadcasts; what cannot is refused
    (device checks aside: they need a device and live in the GPU half)"""
    from lwm_amd.llama_ops import _positions
    B, S = 2, 5

    class Ref:                 # stands in for a device tensor: _positions reads .is_cuda and .device only
        is_cuda, device = True, torch.device("cpu")

    for bad in (torch.zeros(S, dtype=torch.int32), torch.zeros(B, S + 1, dtype=torch.int32), torch.zeros(B + 1, S, dtype=torch.int32),
                torch.zeros(B, S), torch.zeros(1, B, S, dtype=torch.int32)):
        with pytest.raises(ValueError, match="position_ids"):
            _positions(bad, B, S, Ref, "t")


CASES = Bd.cases()


@pytest.mark.parametrize("row,name,edit", CASES, ids=[f"{r.name}: {n}" for r, n, _ in CASES])
def test_every_bad_call_of_the_table_is_well_formed_and_stays_off_the_library(row, name, edit, wire):
    """the device half expects ValueError from the check the case aims at; on the host the device check fires first --
    this run proves that each edit applies to its row (no misspelt argument) and that nothing reaches the library"""
    kw = row.make("cpu")
    edit(kw, "cpu")
    try:
        row.call(kw)
    except ValueError:
        pass
    else:
        assert row.cpu == "torch", "a malformed call on the host came back without an error"
    assert wire.reached == []
