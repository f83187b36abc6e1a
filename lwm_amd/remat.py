"""Per-block activation recompute for the training path (the reference remats its block internals: lwm/llama.py:553,
:674-678).  A block run through `remat_block` keeps, between its forward and its backward, its input `x` and what the
attention op saves beyond q | k | v -- `out` and the log-sum-exp(s) -- and nothing else; the backward runs the block a
second time on a detached `x`, back-propagates through that graph and drops it before it returns, so the live set of a
step is ONE layer's activations whatever the depth.

No kernel of its own: the recompute is the block's own operators run again (RMSNorm, the QKV GEMM + RoPE, wo, w1 | w3,
SwiGLU, w2).  The attention forward is NOT among them: the two attention Functions (lwm_amd.ring._RingAttention,
lwm_amd.ring_c._RingAttentionC) hand their `out` / lse to `attention_record` while a remat block's no-grad forward runs
and ask `attention_replay` for them during the recompute, where they save the recomputed q, k, v beside the recorded
results and launch (and, on a ring, send) nothing.  An attention call that does not go through one of the two has nothing
to replay and simply runs again: correct, slower, no error.  The MLP's own chunk checkpoint
(ringattention.blockwise_feedforward) is off inside the recompute (`recomputing()`): the chunk loop stays, so the GEMMs
see the shapes of the forward, and the MLP runs twice, not three times.

The switch is LLaMAForCausalLM.remat_blocks / LWM_REMAT_BLOCK; this module imports nothing of the package."""
from __future__ import annotations

import contextlib
import threading

import torch

ENV = "LWM_REMAT_BLOCK"
# a step of this many rows or fewer is a decode step: under no_grad its projections leave the library GEMMs
# (llama_ops._decode_rows, at most 32 rows), so the no-grad forward would not be the forward of the un-remat path
MIN_ROWS = 33


def parse_remat_block(value, what=ENV):
    """None / "" / "0" / 0 / False -> False; "1" / 1 / True -> True; anything else is refused"""
    if value is None or value is False or value == "" or value == "0" or (isinstance(value, int) and value == 0):
        return False
    if value is True or value == "1" or (isinstance(value, int) and value == 1):
        return True
    raise ValueError(f"{what}={value!r}: 1 (every block keeps its input and the attention op's out / lse and recomputes the "
                     f"rest in the backward) or 0 / unset (off)")


def saved_bytes(B, S, d, H, dtype, n_lse=1):
    """Bytes one block keeps between its forward and its backward: `x` and the attention `out`, (B, S, d) of `dtype`
    each, and n_lse f32 (B, H, S) log-sum-exps -- B * S * (4 d + 4 H) for a bf16 model on one rank."""
    item = torch.empty((), dtype=dtype).element_size()
    return int(B) * int(S) * (2 * int(d) * item + 4 * int(H) * int(n_lse))


# ----------------------------------------------------------------- record / replay of the attention op's results
class _Tape:
    def __init__(self, mode, items=None):
        self.mode, self.items, self.pos = mode, ([] if items is None else items), 0


_tls = threading.local()       # (the backward runs on autograd's thread: the tape belongs to the thread that runs the block)


@contextlib.contextmanager
def _scope(tape):
    prev = getattr(_tls, "tape", None)
    _tls.tape = tape
    try:
        yield tape
    finally:
        _tls.tape = prev


def recomputing():
    """True while a remat block's backward runs the block again"""
    t = getattr(_tls, "tape", None)
    return t is not None and t.mode == "replay"


def attention_record(out, lses):
    """called by an attention Function's forward with what it saves beyond q, k, v"""
    t = getattr(_tls, "tape", None)
    if t is not None and t.mode == "record":
        t.items.append((out, tuple(lses)))


def attention_replay(q):
    """-> (out, [lse, ...]) of the same call site's recorded forward, or None (not in a recompute, or nothing recorded
    for this call: the caller runs its forward).  `out` comes back as a fresh alias: the Function that returns it
    writes its graph node onto the alias, not onto the kept tensor."""
    t = getattr(_tls, "tape", None)
    if t is None or t.mode != "replay" or t.pos >= len(t.items):
        return None
    out, lses = t.items[t.pos]
    if out.shape != q.shape or out.dtype != q.dtype or out.device != q.device:
        return None
    t.pos += 1
    return out.detach(), list(lses)


# ----------------------------------------------------------------- the block
class _RematBlock(torch.autograd.Function):
    """y = blk(x, *args).  The parameters are inputs (a block whose input needs no gradient still owes them theirs), their
    gradients are RETURNED: accumulation into .grad is autograd's own, as without remat."""

    @staticmethod
    def forward(ctx, blk, args, x, *params):
        with _scope(_Tape("record")) as tape, torch.no_grad():
            y = blk(x, *args)
        ctx.blk, ctx.args = blk, args
        ctx.n_lse = [len(lses) for _, lses in tape.items]
        # saved through autograd: freed after the backward unless the graph is retained, so a second backward() is
        # autograd's own named error -- or, with retain_graph=True, a second recompute with the same results
        ctx.save_for_backward(x, *(t for out, lses in tape.items for t in (out, *lses)))
        return y

    @staticmethod
    def backward(ctx, dout):
        x, *flat = ctx.saved_tensors
        items = []
        for n in ctx.n_lse:
            items.append((flat[0], tuple(flat[1:1 + n])))
            flat = flat[1 + n:]
        need_x, need_p = ctx.needs_input_grad[2], ctx.needs_input_grad[3:]
        params = list(ctx.blk.parameters())
        xd = x.detach().requires_grad_(need_x)
        with _scope(_Tape("replay", items)), torch.enable_grad():
            y = ctx.blk(xd, *ctx.args)
        inputs = ([xd] if need_x else []) + [p for p, need in zip(params, need_p) if need]
        grads = list(torch.autograd.grad(y, inputs, dout, allow_unused=True))     # (frees the recompute graph as it goes)
        del y
        dx = grads.pop(0) if need_x else None
        dps = [grads.pop(0) if need else None for need in need_p]
        return (None, None, dx, *dps)


def applies(blk, x):
    """Whether a block call is recomputed when the switch is on: autograd is recording, something in it wants a
    gradient, no hipGraph capture is under way, and it is not a decode-sized step (MIN_ROWS)."""
    if not torch.is_grad_enabled() or x.numel() // max(x.shape[-1], 1) < MIN_ROWS:
        return False
    if not (x.requires_grad or any(p.requires_grad for p in blk.parameters())):
        return False
    return not (x.is_cuda and torch.cuda.is_current_stream_capturing())


def remat_block(blk, x, freqs_cis, attention_mask=None, segment_ids=None, position_ids=None, layout=None):
    """blk(x, freqs_cis, attention_mask, segment_ids, position_ids, None, layout) -- the uncached call -- keeping only `x`
    and the attention op's out / lse; the mask arguments are held by reference."""
    args = (freqs_cis, attention_mask, segment_ids, position_ids, None, layout)
    return _RematBlock.apply(blk, args, x, *blk.parameters())
