"""The operator-boundary table of tests/test_op_boundary.py (CPU) and tests/test_gpu_op_boundary.py (device), and the
tripwire library both run it under.  TEST INFRASTRUCTURE ONLY.

A row is one wrapper of lwm_amd.llama_ops / lwm_amd.ops that hands `tensor.data_ptr()` to the C library:

    Row(name, fn, make, bad, cpu="refuses")

make(dev) -> dict of keyword arguments of a WELL-FORMED call with every tensor on `dev`; bad: {case name: edit}, where
edit(kw, dev) changes the keyword arguments in place into a call the wrapper must refuse with ValueError BEFORE it touches
the library.  A new wrapper is one new row.

The tripwire stands in for lwm_amd._lib.lib(): it forwards the pure host queries of the ABI and raises AssertionError
for every other symbol, so a missing check fails an assertion and never sends a bad pointer to a device."""
import contextlib

import torch

HOST_QUERIES = ("lwm_version", "lwm_sizeof", "lwm_last_error")


class Tripwire:
    def __init__(self, real):
        """real: a bound library (the product's, or the host emulator's) that answers the host queries"""
        self._real = real
        self.reached = []

    def __getattr__(self, name):
        if name.endswith("_bytes") or name in HOST_QUERIES:
            return getattr(self._real, name)
        self.reached.append(name)
        raise AssertionError(f"reached the C library: {name}")


@contextlib.contextmanager
def tripwire(real):
    """lwm_amd.llama_ops.lib and lwm_amd.ops.lib (and the ring wrapper's) replaced by a Tripwire for the block"""
    from lwm_amd import llama_ops, ops, ring_c
    wire = Tripwire(real)
    saved = [(m, m.lib) for m in (llama_ops, ops, ring_c)]
    for m, _ in saved:
        m.lib = lambda: wire
    try:
        yield wire
    finally:
        for m, f in saved:
            m.lib = f


class Row:
    def __init__(self, name, fn, make, bad, cpu="refuses"):
        """cpu: what the wrapper does with well-formed CPU tensors -- "refuses" (ValueError) or "torch" (a documented
        route to a plain torch expression for operands the kernel does not serve: no library call either way)"""
        self.name, self.fn, self.make, self.bad, self.cpu = name, fn, make, bad, cpu

    def call(self, kw):
        return self.fn(**kw)


# ---------------------------------------------------------------- edits
def to_cpu(name):
    def edit(kw, dev):
        kw[name] = kw[name].cpu()
    return edit


def reshaped(name, shape):
    """the same dtype and device, another shape (filled with zeros)"""
    def edit(kw, dev):
        t = kw[name]
        kw[name] = torch.zeros(shape, dtype=t.dtype, device=t.device)
    return edit


def cast(name, dtype):
    def edit(kw, dev):
        kw[name] = kw[name].to(dtype)
    return edit


def item(name, i, f):
    """kw[name] is a list / tuple: element i replaced by f(element)"""
    def edit(kw, dev):
        seq = list(kw[name])
        seq[i] = f(seq[i])
        kw[name] = type(kw[name])(seq)
    return edit


def dev_and_shape(name, shape):
    """the two standard cases of an optional tensor argument"""
    return {f"{name} on the host": to_cpu(name), f"{name} of shape {tuple(shape)}": reshaped(name, shape)}


def _gen(seed=0):
    return torch.Generator().manual_seed(seed)


def _bf(shape, dev, seed=0):
    return torch.randn(*shape, generator=_gen(seed)).to(torch.bfloat16).to(dev)


def _f(shape, dev, seed=0):
    return torch.randn(*shape, generator=_gen(seed)).to(dev)


def _zeros(shape, dtype, dev):
    return torch.zeros(shape, dtype=dtype, device=dev)


# ---------------------------------------------------------------- lwm_amd.llama_ops
def _llama_rows():
    from lwm_amd import llama_ops as LO
    rows = []
    B, S, H, D, d, P = 2, 16, 2, 64, 128, 64

    def ramp(dev):
        # (not arange: a read at another row offset changes the answer)
        return ((torch.arange(S)[None] * 3 + torch.tensor([[5], [11]])) % P).to(torch.int32).to(dev)

    rope_bad = {
        "position_ids on the host": to_cpu("position_ids"),
        "position_ids (S,)": reshaped("position_ids", (S,)),
        "position_ids (B, S+1)": reshaped("position_ids", (B, S + 1)),
        "position_ids (B+1, S)": reshaped("position_ids", (B + 1, S)),
        "position_ids float": cast("position_ids", torch.float32),
        "freqs_cis with a last dimension of 3": reshaped("freqs_cis", (P, D // 2, 3)),
        "freqs_cis for another head_dim": reshaped("freqs_cis", (P, D // 4, 2)),
        "freqs_cis on the host": to_cpu("freqs_cis"),
        "freqs_cis float64": cast("freqs_cis", torch.float64),
    }
    rows.append(Row("qkv_rope", LO.qkv_rope,
                    lambda dev: dict(x=_bf((B, S, d), dev, 1), wq=_bf((d, H * D), dev, 2) * 0.1, wk=_bf((d, H * D), dev, 3) * 0.1,
                                     wv=_bf((d, H * D), dev, 4) * 0.1, freqs_cis=LO.precompute_freqs_cis(D, P, device=dev),
                                     position_ids=ramp(dev), num_heads=H),
                    dict(rope_bad, **{"wk on the host": to_cpu("wk"), "wv of another shape": reshaped("wv", (d, H * D - 8)),
                                      "x float32": cast("x", torch.float32)})))
    rows.append(Row("apply_rotary_emb", LO.apply_rotary_emb,
                    lambda dev: dict(xq=_bf((B, S, H, D), dev, 1), xk=_bf((B, S, H, D), dev, 2),
                                     freqs_cis=LO.precompute_freqs_cis(D, P, device=dev), position_ids=ramp(dev)),
                    dict(rope_bad, **{"xk on the host": to_cpu("xk"), "xk of another length": reshaped("xk", (B, S + 1, H, D))})))

    C = 256

    def rmsnorm(x, weight):
        m = LO.RMSNorm(C, dtype=x.dtype)
        m.kernel = torch.nn.Parameter(weight)
        return m(x)

    def rmsnorm_res(x, weight):
        m = LO.RMSNorm(C, dtype=x.dtype)
        m.kernel = torch.nn.Parameter(weight)
        return LO.rmsnorm_residual(m, x)

    norm_bad = {"weight on the host": to_cpu("weight"), "weight of C - 8 elements": reshaped("weight", (C - 8,)),
                "weight of 2C elements": reshaped("weight", (2 * C,))}
    norm_make = lambda dev: dict(x=_bf((3, 5, C), dev, 1), weight=_f((C,), dev, 2))
    rows.append(Row("RMSNorm", rmsnorm, norm_make, norm_bad))
    rows.append(Row("rmsnorm_residual", rmsnorm_res, norm_make, dict(norm_bad, **{"x float32": cast("x", torch.float32)})))

    rows.append(Row("swiglu", LO.swiglu, lambda dev: dict(a=_bf((4, 64), dev, 1), b=_bf((4, 64), dev, 2)),
                    {"b of another shape": reshaped("b", (4, 56)), "b on the host": to_cpu("b"),
                     "b transposed in shape": reshaped("b", (64, 4)), "b float32": cast("b", torch.float32)}))
    rows.append(Row("swiglu_halves", LO.swiglu_halves, lambda dev: dict(y13=_bf((4, 128), dev, 1)),
                    {"F not a multiple of 8": reshaped("y13", (4, 24)), "float32": cast("y13", torch.float32)}))

    V = 64

    def tokens(dev):
        return torch.randint(0, V, (B, S), generator=_gen(3)).to(dev)

    def valid(dev):
        return (torch.rand(B, S, generator=_gen(4)) > 0.2).to(torch.float32).to(dev)

    loss_bad = {"tokens of another numel": reshaped("tokens", (B, S + 1)), "tokens transposed": reshaped("tokens", (S, B)),
                "tokens on the host": to_cpu("tokens"), "tokens float": cast("tokens", torch.float32),
                "valid of another shape": reshaped("valid", (B, S - 1)), "valid on the host": to_cpu("valid")}
    rows.append(Row("cross_entropy_loss_and_accuracy", LO.cross_entropy_loss_and_accuracy,
                    lambda dev: dict(logits=_bf((B, S, V), dev, 1), tokens=tokens(dev), valid=valid(dev), sp_sharded=False),
                    loss_bad))
    rows.append(Row("chunked_lm_head_loss", LO.chunked_lm_head_loss,
                    lambda dev: dict(hidden=_bf((B, S, d), dev, 1), lm_head_kernel=_bf((d, V), dev, 2) * 0.1, tokens=tokens(dev),
                                     valid=valid(dev), chunk=8, sp_sharded=False),
                    dict(loss_bad, **{"lm_head_kernel on the host": to_cpu("lm_head_kernel"),
                                      "lm_head_kernel of another d_model": reshaped("lm_head_kernel", (d - 8, V))})))

    K, N = 256, 256
    kern = lambda dev, n=1: [_bf((K, N), dev, 10 + i) * 0.1 for i in range(n)]
    rows.append(Row("gemv", LO.gemv, lambda dev: dict(x=_bf((2, K), dev, 1), kernel=kern(dev)[0]),
                    {"kernel on the host": to_cpu("kernel"), "kernel of another K": reshaped("kernel", (K - 32, N)),
                     "x on the host": to_cpu("x")}))
    rows.append(Row("gemv_multi", LO.gemv_multi, lambda dev: dict(x=_bf((2, K), dev, 1), kernels=kern(dev, 3)),
                    {"kernels[1] on the host": item("kernels", 1, lambda t: t.cpu()),
                     "kernels[2] of another K": item("kernels", 2, lambda t: t[:K - 32].contiguous()),
                     "four kernels": lambda kw, dev: kw.update(kernels=kw["kernels"] + kw["kernels"][:1]),
                     "out_dtype float16": lambda kw, dev: kw.update(out_dtype=torch.float16)}))
    rows.append(Row("gemv_fused (norm on load)", LO.gemv_fused,
                    lambda dev: dict(x=_bf((2, K), dev, 1), kernels=kern(dev, 2),
                                     norm=(_f((2, 2), dev, 5).abs() + 1.0, _bf((K,), dev, 6), 1e-6)),
                    {"kernels[0] on the host": item("kernels", 0, lambda t: t.cpu()),
                     "ss on the host": item("norm", 0, lambda t: t.cpu()),
                     "ss of another row count": item("norm", 0, lambda t: t[:1].contiguous()),
                     "norm weight on the host": item("norm", 1, lambda t: t.cpu()),
                     "norm weight of K - 8 elements": item("norm", 1, lambda t: t[:K - 8].contiguous())}))
    rows.append(Row("gemv_fused (residual, ss out)", LO.gemv_fused,
                    lambda dev: dict(x=_bf((2, K), dev, 1), kernels=kern(dev, 1), residual=_bf((2, N), dev, 7), want_ss=True),
                    {"kernels[0] on the host": item("kernels", 0, lambda t: t.cpu()),
                     "residual on the host": to_cpu("residual"), "residual of another shape": reshaped("residual", (2, N - 8))}))

    # transpose2d / wgrad serve what lwm_transpose_bf16 / lwm_wgrad_bf16 take and hand anything else to torch
    rows.append(Row("transpose2d", LO.transpose2d,
                    lambda dev: dict(src=_bf((64, 128), dev, 1), out=_zeros((128, 64), torch.bfloat16, dev)),
                    {"out on the host": to_cpu("out"), "out of another shape": reshaped("out", (128, 32)),
                     "out float32": cast("out", torch.float32)}, cpu="torch"))
    rows.append(Row("wgrad", LO.wgrad, lambda dev: dict(x2=_bf((64, 256), dev, 1), g2=_bf((64, 256), dev, 2)),
                    {"g2 on the host": to_cpu("g2"), "g2 of another row count": reshaped("g2", (32, 256)),
                     "g2 float32": cast("g2", torch.float32)}, cpu="torch"))
    return rows


# ---------------------------------------------------------------- lwm_amd.ops
def _ops_rows():
    from lwm_amd import ops
    rows = []
    B, Sq, Sk, H, D = 2, 64, 96, 2, 128
    i32, u8, f32, bf16 = torch.int32, torch.uint8, torch.float32, torch.bfloat16

    def qkv(dev, dtype=bf16):
        return dict(q=_f((B, Sq, H, D), dev, 1).to(dtype), k=_f((B, Sk, H, D), dev, 2).to(dtype), v=_f((B, Sk, H, D), dev, 3).to(dtype))

    def masks(dev):
        seg = lambda L: (torch.arange(L)[None].expand(B, L) // 40).to(i32).contiguous().to(dev)
        kv = torch.ones(B, Sk, dtype=u8)
        kv[:, :3] = 0
        return dict(seg_q=seg(Sq), seg_k=seg(Sk), key_valid=kv.to(dev), causal=True, q_start=Sk - Sq)

    qkv_bad = {"k on the host": to_cpu("k"), "v of another length": reshaped("v", (B, Sk - 32, H, D)),
               "k of another head count": reshaped("k", (B, Sk, H + 1, D)), "v float32": cast("v", f32)}
    mask_bad = dict(**dev_and_shape("seg_q", (B, Sq + 1)), **dev_and_shape("seg_k", (B, Sk - 1)),
                    **dev_and_shape("key_valid", (B, Sk + 32)), **{"seg_k int64": cast("seg_k", torch.int64)})

    rows.append(Row("attn_fwd_block (final)", ops.attn_fwd_block,
                    lambda dev: dict(qkv(dev), **masks(dev), out=_zeros((B, Sq, H, D), bf16, dev), lse=_zeros((B, H, Sq), f32, dev)),
                    dict(qkv_bad, **mask_bad, **dev_and_shape("out", (B, Sq + 64, H, D)), **dev_and_shape("lse", (B, H, Sq + 64)),
                         **{"out float32": cast("out", f32)})))
    rows.append(Row("attn_fwd_block (carry)", ops.attn_fwd_block,
                    lambda dev: dict(qkv(dev), causal=False, final=False, carry_in=False,
                                     out_acc=_zeros((B, Sq, H, D), f32, dev), lse_acc=_zeros((B, H, Sq), f32, dev)),
                    dict(**dev_and_shape("out_acc", (B, Sq, H + 1, D)), **dev_and_shape("lse_acc", (B, Sq, H)))))

    def dmask(dev):
        return dict(qkv(dev), causal=False, dense_mask=torch.ones(B, Sq, Sk, dtype=u8).to(dev))

    rows.append(Row("attn_fwd_splitk", ops.attn_fwd_splitk, lambda dev: dict(dmask(dev), k_splits=2),
                    dict(qkv_bad, **dev_and_shape("dense_mask", (B, Sq + 1, Sk)), **{"q float32": cast("q", f32)})))

    def parts(dev):
        P = 2
        return dict(o_parts=_f((P, B, Sq, H, D), dev, 1), lse_parts=_f((P, B, H, Sq), dev, 2),
                    out=_zeros((B, Sq, H, D), bf16, dev), lse=_zeros((B, H, Sq), f32, dev))

    rows.append(Row("attn_combine", ops.attn_combine, parts,
                    dict(**dev_and_shape("lse_parts", (3, B, H, Sq)), **dev_and_shape("out", (B, Sq + 64, H, D)),
                         **dev_and_shape("lse", (B, H, Sq + 64)), **{"o_parts on the host": to_cpu("o_parts")})))

    def parts_f32(dev):
        kw = parts(dev)
        del kw["out"]
        return dict(kw, want_bf16=False, out_f32=_zeros((B, Sq, H, D), f32, dev))

    rows.append(Row("attn_combine (f32 out)", ops.attn_combine, parts_f32, dev_and_shape("out_f32", (B, Sq + 64, H, D))))

    def bwd(dev):
        return dict(qkv(dev), **masks(dev), dout=_bf((B, Sq, H, D), dev, 4), lse=_f((B, H, Sq), dev, 5),
                    delta=_zeros(ops.bwd_stats_shape(B, H, Sq), f32, dev))

    bwd_bad = dict(qkv_bad, **mask_bad, **dev_and_shape("dout", (B, Sq - 32, H, D)), **dev_and_shape("lse", (B, H, Sq - 32)),
                   **dev_and_shape("delta", (B, H, 2, 32)))
    rows.append(Row("attn_bwd_delta", ops.attn_bwd_delta,
                    lambda dev: dict(out=_bf((B, Sq, H, D), dev, 1), dout=_bf((B, Sq, H, D), dev, 2), lse=_f((B, H, Sq), dev, 3),
                                     delta=_zeros(ops.bwd_stats_shape(B, H, Sq), f32, dev)),
                    dict(**dev_and_shape("dout", (B, Sq + 64, H, D)), **dev_and_shape("lse", (B, H, Sq + 1)),
                         **dev_and_shape("delta", (B, H, 2, 32)), **{"dout float32": cast("dout", f32)})))
    rows.append(Row("attn_bwd_dq_block (final)", ops.attn_bwd_dq_block,
                    lambda dev: dict(bwd(dev), dq=_zeros((B, Sq, H, D), bf16, dev)),
                    dict(bwd_bad, **dev_and_shape("dq", (B, Sq + 64, H, D)))))
    rows.append(Row("attn_bwd_dq_block (carry)", ops.attn_bwd_dq_block,
                    lambda dev: dict(bwd(dev), final=False, dq_acc=_zeros((B, H, Sq, D), f32, dev), acc_head_major=True),
                    dev_and_shape("dq_acc", (B, Sq, H, D))))
    rows.append(Row("attn_bwd_dkdv_block (final)", ops.attn_bwd_dkdv_block,
                    lambda dev: dict(bwd(dev), dk=_zeros((B, Sk, H, D), bf16, dev), dv=_zeros((B, Sk, H, D), bf16, dev)),
                    dict(bwd_bad, **dev_and_shape("dk", (B, Sk + 32, H, D)), **dev_and_shape("dv", (B, Sq, H, D)))))
    rows.append(Row("attn_bwd_dkdv_block (carry)", ops.attn_bwd_dkdv_block,
                    lambda dev: dict(bwd(dev), final=False, dk_acc=_zeros((B, Sk, H, D), f32, dev),
                                     dv_acc=_zeros((B, Sk, H, D), f32, dev)),
                    dict(**dev_and_shape("dk_acc", (B, Sq, H, D)), **dev_and_shape("dv_acc", (B, Sk, H + 1, D)))))
    rows.append(Row("segment_blocks", ops.segment_blocks,
                    lambda dev: dict(seg=masks(dev)["seg_k"], valid=masks(dev)["key_valid"]),
                    dict(**dev_and_shape("valid", (B, Sk - 1)), **{"seg int64": cast("seg", torch.int64)})))

    # KV caches
    R = 32
    rows.append(Row("kv_cache_write", ops.kv_cache_write,
                    lambda dev: dict(cache=_zeros((B, R, H, D), bf16, dev), src=_bf((B, 8, H, D), dev, 1), dst_row0=5),
                    {"src on the host": to_cpu("src"), "src of another head count": reshaped("src", (B, 8, H + 1, D)),
                     "src of another batch": reshaped("src", (B + 1, 8, H, D)),
                     "rows past the end": lambda kw, dev: kw.update(dst_row0=R - 4),
                     "negative source row": lambda kw, dev: kw.update(src_row0=-1, nrows=4)}))
    rows.append(Row("kv_cache_write_at", ops.kv_cache_write_at,
                    lambda dev: dict(cache=_zeros((B, R, H, D), bf16, dev), src=_bf((B, 8, H, D), dev, 1),
                                     index_dev=torch.tensor([5], dtype=i32).to(dev)),
                    {"src on the host": to_cpu("src"), "src of another head count": reshaped("src", (B, 8, H + 1, D)),
                     "index on the host": to_cpu("index_dev"), "index of two elements": reshaped("index_dev", (2,)),
                     "index int64": cast("index_dev", torch.int64)}))

    def kv8(dev):
        return dict(cache=_zeros((B, R, H, D), u8, dev), scale=torch.ones(B, R, H).to(dev), src=_bf((B, 8, H, D), dev, 1))

    kv8_bad = dict(**dev_and_shape("scale", (B, R, H + 1)), **dev_and_shape("src", (B, 8, H + 1, D)),
                   **{"cache on the host": to_cpu("cache"), "src float32": cast("src", f32)})
    rows.append(Row("kv8_cache_write", ops.kv8_cache_write, lambda dev: dict(kv8(dev), dst_row0=5),
                    dict(kv8_bad, **{"rows past the end": lambda kw, dev: kw.update(dst_row0=R - 4)})))
    rows.append(Row("kv8_cache_write_at", ops.kv8_cache_write_at,
                    lambda dev: dict(kv8(dev), index_dev=torch.tensor([5], dtype=i32).to(dev)),
                    dict(kv8_bad, **{"index on the host": to_cpu("index_dev"), "index of two elements": reshaped("index_dev", (2,))})))
    rows.append(Row("attn_decode_kv8", ops.attn_decode_kv8,
                    lambda dev: dict(q=_bf((B, 1, H, D), dev, 1), cached_key=torch.full((B, R, H, D), 0x38, dtype=u8).to(dev),
                                     key_scale=torch.ones(B, R, H).to(dev), cached_value=torch.full((B, R, H, D), 0x38, dtype=u8).to(dev),
                                     value_scale=torch.ones(B, R, H).to(dev), dense_mask=torch.ones(B, 1, R, dtype=u8).to(dev),
                                     k_splits=2),
                    dict(**dev_and_shape("cached_key", (B, R + 1, H, D)), **dev_and_shape("cached_value", (B, R, H + 1, D)),
                         **dev_and_shape("key_scale", (B, R, H + 1)), **dev_and_shape("value_scale", (B, R - 1, H)),
                         **dev_and_shape("dense_mask", (B, 1, R + 8)), **{"two queries": reshaped("q", (B, 2, H, D))})))

    # casts and sums
    rows.append(Row("cast_f32_to_bf16", ops.cast_f32_to_bf16,
                    lambda dev: dict(src=_f((4, 64), dev, 1), dst=_zeros((4, 64), bf16, dev)),
                    dict(**dev_and_shape("dst", (4, 56)), **{"dst float32": cast("dst", f32)})))
    rows.append(Row("sum_f32_to_bf16", ops.sum_f32_to_bf16,
                    lambda dev: dict(srcs=[_f((4, 64), dev, i) for i in range(3)], dst=_zeros((4, 64), bf16, dev)),
                    dict(**dev_and_shape("dst", (4, 56)), **{"srcs[1] on the host": item("srcs", 1, lambda t: t.cpu()),
                                                             "srcs[2] of another shape": item("srcs", 2, lambda t: t[:2].contiguous())})))

    # VQGAN primitives
    Cin, Cout = 32, 64
    rows.append(Row("conv2d_nhwc", ops.conv2d_nhwc,
                    lambda dev: dict(x=_f((1, 8, 8, Cin), dev, 1), w=_f((3, 3, Cin, Cout), dev, 2) * 0.1, bias=_f((Cout,), dev, 3),
                                     residual=_f((1, 8, 8, Cout), dev, 4), out=_zeros((1, 8, 8, Cout), f32, dev)),
                    dict(**dev_and_shape("bias", (Cout - 8,)), **dev_and_shape("residual", (1, 8, 4, Cout)),
                         **dev_and_shape("out", (1, 8, 4, Cout)), **dev_and_shape("w", (3, 3, Cin + 8, Cout)))))
    rows.append(Row("groupnorm_silu", ops.groupnorm_silu,
                    lambda dev: dict(x=_f((1, 8, 8, 128), dev, 1), gamma=_f((128,), dev, 2), beta=_f((128,), dev, 3),
                                     out=_zeros((1, 8, 8, 128), f32, dev)),
                    dict(**dev_and_shape("gamma", (96,)), **dev_and_shape("beta", (256,)),
                         **dev_and_shape("out", (1, 8, 4, 128)), **{"groups that do not divide C": lambda kw, dev: kw.update(groups=24)})))
    E, De = 128, 64
    rows.append(Row("vq_sqnorm", ops.vq_sqnorm, lambda dev: dict(codebook=_f((E, De), dev, 1)), {"float64": cast("codebook", torch.float64)}))
    rows.append(Row("vq_argmin", ops.vq_argmin,
                    lambda dev: dict(z=_f((2, 5, De), dev, 1), codebook=_f((E, De), dev, 2), se=_f((E,), dev, 3).abs()),
                    dict(**dev_and_shape("se", (E - 1,)), **dev_and_shape("codebook", (E, De + 8)))))
    rows.append(Row("vq_gather", ops.vq_gather,
                    lambda dev: dict(codebook=_f((E, De), dev, 1), idx=torch.randint(0, E, (2, 5), generator=_gen(2)).to(i32).to(dev),
                                     z=_f((2, 5, De), dev, 3)),
                    dict(**dev_and_shape("z", (2, 4, De)), **{"idx on the host": to_cpu("idx"), "idx int64": cast("idx", torch.int64)})))

    # sampler
    Bs, V = 2, 512
    rows.append(Row("sample_tokens", ops.sample_tokens,
                    lambda dev: dict(logits=_f((2 * Bs, V), dev, 1), temperature=1.0, top_k=8, seed=7,
                                     step_dev=torch.tensor([3], dtype=i32).to(dev), cfg_scale=torch.full((Bs,), 2.0).to(dev),
                                     done=_zeros((Bs,), u8, dev), eos=1, tokens_out=_zeros((2 * Bs, 1), torch.int64, dev), copies=2,
                                     seq_out=_zeros((Bs, 8), torch.int64, dev)),
                    dict(**dev_and_shape("cfg_scale", (Bs + 1,)), **dev_and_shape("step_dev", (2,)), **dev_and_shape("done", (Bs + 1,)),
                         **dev_and_shape("tokens_out", (Bs, 1)), **dev_and_shape("seq_out", (Bs + 1, 8)),
                         **{"logits float64": cast("logits", torch.float64)})))
    return rows


def table():
    return _llama_rows() + _ops_rows()


def cases():
    """[(row, case name, edit)] over the whole table"""
    return [(r, n, e) for r in table() for n, e in r.bad.items()]
