"""Model HARNESS: the LLaMA transformer of lwm/llama.py assembled from this package's
operators, so that the hot path can be validated and timed in its real position
(BASELINE config #1: 2-layer slice of LWM-7B, S = 4096).  It is not a product subsystem of
its own: every projection is a plain library GEMM (hipBLASLt through torch.matmul), the
embedding a gather; what is hand-written HIP is what sits between them -- RMSNorm, RoPE,
RingAttention, the SwiGLU gate, the chunked lm_head loss.

Names, parameter layouts and config knobs follow the reference: flax Dense kernels are
(in, out) (lwm/llama.py:390-421, :631-655); `wte`, `h.<i>.attention.{wq,wk,wv,wo}`,
`h.<i>.feed_forward.{w1,w2,w3}`, `h.<i>.{attention_norm,ffn_norm}.kernel`, `ln_f.kernel`,
`lm_head.kernel` (lwm/llama.py:664-744, :982-1106).
"""
from __future__ import annotations

import os

import torch

from . import kv4 as _kv4, kv6 as _kv6, dropout as _dropout, llama_ops as _lo, ops as _ops, remat as _remat
from .llama_ops import (LLaMAMLP, RMSNorm, apply_rotary_emb, chunked_lm_head_loss, decode_rows_scope, dense, dense_fused,
                        dense_multi, fused_dense_ok, parse_decode_rows, precompute_freqs_cis, qkv_rope, rmsnorm_residual,
                        rows_x_ok, swiglu)
from .ringattention import (blockwise_feedforward, concatenate_to_cache, ringattention,
                            ringattention_inference, sp_layout_is_explicit, sp_positions, sp_size_rank)
from .wpack import FORMATS

# The model sizes of lwm/llama.py:33-130:
# name: (hidden, intermediate, layers, heads, max_sequence_length, rms_norm_eps)
_SIZES = {"200m": (1024, 2048, 14, 8, 2048, 1e-6), "1b": (2048, 5504, 22, 16, 2048, 1e-6),
          "3b": (3200, 8640, 26, 32, 2048, 1e-6), "7b": (4096, 11008, 32, 32, 4096, 1e-6),
          "13b": (5120, 13824, 40, 40, 2048, 1e-6), "30b": (6656, 17920, 60, 52, 2048, 1e-6),
          "65b": (8192, 22016, 80, 64, 2048, 1e-5), "debug": (256, 256, 2, 2, 2048, 1e-6)}
LLAMA_STANDARD_CONFIGS = {
    name: dict(vocab_size=32000, hidden_size=d, intermediate_size=f, num_hidden_layers=L, num_attention_heads=h,
               max_sequence_length=s, initializer_range=0.02, rms_norm_eps=eps, use_cache=True,
               tie_word_embeddings=False)
    for name, (d, f, L, h, s, eps) in _SIZES.items()}


def parse_config_updates(text):
    """`--update_llama_config` (lwm/train.py:120-121, scripts/run_*.sh): a string such as
    "dict(theta=10000000,max_sequence_length=131072,scan_attention=True)" or a dict literal.
    The reference eval()s it; here only `dict(name=literal, ...)` / `{...}` of Python literals is
    accepted."""
    import ast
    text = text.strip()
    if not text:
        return {}
    node = ast.parse(text, mode="eval").body
    if isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id == "dict" and not node.args:
        out = {}
        for kw in node.keywords:
            if kw.arg is None:
                raise ValueError("update_llama_config: **expansion is not accepted")
            out[kw.arg] = ast.literal_eval(kw.value)
        return out
    val = ast.literal_eval(node)
    if not isinstance(val, dict):
        raise ValueError("update_llama_config must be dict(...) or a dict literal")
    return val


class LLaMAConfig:
    """lwm/llama.py:133-199: same field names and defaults.  resid_pdrop and embd_pdrop are honoured by a training-mode
    forward (DropoutState below); attn_pdrop > 0 is refused there: the reference hands it to a package that is not part
    of it."""

    def __init__(self, vocab_size=32000, hidden_size=4096, intermediate_size=11008, num_hidden_layers=32,
                 num_attention_heads=32, max_sequence_length=4096, rms_norm_eps=1e-6, initializer_range=0.02,
                 use_cache=True, bos_token_id=0, eos_token_id=1, resid_pdrop=0.0, embd_pdrop=0.0, attn_pdrop=0.0,
                 tie_word_embeddings=False, scan_attention=True, scan_mlp=True, scan_query_chunk_size=1024,
                 scan_key_chunk_size=1024, scan_mlp_chunk_size=1024, scan_layers=True, param_scan_axis=0, mesh_dim=None,
                 theta=10000, **kwargs):
        # (every keyword and default of the reference's signature -- tests/test_golden.py holds them to the reference's own
        # __init__; scan_layers / param_scan_axis describe the checkpoint layout)
        self.vocab_size, self.hidden_size, self.intermediate_size = vocab_size, hidden_size, intermediate_size
        self.num_hidden_layers, self.num_attention_heads = num_hidden_layers, num_attention_heads
        self.max_sequence_length, self.rms_norm_eps = max_sequence_length, rms_norm_eps
        self.initializer_range = initializer_range
        self.use_cache, self.bos_token_id, self.eos_token_id = use_cache, bos_token_id, eos_token_id
        self.resid_pdrop, self.embd_pdrop, self.attn_pdrop = resid_pdrop, embd_pdrop, attn_pdrop
        self.tie_word_embeddings = tie_word_embeddings
        self.scan_attention, self.scan_mlp = scan_attention, scan_mlp
        self.scan_query_chunk_size, self.scan_key_chunk_size = scan_query_chunk_size, scan_key_chunk_size
        self.scan_mlp_chunk_size, self.theta = scan_mlp_chunk_size, theta
        self.scan_layers, self.param_scan_axis, self.mesh_dim = scan_layers, param_scan_axis, mesh_dim
        for k, v in kwargs.items():
            setattr(self, k, v)
        self._validate()

    def _validate(self):
        """The attention kernels are written for head_dim 128 (LWM-7B, lwm/llama.py:70-81; also the 13b /
        30b / 65b sizes).  A size they cannot run -- the 3b table entry has head_dim 100 -- is refused
        here, when the config is made, not at the first kernel launch."""
        h, d = self.num_attention_heads, self.hidden_size
        if h <= 0 or d % h or d // h != 128:
            raise NotImplementedError(
                f"hidden_size {d} / num_attention_heads {h}: head_dim must be 128 for the MI355X attention "
                f"kernels (lwm_amd/csrc/attn_common.h); this is the '3b' entry of the reference's size table")

    def update(self, updates):
        """ConfigDict-style in-place update; a string is parsed like --update_llama_config."""
        if isinstance(updates, str):
            updates = parse_config_updates(updates)
        for k, v in dict(updates).items():
            setattr(self, k, v)
        self._validate()
        return self

    def to_dict(self):
        return {k: v for k, v in vars(self).items() if not k.startswith("_")}

    @classmethod
    def from_dict(cls, d):
        return cls(**dict(d))

    @classmethod
    def load_config(cls, path, **updates):
        """lwm/llama.py:300-312: a standard size name, 'json::<file>' or 'pickle::<file>' (the latter
        holds {'llama_config': {...}})."""
        if path in LLAMA_STANDARD_CONFIGS:
            cfg = dict(LLAMA_STANDARD_CONFIGS[path])
        else:
            if "::" not in path:
                raise ValueError(f"unknown model size {path!r}; expected one of {sorted(LLAMA_STANDARD_CONFIGS)} "
                                 "or json::<file> / pickle::<file>")
            load_type, load_path = path.split("::", 1)
            if load_type == "json":
                import json
                with open(load_path) as f:
                    cfg = json.load(f)
            elif load_type == "pickle":
                from .weights import load_pickle_tree
                cfg = dict(load_pickle_tree(load_path)["llama_config"])
            else:
                raise ValueError(f"Unsupported load config type: {load_type}")
        cfg.update(updates)
        return cls(**cfg)


class DropoutState:
    """What the dropout sites of one model share: the (seed, step) pair of set_dropout_rng.  A site -- 0 the embedding,
    1 + 2 i the attention output of layer i, 2 + 2 i its MLP output (lwm/llama.py:998 / :1017, :423 / :618, :656-660) -- is
    ACTIVE iff its module is in training mode, its rate (embd_pdrop / resid_pdrop) is > 0 and there is no KV cache; an
    active site runs lwm_amd.llama_ops.dropout_add, whose mask is a function of (seed, step, site, row, channel) and of
    nothing else: no hidden global generator, nothing stored.  The backward, the recompute of a remat block and of an
    MLP chunk read the pair again: it stays as it is until the step's backward has run.  The masks are this build's own
    stream (i.i.d. keep with probability 1 - round(p * 65536) / 65536), not jax's threefry bits: a run does not reproduce
    the reference's masks, only their distribution."""

    def __init__(self):
        self.rng = None

    def set(self, seed, step):
        self.rng = (_dropout._u32(seed, "seed"), _dropout._u32(step, "step"))

    def site(self, module, rate, cache, site):
        """None (inactive), or the (p, rng, site) that dropout_add takes"""
        if not (module.training and rate > 0 and cache is None):
            return None
        if self.rng is None:
            raise ValueError(f"a training-mode forward with dropout rate {rate} needs its random stream named: call "
                             "model.set_dropout_rng(seed, step) before every step (model.eval() turns dropout off)")
        if sp_size_rank("sp")[0] > 1:
            raise NotImplementedError(
                f"dropout (rate {rate}) with sp > 1: the mask is a function of the GLOBAL row, and handing a rank's rows "
                "their global rows (dropout_add's s_offset, per run of the layout) is not wired up; one rank, or rates 0")
        return (rate, self.rng, site)


def _multi_rank():
    """More than one rank along the bound "sp" axis (never the WORLD size: see set_sp_group)."""
    return sp_size_rank("sp")[0] > 1


def _dense(i, o, std, dtype):
    return torch.nn.Parameter(torch.randn(i, o, dtype=torch.float32).mul_(std).to(dtype))


def key_padding_bias(attention_mask):
    """lwm/llama.py:527-537: the (B, S_global) key mask as the additive bias the blockwise branch hands to ringattention,
    (B,1,1,S_global) with 0 where attention_mask > 0 and finfo.min elsewhere."""
    B, S = attention_mask.shape
    return torch.where(attention_mask.reshape(B, 1, 1, S) > 0, 0.0, torch.finfo(torch.float32).min)


def cached_visibility(B, Q, max_len, q0, attention_mask, device):
    """lwm/llama.py:574-592 with a cache present: key j of the max_len cache rows is visible to query i of the block iff
    j <= q0 + i (q0 = cache_index, plus the block's offset when the update is sharded) and attention_mask[b, j] > 0
    (attention_mask: (B, >= max_len) or None).  -> (B,1,Q,max_len) bool."""
    ar = torch.arange(max_len, device=device)
    mask = (ar[None, :] <= (torch.arange(Q, device=device) + q0)[:, None])[None, None].expand(B, 1, Q, max_len)
    if attention_mask is not None:
        mask = mask & (attention_mask[:, None, None, :max_len] > 0)
    return mask


def capture_decode_step(step, device, capture=True):
    """The scaffold of a hipGraph-captured decode loop: `step` (a one-token step whose inputs and outputs are static
    tensors and whose cache index lives on the device) runs once eagerly on a side stream -- library handles, first-call
    state -- and is then captured once, on one stream.  -> (the eager call's result, the graph or None, the captured
    call's result, which every replay rewrites)."""
    side = torch.cuda.Stream(device=device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):
        first = step()
    torch.cuda.current_stream(device).wait_stream(side)
    if not capture:
        return first, None, None
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        static = step()
    return first, g, static


class LLaMAAttention(torch.nn.Module):
    """FlaxLLaMAAttention.__call__, training branch (lwm/llama.py:494-570, :616-617)."""

    def __init__(self, cfg: LLaMAConfig, dtype=torch.bfloat16):
        super().__init__()
        self.cfg, self.dtype = cfg, dtype
        d = cfg.hidden_size
        self.num_heads, self.head_dim = cfg.num_attention_heads, d // cfg.num_attention_heads
        self.wq, self.wk, self.wv, self.wo = (_dense(d, d, cfg.initializer_range, dtype) for _ in range(4))

    def forward(self, x, freqs_cis, attention_mask=None, segment_ids=None, position_ids=None, cache=None, layout=None,
                residual=None):
        """layout (extension): which global positions this rank's rows are -- None = the rule bound to the "sp" axis
        (lwm_amd.ringattention.set_sp_group), "contiguous" | "zigzag", or a lwm_amd.ring.SeqLayout (a packed batch's
        balanced ownership table, lwm_amd.ring.balanced_layout).
        residual (extension): the block's `x`, added to the result (lwm/llama.py:726) -- in the wo GEMM's epilogue."""
        B, S, d = x.shape
        if self.training and cache is None and self.cfg.attn_pdrop > 0:
            raise NotImplementedError(
                f"attn_pdrop = {self.cfg.attn_pdrop} in a training-mode forward: the reference hands it to the ringattention "
                "package (lwm/llama.py:553-566), which is not part of it -- its semantics cannot be pinned; attn_pdrop=0, "
                "or model.eval()")
        split = lambda t: t.reshape(B, S, self.num_heads, self.head_dim)      # reshape, no transpose (:434-438)
        fused = cache is None and freqs_cis.is_cuda and fused_dense_ok(x, (self.wq, self.wk, self.wv, self.wo))
        if fused:
            # wq | wk | wv as ONE library GEMM into a (B,S,3,H,D) buffer, RoPE on its q | k part in one launch; the
            # attention kernels take the three strided views as they are
            xq, xk, xv = qkv_rope(x, self.wq, self.wk, self.wv, freqs_cis, position_ids, self.num_heads)
            if _multi_rank():
                xq, xk, xv = xq.contiguous(), xk.contiguous(), xv.contiguous()      # (the exchange sends whole blocks)
        else:
            xq, xk, xv = (split(t) for t in dense_multi(x, (self.wq, self.wk, self.wv)))
            xq, xk = apply_rotary_emb(xq, xk, freqs_cis, position_ids)
            xv = xv.contiguous()
        if cache is not None:
            out = dense(self._cached(xq, xk, xv, attention_mask, cache).reshape(B, S, d), self.wo)
            return out if residual is None else residual + out
        bias = None
        if attention_mask is not None:                                        # (:527-537)
            # the bias is NOT sharded over "sp" (lwm/llama.py:563): it covers the global sequence
            n_sp = sp_size_rank("sp")[0]
            if attention_mask.shape[-1] != S * n_sp:
                raise ValueError(f"attention_mask covers {attention_mask.shape[-1]} positions; the sequence ring "
                                 f"needs the global length {S * n_sp} (= local {S} x sp {n_sp}) on every rank")
            bias = key_padding_bias(attention_mask.reshape(B, S * n_sp))
        out = ringattention(xq, xk, xv, bias, segment_ids, axis_name="sp", float32_logits=True,
                            cache_idx=None,
                            blockwise_kwargs=dict(causal_block_size=1, deterministic=True, attn_pdrop=0.0,
                                                  query_chunk_size=self.cfg.scan_query_chunk_size,
                                                  key_chunk_size=self.cfg.scan_key_chunk_size),
                            layout=layout)
        if fused:
            return dense_fused(out.reshape(B, S, d), (self.wo,), residual)
        out = out.reshape(B, S, d) @ self.wo
        return out if residual is None else residual + out

    def _cached(self, xq, xk, xv, attention_mask, cache):
        """The inference branch (lwm/llama.py:571-614): mask = key j visible to query i iff
        j <= cache_index + i and attention_mask[j] (:577-592); the new keys/values are written into
        the cache at cache_index (:440-492); attention runs over the WHOLE cache (kv_len =
        max_length != q_len).  `cache`: dict(cached_key, cached_value (B, max_length, H, D),
        cache_index int); `attention_mask`: (B, max_length), ones beyond the prompt (:1121-1124)."""
        B, Q = xq.shape[:2]
        ck, cv = cache["cached_key"], cache["cached_value"]
        if "key_scale" in cache:
            return self._cached_kvq(_ops.KV8, xq, xk, xv, attention_mask, cache)
        if "key_scale_e8m0" in cache:
            # the 4-bit and the 6-bit cache name their scale tensors alike: a head of cached_key is 64 or 96 bytes
            f = _kv6.KV6 if ck.shape[-1] == _kv6.KV6.head_bytes else _kv4.KV4
            return self._cached_kvq(f, xq, xk, xv, attention_mask, cache)
        if "index_dev" in cache:
            # hipGraph-capturable decode step: cache_index lives on the device (one int32 shared by all
            # layers), the mask was built from it once for this step, and the new row is written by
            # lwm_kv_cache_write_at -- no host value changes between replays.
            _ops.kv_cache_write_at(ck, xk.contiguous(), cache["index_dev"])
            _ops.kv_cache_write_at(cv, xv, cache["index_dev"])
            return ringattention_inference(xq.contiguous(), ck, cv, cache["mask_dev"], axis_name="sp")
        n_sp, r_sp = sp_size_rank("sp")
        # the cache is sharded over "sp" (lwm/llama.py:454-467): every rank holds max_length/sp rows
        max_len, idx = ck.shape[1] * n_sp, int(cache["cache_index"])
        if xq.dtype == torch.float32 and n_sp > 1:
            raise NotImplementedError("cached inference in float32 runs on one rank (the sharded decode / dense-mask kernels "
                                      "take bf16 operands): --dtype=bf16, or mesh_dim without an sp axis")
        # (float32 -- the reference's --dtype=fp32 -- takes the structured form for decode steps too: the f32 flavour of the
        #  op evaluates `key <= cache_index + query AND attention_mask[key]` itself, there is no f32 dense-mask kernel)
        if (Q > 1 or xq.dtype == torch.float32) and n_sp == 1:
            # prefill into the cache: the same mask, handed over as its structure (see
            # ringattention_inference) -- key tiles past cache_index + Q are never read
            cache["cache_index"] = concatenate_to_cache(ck, cv, xk.contiguous(), xv, idx, axis_name="sp")
            kvld = None if attention_mask is None else attention_mask[:, :max_len]
            return ringattention_inference(xq.contiguous(), ck, cv, None, axis_name="sp", causal_offset=idx,
                                           key_valid=kvld)
        # a sharded prefill block (Q > 1) holds the queries [r*Q, (r+1)*Q) of the update; a decode query
        # is replicated (lwm/llama.py:599)
        q0 = idx + (r_sp * Q if Q > 1 else 0)
        mask = cached_visibility(B, Q, max_len, q0, attention_mask, xq.device)
        cache["cache_index"] = concatenate_to_cache(ck, cv, xk.contiguous(), xv, idx, axis_name="sp")
        return ringattention_inference(xq.contiguous(), ck, cv, mask, axis_name="sp")

    def _cached_kvq(self, f, xq, xk, xv, attention_mask, cache):
        """_cached over a quantised cache of format f (init_cache(kv_dtype="fp8" / "fp6" / "fp4"): ops.KV8, kv6.KV6, kv4.KV4;
        csrc/attn_decode_kv8.h, attn_decode_kv6.h, attn_decode_kv4.h).  Prefill (cache_index == 0): the cached path attends over rows [0, Q)
        only -- rows past Q are invisible -- so the block attends over its OWN bf16 keys and values under the same
        structured mask, and the rows are quantised into the cache afterwards: the prompt's own attention sees
        unquantised keys.  A decode step quantises its row, then streams the cache (lwm_attn_decode_kv8 / _kv6 / _kv4 + the
        split-K combine).  A block at cache_index > 0 is refused unless the format has a block kernel and the cache was
        made for blocks."""
        from .ring import _pick_splits
        B, Q, H, D = xq.shape
        ck, cv, ks, vs = cache["cached_key"], cache["cached_value"], cache[f.scale_keys[0]], cache[f.scale_keys[1]]
        _kvq_refuse(f, xq.dtype, sp_size_rank("sp")[0], D)
        xq, xk, xv = xq.contiguous(), xk.contiguous(), xv.contiguous()
        max_len = ck.shape[1]
        blocks = (f"kv_dtype={f.kv_dtype!r} with Q > 1 at cache_index > 0: the {f.bits} cache takes a prompt at cache_index 0 and "
                  "one token per step after it" + ("" if f.block_kernel else f" (a block kernel over the {f.bits} cache is not built)"))
        if "index_dev" in cache:                   # hipGraph-capturable step: see _cached
            if Q != 1:
                raise NotImplementedError(blocks)
            _ops._kvq_cache_write_at(f, ck, ks, xk, cache["index_dev"])
            _ops._kvq_cache_write_at(f, cv, vs, xv, cache["index_dev"])
            mask = (cache["mask_dev"][:, 0] != 0).to(torch.uint8).contiguous()
        else:
            idx = int(cache["cache_index"])
            if idx == 0:
                kvld = None if attention_mask is None else attention_mask[:, :Q]
                out = ringattention_inference(xq, xk, xv, None, axis_name="sp", causal_offset=0, key_valid=kvld)
                _ops._kvq_cache_write(f, ck, ks, xk, dst_row0=0)
                _ops._kvq_cache_write(f, cv, vs, xv, dst_row0=0)
                cache["cache_index"] = Q
                return out
            if Q != 1 and not (f.block_kernel and cache.get("kv8_blocks")):
                raise NotImplementedError(blocks)
            _ops._kvq_cache_write(f, ck, ks, xk, dst_row0=idx)
            _ops._kvq_cache_write(f, cv, vs, xv, dst_row0=idx)
            cache["cache_index"] = n = idx + Q
            if Q != 1:
                # a block appended to a live cache (init_cache(chunked_prefill=True)): the decode step's rule -- quantise
                # your own rows, then read the cache -- for Q rows at once: the same as feeding the tokens one at a time.
                # the format's block kernel (lwm_attn_prefill_kv8 / _kv6) dequantises while it stages; no bf16 copy of the
                # cache is made
                kvld = None if attention_mask is None else (attention_mask[:, :n] != 0).to(torch.uint8)
                o_parts, l_parts = _ops._kvq_block_fn(f)(xq, ck[:, :n], ks[:, :n], cv[:, :n], vs[:, :n], q_start=idx,
                                                    k_splits=_pick_splits(B, Q, H, n), key_valid=kvld)
                if o_parts.shape[0] == 1:
                    # one piece: the partial IS the normalised output, and attn_combine's merge of one piece is the
                    # identity followed by the rounding to bf16 (the same bits: tests/test_gpu_kv8_prefill.py) -- but a
                    # workgroup per (row, head) built for hundreds of decode pieces: 1.9 ms for a 4096 x 32 block against
                    # the cast kernel's HBM time (profiles/r10_kv8_prefill.md)
                    return _ops.cast_f32_to_bf16(o_parts[0])
                return _ops.attn_combine(o_parts, l_parts, want_bf16=True)[0]
            mask = cached_visibility(B, 1, max_len, idx, attention_mask, xq.device)[:, 0].to(torch.uint8).contiguous()
        o_parts, l_parts = _ops._kvq_attn_decode(f, xq, ck, ks, cv, vs, k_splits=_pick_splits(B, 1, H, max_len), dense_mask=mask)
        return _ops.attn_combine(o_parts, l_parts, want_bf16=True)[0]


def _kvq_refuse(f, dtype, n_sp, D):
    """what no quantised cache serves, by name (init_cache and every step check the same three things)"""
    if dtype != torch.bfloat16:
        raise NotImplementedError(f"kv_dtype={f.kv_dtype!r} with a float32 model: the {f.bits} cache quantises bf16 rows and its "
                                  "decode kernel takes a bf16 query (--dtype=bf16, or the default cache)")
    if n_sp > 1:
        raise NotImplementedError(f"kv_dtype={f.kv_dtype!r} with sp > 1: the {f.bits} cache is not sharded over the sequence ring "
                                  "(one rank, or the default cache)")
    if D != 128:
        raise NotImplementedError(f"kv_dtype={f.kv_dtype!r}: head_dim {D} (the {f.bits} decode kernel is built for 128)")


class LLaMABlock(torch.nn.Module):
    """FlaxLLaMABlock (lwm/llama.py:664-744): pre-norm residual block, blockwise FFN."""

    def __init__(self, cfg: LLaMAConfig, dtype=torch.bfloat16):
        super().__init__()
        self.cfg = cfg
        self.attention_norm = RMSNorm(cfg.hidden_size, cfg.rms_norm_eps, dtype)
        self.attention = LLaMAAttention(cfg, dtype)
        self.ffn_norm = RMSNorm(cfg.hidden_size, cfg.rms_norm_eps, dtype)
        self.feed_forward = LLaMAMLP(cfg.hidden_size, cfg.intermediate_size, dtype, cfg.initializer_range)
        self.layer_index = 0               # the model numbers its blocks: the dropout sites of layer i are 1 + 2 i, 2 + 2 i
        self._dropout = DropoutState()     # (the model shares ONE state among its blocks)

    def set_dropout_rng(self, seed, step):
        """a block on its own: see LLaMAForCausalLM.set_dropout_rng"""
        self._dropout.set(seed, step)

    def forward(self, x, freqs_cis, attention_mask=None, segment_ids=None, position_ids=None, cache=None, layout=None):
        drop_a = self._dropout.site(self, self.cfg.resid_pdrop, cache, 1 + 2 * self.layer_index)
        if drop_a is not None:
            return self._forward_dropout(x, freqs_cis, attention_mask, segment_ids, position_ids, layout, drop_a)
        if cache is None and x.is_cuda and x.dtype == torch.bfloat16:
            # training / uncached branch: `x` goes through each norm as (norm(x), x) so that the residual branch's gradient
            # is added inside the RMSNorm backward kernel, and each residual add rides in the epilogue of the GEMM before it
            h, x = rmsnorm_residual(self.attention_norm, x)
            x = self.attention(h, freqs_cis, attention_mask, segment_ids, position_ids, None, layout, residual=x)
            h, x = rmsnorm_residual(self.ffn_norm, x)
            if self.cfg.scan_mlp and h.shape[1] >= self.cfg.scan_mlp_chunk_size:      # (:728-734)
                return x + blockwise_feedforward(self.feed_forward, h, self.cfg.scan_mlp_chunk_size)
            return self.feed_forward(h, residual=x)
        x = x + self.attention(self.attention_norm(x), freqs_cis, attention_mask, segment_ids, position_ids, cache, layout)
        h = self.ffn_norm(x)
        if self.cfg.scan_mlp and h.shape[1] >= self.cfg.scan_mlp_chunk_size:      # (:728-734)
            ff = blockwise_feedforward(self.feed_forward, h, self.cfg.scan_mlp_chunk_size)
        else:
            ff = self.feed_forward(h)
        return x + ff

    def _forward_dropout(self, x, freqs_cis, attention_mask, segment_ids, position_ids, layout, drop_a):
        """forward with the residual dropout sites active (training mode, resid_pdrop > 0, no cache): both branches of
        forward, with wo and w2 run WITHOUT their residual epilogue and dropout_add doing the add in their place
        (lwm/llama.py:618 + :726, :660 + :743); the rmsnorm_residual pairing stays.  In the chunked MLP the dropout sits
        inside the chunk, as in the reference (:659-660), each chunk at its own row offset, and the add stays outside."""
        drop_m = (drop_a[0], drop_a[1], drop_a[2] + 1)
        fused = x.is_cuda and x.dtype == torch.bfloat16
        if fused:
            h, x = rmsnorm_residual(self.attention_norm, x)
        else:
            h = self.attention_norm(x)
        a = self.attention(h, freqs_cis, attention_mask, segment_ids, position_ids, None, layout)
        x = _lo.dropout_add(a.contiguous(), x.contiguous(), *drop_a)
        if fused:
            h, x = rmsnorm_residual(self.ffn_norm, x)
        else:
            h = self.ffn_norm(x)
        if self.cfg.scan_mlp and h.shape[1] >= self.cfg.scan_mlp_chunk_size:      # (:728-734)
            return x + blockwise_feedforward(lambda c, s0: self.feed_forward(c, dropout=drop_m, s_offset=s0), h,
                                             self.cfg.scan_mlp_chunk_size, with_offset=True)
        return self.feed_forward(h, residual=x.contiguous(), dropout=drop_m)


class LLaMAForCausalLM(torch.nn.Module):
    """FlaxLLaMAModule + lm_head (lwm/llama.py:982-1106), loss of lwm/train.py:171-181."""

    def __init__(self, cfg: LLaMAConfig, dtype=torch.bfloat16):
        super().__init__()
        self.cfg, self.dtype = cfg, dtype
        self.wte = torch.nn.Parameter(torch.randn(cfg.vocab_size, cfg.hidden_size).mul_(cfg.initializer_range).to(dtype))
        self.h = torch.nn.ModuleList(LLaMABlock(cfg, dtype) for _ in range(cfg.num_hidden_layers))
        self._dropout = DropoutState()
        for i, blk in enumerate(self.h):
            blk.layer_index, blk._dropout = i, self._dropout
        self.ln_f = RMSNorm(cfg.hidden_size, cfg.rms_norm_eps, dtype)
        self.lm_head = _dense(cfg.hidden_size, cfg.vocab_size, cfg.initializer_range, dtype)
        self._freqs = None
        self._decode_packs = None  # quantize_decode_weights: (wpack.WeightFormat, {parameter name: its pack}); one kind at a time
        self._decode_rows = None   # decode_rows: None = LWM_DECODE_ROWS
        self._remat_blocks = None  # remat_blocks: None = LWM_REMAT_BLOCK

    def _table(self, device):
        if self._freqs is None or self._freqs.device != device:
            head_dim = self.cfg.hidden_size // self.cfg.num_attention_heads
            self._freqs = precompute_freqs_cis(head_dim, self.cfg.max_sequence_length, self.cfg.theta, device=device)
        return self._freqs

    @staticmethod
    def _ring_position_ids(input_ids, position_ids, cache, layout=None):
        """position_ids of a sequence-sharded training batch: the GLOBAL positions of this rank's rows under the
        ownership rule bound to the "sp" axis (lwm_amd.ringattention.set_sp_group: zigzag by default, or the
        reference's contiguous blocks, lwm/llama.py:560-562) or under `layout` -- the rows were cut with `sp_shard`,
        so RoPE and the causal mask both see where each token really sits.

        A caller that brings its OWN position_ids to a sharded training batch cut the rows itself; the masks are
        evaluated at the positions the ownership rule gives those rows, so the rule has to be NAMED then -- `layout=`
        here, set_sp_group(group, layout=...) or LWM_SP_LAYOUT.  With the defaulted rule (zigzag) a batch sharded the
        reference's way would get RoPE at contiguous positions and causal masks at zigzag ones, without an error
        anywhere: refused instead."""
        n_sp = sp_size_rank("sp")[0]
        if n_sp > 1 and position_ids is None and cache is None:
            B, S = input_ids.shape
            position_ids = sp_positions(S, "sp", input_ids.device, layout).to(torch.int32)[None].expand(B, S).contiguous()
        elif n_sp > 1 and cache is None and layout is None and not sp_layout_is_explicit("sp"):
            raise ValueError(
                "position_ids were given for a sequence-sharded batch, but nobody said which global positions this "
                "rank's rows ARE: pass layout= ('contiguous' = the reference's blocks, lwm/llama.py:560-562; 'zigzag' = "
                "what sp_shard cuts by default; or a SeqLayout), or name the rule once with "
                "set_sp_group(group, layout=...) / LWM_SP_LAYOUT")
        if n_sp > 1 and position_ids is None:
            raise ValueError("cached inference over a sequence ring needs explicit global position_ids")
        return n_sp, position_ids

    @property
    def decode_rows(self):
        """None, or N in 5..32: cached one-token steps of up to N batch rows run through the fused step and
        lwm_gemm_rows_fused_bf16 / _w8 / _w6 (csrc/gemm_rows.h) instead of block by block through the library GEMMs, and the
        heads' f32 logits with them.  Opt-in (such steps then differ in their low bits); unset, the attribute reads
        LWM_DECODE_ROWS.  Values outside 5..32 raise ValueError."""
        return parse_decode_rows(os.environ.get("LWM_DECODE_ROWS")) if self._decode_rows is None else self._decode_rows

    @decode_rows.setter
    def decode_rows(self, n):
        self._decode_rows = parse_decode_rows(n, "decode_rows")

    @property
    def remat_blocks(self):
        """Per-block activation recompute (lwm_amd/remat.py): a training step keeps, per block, its input and the
        attention op's out / lse -- remat.saved_bytes -- and runs the block's other operators again in the backward; the
        attention forward is not run again.  Same loss and gradients.  Opt-in; None (the default) reads LWM_REMAT_BLOCK
        (1 = on; 0, "" or unset = off; anything else raises ValueError), True / False set it.  Inert with a KV cache,
        under no_grad, where nothing requires a gradient and inside a hipGraph capture."""
        rb = getattr(self, "_remat_blocks", None)
        return _remat.parse_remat_block(os.environ.get(_remat.ENV)) if rb is None else rb

    @remat_blocks.setter
    def remat_blocks(self, on):
        self._remat_blocks = None if on is None else _remat.parse_remat_block(on, "remat_blocks")

    def set_dropout_rng(self, seed, step):
        """Names the random stream of the NEXT training step's dropout sites (DropoutState): two integers in [0, 2^32),
        the Philox key as they stand (ValueError otherwise).  The same pair gives the same masks -- in the forward, the
        backward and every recompute; a training loop passes its seed and a step counter that never repeats
        (lwm_amd.cli.train: step * accumulate_gradient_steps + micro-step).  A training-mode forward with a rate > 0 and
        no pair set raises ValueError; with both rates 0, in eval() and with a KV cache nothing reads it."""
        self._dropout.set(seed, step)
        return self

    def _embd_dropout(self, x, cache):
        """the embedding's dropout site (site 0; lwm/llama.py:1017, lwm/vision_llama.py:313) over embedded tokens x"""
        drop = self._dropout.site(self, self.cfg.embd_pdrop, cache, 0)
        return x if drop is None else _lo.dropout_add(x.contiguous(), None, *drop)

    def hidden_states(self, input_ids, attention_mask=None, segment_ids=None, position_ids=None, cache=None, layout=None):
        n_sp, position_ids = self._ring_position_ids(input_ids, position_ids, cache, layout)
        x = self._embd_dropout(torch.nn.functional.embedding(input_ids.long(), self.wte), cache)
        return self._layers(x, n_sp, attention_mask, segment_ids, position_ids, cache, layout)

    def _layers(self, x, n_sp, attention_mask, segment_ids, position_ids, cache, layout):
        """the blocks and the final norm over embedded tokens x (B, S, d)"""
        fc = self._table(x.device)
        if cache is not None and self._fused_decode_ok(x, n_sp):
            return self.ln_f(self._decode_layers_fused(x, fc, attention_mask, position_ids, cache))
        with decode_rows_scope(self.decode_rows):
            x = self._blocks(x, fc, attention_mask, segment_ids, position_ids, cache, layout)
        return self.ln_f(x)

    def _blocks(self, x, fc, attention_mask, segment_ids, position_ids, cache, layout):
        """the blocks in turn; with remat_blocks on, an uncached block call that autograd records goes through
        lwm_amd.remat.remat_block (every other call is the plain one: remat.applies)"""
        remat = cache is None and self.remat_blocks
        for i, blk in enumerate(self.h):
            if remat and _remat.applies(blk, x):
                x = _remat.remat_block(blk, x, fc, attention_mask, segment_ids, position_ids, layout)
            else:
                x = blk(x, fc, attention_mask, segment_ids, position_ids, None if cache is None else cache[i], layout)
        return x

    def _fused_decode_ok(self, x, n_sp):
        """One token per batch row through the KV cache, bf16, no autograd, one rank: the layers can run as GEMV launch
        pairs that carry their neighbours (lwm_gemv_fused_bf16; LWM_DECODE_FUSED=0 issues every launch on its own).  At most
        four rows -- or decode_rows of them, where that is set: rows 5.. then go through lwm_gemm_rows_fused_*."""
        d = self.cfg.hidden_size
        # (d / 128 partial sums of squares per row ride along: lwm_gemv_fused_bf16 takes at most 64 of them; the weights
        # must be what the GEMV streams -- contiguous bf16 -- or the per-block path runs)
        return (os.environ.get("LWM_DECODE_FUSED", "1") == "1" and x.shape[1] == 1 and x.shape[0] <= (self.decode_rows or 4) and n_sp == 1
                and x.is_cuda and x.dtype == torch.bfloat16 and not torch.is_grad_enabled() and d % 128 == 0
                and d <= 8192 and self.cfg.intermediate_size % 32 == 0 and self.cfg.intermediate_size <= 12288
                and all(p.dtype == torch.bfloat16 and p.is_contiguous() for p in self.h[0].parameters() if p.dim() == 2))

    @staticmethod
    def _norm_weight_bf16(norm):
        """the RMSNorm weight as the kernels read it (bf16), cached on the module while the parameter is unchanged"""
        w = norm.kernel
        hit = getattr(norm, "_lwm_bf16", None)
        if hit is None or hit[0] != (w._version, w.data_ptr()):
            hit = ((w._version, w.data_ptr()), w.detach().to(torch.bfloat16).contiguous())
            norm._lwm_bf16 = hit
        return hit[1]

    # ---- 8-bit, 6-bit and 4-bit decode weights (extension; include/lwm_hip.h "8-bit decode weights" ff., lwm_amd/wpack.py)
    def _decode_weight_params(self):
        """(name, parameter) of every kernel a cached one-token step streams through the GEMV"""
        for i, blk in enumerate(self.h):
            for mod, names in (("attention", ("wq", "wk", "wv", "wo")), ("feed_forward", ("w1", "w2", "w3"))):
                for n in names:
                    yield f"h.{i}.{mod}.{n}", getattr(getattr(blk, mod), n)
        yield "lm_head", self.lm_head

    @torch.no_grad()
    def quantize_decode_weights(self, mode="fp8"):
        """Every projection kernel of the blocks and lm_head is ROUNDED IN PLACE to the values the format of `mode` can hold
        and a pack of it is kept beside it.  After it the model IS the rounded model: prefill, training ops,
        LWM_DECODE_FUSED=0 and batches over the format's rows run as before on the rounded bf16 parameters, while the fused
        one-token step and the f32 logits of the heads stream the packs -- bit for bit what the bf16 entries give on the
        rounded parameters, from a fraction of the bytes.  The bf16 parameters stay: the weights take 1 + that fraction of
        their memory.  A pack whose parameter changes afterwards is refused at its next use (RuntimeError): quantise again.
        A later call with another mode replaces the packs (rounding the already rounded kernels again); only one kind of
        pack is held at a time.  mode="bf16" / None = drop_decode_weights().  bf16 models on one rank.
        "fp8" (lwm_amd/w8.py): e4m3 codes, one power-of-two scale per 128 rows of K and column; 0.516 of the bytes;
            lwm_gemv_fused_w8 at up to 4 rows, lwm_gemm_rows_fused_w8 at 5..decode_rows rows.
        "fp6" (lwm_amd/w6.py): MXFP6, e2m3 codes -- three mantissa bits, as e4m3 -- and one power-of-two scale per 32 rows of
            K and column; 0.391 of the bytes (0.757 of the 8-bit packs'); lwm_gemv_fused_w6 at up to 4 rows,
            lwm_gemm_rows_fused_w6 at 5..decode_rows rows.
        "fp4" (lwm_amd/w4.py): MXFP4, e2m1 codes, one power-of-two scale per 32 rows of K and column; 0.266 of the bytes;
            lwm_gemv_fused_w4 at up to 4 rows.  There is no 4-bit body for more rows: where decode_rows is set, steps of 5..
            rows run lwm_gemm_rows_fused_bf16 over the bf16 parameters -- those ARE the rounded model, so that route
            computes the same model and only saves no bytes.  4-bit round-to-nearest moves a model's logits far more than
            the 8-bit packs do: check quality on the model in use."""
        if mode in (None, "bf16"):
            return self.drop_decode_weights()
        fmt = FORMATS.get(mode)
        if fmt is None:
            raise ValueError(f"quantize_decode_weights({mode!r}): 'fp8', 'fp6', 'fp4', or 'bf16' / None (drop_decode_weights)")
        if self.dtype != torch.bfloat16:
            raise NotImplementedError(f"quantize_decode_weights({mode!r}) with a float32 model: the {fmt.bits} packs are made from bf16 "
                                      "kernels and the GEMV that streams them takes bf16 activations (--dtype=bf16, or bf16 weights)")
        if sp_size_rank("sp")[0] > 1:
            raise NotImplementedError(f"quantize_decode_weights({mode!r}) with sp > 1: the fused one-token step runs on one rank "
                                      "(one rank, or bf16 decode weights)")
        quantise_weight = getattr(fmt.module, "quantise_weight")
        packs = {}
        for name, p in self._decode_weight_params():
            try:
                packs[name] = quantise_weight(p)
            except ValueError as e:
                raise ValueError(f"quantize_decode_weights({mode!r}): {name}: {e}") from None
        self._decode_packs = (fmt, packs)
        return self

    def drop_decode_weights(self):
        """Back to bf16 weight streaming.  The parameters stay as they are (rounded, if they were quantised)."""
        self._decode_packs = None
        return self

    def decode_packs(self, mode=None):
        """{parameter name: pack} if the packs of `mode` ("fp8", "fp6", "fp4") are held, else None; without a mode: the held
        (wpack.WeightFormat, packs), or None"""
        held = getattr(self, "_decode_packs", None)
        if mode is None or held is None:
            return held
        return held[1] if held[0].mode == mode else None

    def _checked_packs(self, names, kernels):
        """the held packs of `kernels`, each checked against its parameter as it is NOW"""
        packs = self._decode_packs[1]
        return [packs[n].check(k, n) for n, k in zip(names, kernels)]

    def _decode_layers_fused(self, x, fc, attention_mask, position_ids, cache):
        """The blocks of a cached one-token step (lwm/llama.py:704-744 with q_len = 1) with each RMSNorm folded into the
        x load of the projections that follow it and each residual add into the reduction of the projection before it:
        per layer 4 fewer launches of the ~19; same roundings as the separate kernels (rstd sums in another order)."""
        from . import llama_ops
        B, _, d = x.shape
        # <= 4 rows: the GEMV; above (decode_rows): the same launch pairs on the matrix pipe.  (Looked up at call time: the
        # entries can be wrapped.)
        gemv_fused = llama_ops.gemv_fused if B <= 4 else llama_ops.gemm_rows_fused
        held = getattr(self, "_decode_packs", None)
        # the same launch pairs over the held packs (bit for bit on the rounded parameters); a format without a rows entry
        # leaves more than 4 rows to the rounded bf16 parameters
        if held is not None and (B <= 4 or held[0].proj.entries[1] is not None):
            fused_packs = getattr(held[0].module, held[0].proj.fused[1 if B > 4 else 0])
            names = {id(p): n for n, p in self._decode_weight_params()}
            gemv_fused = lambda x, ks, **kw: fused_packs(x, self._checked_packs([names[id(k)] for k in ks], ks), **kw)    # noqa: E731
        H, D = self.cfg.num_attention_heads, d // self.cfg.num_attention_heads
        x2 = x.reshape(B, d)
        ss = torch.zeros(B, 32, dtype=torch.float32, device=x.device)
        ss[:, 0] = x2.float().pow(2).sum(-1)
        eps = self.cfg.rms_norm_eps
        for i, blk in enumerate(self.h):
            att, mlp = blk.attention, blk.feed_forward
            q, k, v = gemv_fused(x2, (att.wq, att.wk, att.wv), norm=(ss, self._norm_weight_bf16(blk.attention_norm), eps))
            split = lambda t: t.reshape(B, 1, H, D)
            xq, xk = apply_rotary_emb(split(q), split(k), fc, position_ids)
            a = att._cached(xq, xk, split(v).contiguous(), attention_mask, cache[i]).reshape(B, d)
            (x2,), ss = gemv_fused(a, (att.wo,), residual=x2, want_ss=True)
            gate, up = gemv_fused(x2, (mlp.w1, mlp.w3), norm=(ss, self._norm_weight_bf16(blk.ffn_norm), eps))
            (x2,), ss = gemv_fused(swiglu(gate, up), (mlp.w2,), residual=x2, want_ss=True)
        return x2.reshape(B, 1, d)

    def init_cache(self, batch_size, max_length, device=None, kv_dtype=None, *, chunked_prefill=False):
        """FlaxLLaMAPreTrainedModel.init_cache (lwm/llama.py:810-825): per layer, zeroed
        (B, max_length, H, D) key/value caches and cache_index = 0.
        kv_dtype="fp8" (extension): the 8-bit cache of csrc/attn_decode_kv8.h -- per layer cached_key / cached_value as
        uint8 e4m3fn bytes plus key_scale / value_scale (B, max_length, H) f32: 0.516 of the bytes, held and read per
        decode step.  bf16 models on one rank; a prompt at cache_index 0, then one token per step.
        chunked_prefill=True (with kv_dtype="fp8"): the cache also takes BLOCKS of tokens at cache_index > 0 (chunked
        prefill, a follow-up turn): such a block is quantised into the cache first and then attends over the quantised
        rows, its own included -- the decode step's rule, so a block equals its tokens fed one at a time, whereas a block
        at cache_index 0 sees its own unquantised keys.  Opt-in because of that difference.  The default cache takes blocks
        anywhere as it is; the flag changes nothing for it.
        kv_dtype="fp4" (extension): the 4-bit MXFP4 cache of csrc/attn_decode_kv4.h -- per layer cached_key / cached_value
        as uint8 (B, max_length, H, 64) e2m1 nibble pairs plus key_scale_e8m0 / value_scale_e8m0 (B, max_length, H, 4) e8m0
        bytes: 0.27 of the bytes.  bf16 models on one rank; a prompt at cache_index 0, then one token per step;
        chunked_prefill=True is refused (a block kernel over the 4-bit cache is not built).
        kv_dtype="fp6" (extension): the 6-bit MXFP6 cache of csrc/attn_decode_kv6.h -- per layer cached_key / cached_value
        as uint8 (B, max_length, H, 96) e2m3 blocks plus key_scale_e8m0 / value_scale_e8m0 (B, max_length, H, 4) e8m0 bytes:
        0.39 of the bytes.  bf16 models on one rank; takes chunked_prefill=True as the 8-bit cache does."""
        device = device or self.wte.device
        H = self.cfg.num_attention_heads
        D = self.cfg.hidden_size // H
        n_sp = sp_size_rank("sp")[0]
        if max_length % n_sp:
            raise ValueError(f"max_length {max_length} is not divisible by the sp ring size {n_sp}")
        formats = {"fp8": _ops.KV8, "fp6": _kv6.KV6, "fp4": _kv4.KV4}
        if kv_dtype is not None and kv_dtype not in formats:
            raise ValueError(f"kv_dtype={kv_dtype!r}: None (the model's dtype), 'fp6', 'fp8' or 'fp4'")
        if kv_dtype is not None:
            f = formats[kv_dtype]
            _kvq_refuse(f, self.dtype, n_sp, D)
            if chunked_prefill and not f.block_kernel:
                raise NotImplementedError(f"kv_dtype={f.kv_dtype!r} with chunked prefill (chunked_prefill=True, prefill_chunk=N): a "
                                          f"block kernel over the {f.bits} cache is not built; kv_dtype='fp8' and 'fp6' take blocks")
            q = lambda: torch.zeros(batch_size, max_length, H, f.head_bytes, dtype=torch.uint8, device=device)
            sc = lambda: torch.full((batch_size, max_length, H) + f.scale_tail, f.scale_one, dtype=f.scale_dtype, device=device)
            mark = dict(kv8_blocks=True) if chunked_prefill else {}
            return [{"cached_key": q(), "cached_value": q(), f.scale_keys[0]: sc(), f.scale_keys[1]: sc(), "cache_index": 0, **mark}
                    for _ in self.h]
        # sharded over "sp": each rank holds its contiguous max_length/sp rows (lwm/llama.py:454-467)
        z = lambda: torch.zeros(batch_size, max_length // n_sp, H, D, dtype=self.dtype, device=device)
        return [dict(cached_key=z(), cached_value=z(), cache_index=0) for _ in self.h]

    @staticmethod
    def device_index_cache(cache, index_dev):
        """The per-layer cache dicts of a captured decode step: the same tensors, the row index on the device."""
        return [{**{k: t for k, t in c.items() if k != "cache_index"}, "index_dev": index_dev} for c in cache]

    @torch.no_grad()
    def generate(self, input_ids, attention_mask=None, max_new_tokens=16, max_length=None, return_logits=False,
                 graph=False, kv_dtype=None, prefill_chunk=None):
        """Greedy decoding through the KV cache: prepare_inputs_for_generation /
        update_inputs_for_generation of the reference (lwm/llama.py:1113-1137) + argmax.
        Prefill writes the prompt's keys/values at cache_index 0 and attends over the whole
        (B, max_length) cache under the dense mask; every further step feeds one token.

        graph=True: the one-token step (every layer's RMSNorm, projections, RoPE, cache write, decode
        attention, MLP, and the head) is captured ONCE in a hipGraph and replayed per token; the
        cache index, position and current token advance on the device inside the graph.  A decode
        step is some 15 launches per layer of a few microseconds of work each -- launch-bound when
        issued one by one.  Single-rank only (the cross-rank combine is not captured).

        kv_dtype="fp8": the 8-bit KV cache (init_cache); the prompt attends over its own bf16 keys, every later
        step over the quantised cache.  Works with graph=True.  kv_dtype="fp4": the 4-bit MXFP4 cache, by the same
        rules; prefill_chunk is refused with it (a block kernel over the 4-bit cache is not built).  kv_dtype="fp6": the
        6-bit MXFP6 cache, by the 8-bit cache's rules, prefill_chunk included.

        prefill_chunk=N: the prompt goes through the layers in blocks of N tokens (the last may be shorter), so the
        transient activations of the prefill are bounded by N instead of the prompt length.  With kv_dtype="fp8" or "fp6" the
        cache is created with chunked_prefill=True: the first block sees its own unquantised keys, every later block the
        quantised rows (init_cache).  One rank; works with graph=True (the captured step starts after the prefill)."""
        B, S = input_ids.shape
        check_prefill_chunk(prefill_chunk)
        max_length = max_length or (S + max_new_tokens)
        dev = input_ids.device
        if graph and self.dtype == torch.float32:
            raise NotImplementedError("generate(graph=True) captures the bf16 decode kernels; a float32 model decodes eagerly "
                                      "(graph=False) through the f32 flavour of the attention op")
        # (the default cache through the three-argument call every stand-in model answers)
        cache = self.init_cache(B, max_length, dev, **cache_kwargs(kv_dtype, prefill_chunk))
        ext = torch.ones(B, max_length, dtype=torch.int32, device=dev)
        if attention_mask is not None:
            pos = attention_mask.to(torch.int32).cumsum(-1) - 1
            ext[:, :S] = attention_mask.to(torch.int32)
        else:
            pos = torch.arange(S, dtype=torch.int32, device=dev)[None].expand(B, S)
        pos = pos.clamp_min(0).to(torch.int32).contiguous()
        head = self.lm_head        # f32 logits: bf16 operands are exact in f32, so `dense(.., torch.float32)` on the
        #                            bf16 kernel forms the same products as h.float() @ kernel.float() and reads half the bytes
        tokens, logits_out = [input_ids], []

        def emit(logits):
            if return_logits:
                logits_out.append(logits.clone())
            nxt = logits.argmax(-1, keepdim=True).to(input_ids.dtype)
            tokens.append(nxt.clone())
            return nxt

        # prefill (and, without graph, every later step): host-side cache_index
        step_in = input_ids
        n_eager = max_new_tokens if not graph else min(1, max_new_tokens)
        if prefill_chunk is not None and n_eager > 0:
            # every block but the last only fills the cache; the last one is the first pass of the loop below
            for a in range(0, S - prefill_chunk, prefill_chunk):
                self.hidden_states(input_ids[:, a:a + prefill_chunk], ext, None, pos[:, a:a + prefill_chunk].contiguous(), cache)
            a = max(0, (S - 1) // prefill_chunk * prefill_chunk)
            step_in, pos = input_ids[:, a:], pos[:, a:].contiguous()
        for _ in range(n_eager):
            h = self.hidden_states(step_in, ext, None, pos, cache)
            step_in = emit(_head_logits(self, h[:, -1], head))
            pos = (pos[:, -1:] + 1).contiguous()
        if graph and max_new_tokens > 1:
            import torch.distributed as dist
            if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
                raise NotImplementedError("generate(graph=True) is single-rank")
            idx = torch.tensor([int(cache[0]["cache_index"])], dtype=torch.int32, device=dev)
            ar = torch.arange(max_length, device=dev, dtype=torch.int32)
            tok, posd = step_in.clone(), pos.clone()
            dcache = self.device_index_cache(cache, idx)

            def step():
                mask = ((ar[None, :] <= idx) & (ext > 0))[:, None, None, :]
                for c in dcache:
                    c["mask_dev"] = mask
                logits = _head_logits(self, self.hidden_states(tok, ext, None, posd, dcache)[:, -1], head)
                tok.copy_(logits.argmax(-1, keepdim=True).to(tok.dtype))
                posd.add_(1)
                idx.add_(1)
                return logits

            first, g, static_logits = capture_decode_step(step, dev, capture=max_new_tokens > 2)
            emit(first)
            for _ in range(max_new_tokens - 2):
                g.replay()
                emit(static_logits)
        out = torch.cat(tokens, dim=1)
        return (out, torch.stack(logits_out, 1)) if return_logits else out

    def loss(self, input_tokens, target_tokens, loss_masks=None, attention_mask=None, segment_ids=None,
             position_ids=None, chunk=8192, layout=None, sp_sharded=True):
        """lwm/train.py:171-181.  Over a sequence ring (more than one rank on the "sp" axis) the arguments are this
        rank's ROWS of the batch (sp_shard) and the result is this rank's SHARE of the reference's per-sequence mean:
        the count of valid targets is all-reduced over "sp" (every sp rank must enter the call), and the shares add up
        to the reference's loss.  sp_sharded=False says the tokens are REPLICATED on the sp ranks (evaluation /
        scoring of a short batch on every rank): no collective, each rank gets the whole loss."""
        h = self.hidden_states(input_tokens, attention_mask, segment_ids, position_ids, layout=layout)
        return chunked_lm_head_loss(h, self.lm_head, target_tokens, loss_masks, chunk, sp_sharded=sp_sharded)


def model_decode_rows(model):
    """model.decode_rows; LWM_DECODE_ROWS for a stand-in model without the attribute"""
    try:
        return model.decode_rows
    except AttributeError:
        return parse_decode_rows(os.environ.get("LWM_DECODE_ROWS"))


def head_logits(model, h, head):
    """f32 logits of `head`: through its 8-bit, 6-bit or 4-bit pack (quantize_decode_weights) where the model holds one for
    `head` and the rows go through the GEMV (at most four, no autograd) or, up to decode_rows, the format's rows entry; else
    `dense(h, head, torch.float32)` (the GEMV for <= 4 rows, lwm_gemm_rows_fused_bf16 up to model.decode_rows, the library
    beyond) -- a stand-in model without packs always gets that"""
    held = getattr(model, "_decode_packs", None)
    rows = h.numel() // h.shape[-1]
    if held is not None and h.is_cuda and h.dtype == torch.bfloat16 and not torch.is_grad_enabled():
        fmt, packs = held
        same = lambda p: p is head or (p.data_ptr() == head.data_ptr() and p.shape == head.shape and p.stride() == head.stride())
        name = next((n for n in packs if "." not in n and same(getattr(model, n))), None)
        limit = 4 if fmt.proj.entries[1] is None else max(4, model_decode_rows(model) or 4)
        if name is not None and rows <= limit:
            h2 = h.reshape(rows, h.shape[-1])
            if rows > 4 and not rows_x_ok(h2):
                h2 = h2.clone(memory_format=torch.contiguous_format)
            fused = getattr(fmt.module, fmt.proj.fused[1 if rows > 4 else 0])      # (looked up at call time: the entries can be wrapped)
            (y,) = fused(h2, model._checked_packs((name,), (head,)), out_dtype=torch.float32)
            return y.reshape(*h.shape[:-1], y.shape[-1])
    with decode_rows_scope(model_decode_rows(model)):
        return dense(h, head, torch.float32)


_head_logits = head_logits


def check_prefill_chunk(prefill_chunk):
    """generate(prefill_chunk=): None, or a block length >= 1 on one rank"""
    if prefill_chunk is None:
        return
    if int(prefill_chunk) != prefill_chunk or prefill_chunk < 1:
        raise ValueError(f"prefill_chunk={prefill_chunk!r}: None (the whole prompt in one call) or a block length >= 1")
    if sp_size_rank("sp")[0] > 1:
        raise NotImplementedError("prefill_chunk with sp > 1: chunked prefill runs on one rank (a sharded prefill block is "
                                  "already 1/sp of the prompt)")


def cache_kwargs(kv_dtype, prefill_chunk=None):
    """The keyword arguments of init_cache for a generate() call: only what is non-default is passed, so that a stand-in
    model with the three-argument init_cache keeps working."""
    kw = {} if kv_dtype is None else dict(kv_dtype=kv_dtype)
    if kv_dtype in ("fp8", "fp6", "fp4") and prefill_chunk is not None:
        kw["chunked_prefill"] = True             # (init_cache refuses it for 'fp4', by name)
    return kw


def hf_rotary_to_interleaved(w_out_in, num_heads):
    """HF-PyTorch LLaMA checkpoints (README.md:74, scripts/sample_pyt.py:8) store wq/wk for the
    rotate_half RoPE convention; the reference rotates interleaved (even, odd) pairs
    (lwm/llama.py:360-364).  w_out_in: torch Linear weight (out, in).  Returns the flax-layout
    kernel (in, out) whose head dims are re-ordered [0, d/2, 1, d/2+1, ...] so that interleaved
    RoPE on it equals rotate_half RoPE on the original."""
    out_f, in_f = w_out_in.shape
    hd = out_f // num_heads
    w = w_out_in.reshape(num_heads, 2, hd // 2, in_f).transpose(1, 2).reshape(out_f, in_f)
    return w.t().contiguous()
