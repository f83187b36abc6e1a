"""Vision-language variant of the model HARNESS (lwm/vision_llama.py): the transformer is the one of
lwm_amd/llama.py -- same blocks, same RingAttention hot path -- plus a second embedding table for the
VQGAN code vocabulary (`vte`, 8192 codes + 256 special tokens, lwm/vision_llama.py:30-32, :264-270), a
second output head (`vision_head`, :354-360), the per-position choice between the two embeddings
(:307-311) and the 0.5 * (vision CE + text CE) objective of lwm/train.py:183-202.  BASELINE config #4
(VQGAN-tokenised video frames in a 256K context) runs through this module."""
from __future__ import annotations

import torch

from . import ops as _ops
from .llama import (LLaMAConfig, LLaMAForCausalLM, _dense, cache_kwargs, capture_decode_step, check_prefill_chunk,
                    head_logits)
from .llama_ops import chunked_lm_head_loss
from .ringattention import sp_size_rank


class VideoLLaMAConfig(LLaMAConfig):
    """lwm/vision_llama.py:29-36."""

    def __init__(self, vision_vocab_size=8448, tie_vision_embeddings=False, sample_mode="all", **kwargs):
        super().__init__(**kwargs)
        self.vision_vocab_size = vision_vocab_size      # 8192 + 256
        self.tie_vision_embeddings = tie_vision_embeddings
        self.sample_mode = sample_mode


def _head_logits(model, h, head):
    """`dense(h, head, torch.float32)`, through the head's 8-bit, 6-bit or 4-bit pack where the model has one (llama.head_logits)"""
    return head_logits(model, h, head)


class VideoLLaMAForCausalLM(LLaMAForCausalLM):
    def __init__(self, cfg: VideoLLaMAConfig, dtype=torch.bfloat16):
        super().__init__(cfg, dtype)
        std = cfg.initializer_range
        self.vte = torch.nn.Parameter(torch.randn(cfg.vision_vocab_size, cfg.hidden_size).mul_(std).to(dtype))
        if not cfg.tie_vision_embeddings:
            self.vision_head = _dense(cfg.hidden_size, cfg.vision_vocab_size, std, dtype)

    def _embed(self, input_ids, vision_masks):
        """lwm/vision_llama.py:298-311: one-token steps pick the table by sample_mode; otherwise text
        positions read wte, vision positions read vte (ids are zeroed for the table they do not use)."""
        ids = input_ids.long()
        if ids.shape[1] == 1 and self.cfg.sample_mode in ("text", "vision"):
            return torch.nn.functional.embedding(ids, self.wte if self.cfg.sample_mode == "text" else self.vte)
        if ids.shape[1] == 1:
            raise NotImplementedError("sample_mode='all' cannot decode one token at a time (lwm/vision_llama.py:303)")
        vm = vision_masks.to(torch.bool)
        zero = torch.zeros_like(ids)
        text = torch.nn.functional.embedding(torch.where(vm, zero, ids), self.wte)
        vis = torch.nn.functional.embedding(torch.where(vm, ids, zero), self.vte)
        return torch.where(vm[..., None], vis, text)

    def hidden_states(self, input_ids, vision_masks, attention_mask=None, segment_ids=None, position_ids=None,
                      cache=None, layout=None):
        n_sp, position_ids = self._ring_position_ids(input_ids, position_ids, cache, layout)
        x = self._embd_dropout(self._embed(input_ids, vision_masks), cache)      # (after the vte / wte mix: :313)
        if self.decode_rows is not None:
            # opt-in (decode_rows / LWM_DECODE_ROWS): a cached one-token step of sample_mode 'text' / 'vision' takes the
            # fused step of the text model at any row count the option covers -- and with it the 8-bit or 6-bit packs
            return self._layers(x, n_sp, attention_mask, segment_ids, position_ids, cache, layout)
        return self.ln_f(self._blocks(x, self._table(x.device), attention_mask, segment_ids, position_ids, cache, layout))

    def _decode_weight_params(self):
        """... and the vision head where it is a parameter of its own (the tied head is a transposed view of vte and
        stays on the bf16 path)"""
        yield from super()._decode_weight_params()
        if not self.cfg.tie_vision_embeddings and self.vision_head.is_contiguous():
            yield "vision_head", self.vision_head

    def _vision_kernel(self):
        return self.vte.t() if self.cfg.tie_vision_embeddings else self.vision_head

    def loss(self, input_tokens, input_vision_masks, target_tokens, target_vision_masks, loss_masks=None,
             attention_mask=None, segment_ids=None, position_ids=None, chunk=8192, layout=None, sp_sharded=True):
        """modality 'vision,text' of lwm/train.py:183-209 -> (loss, metrics); both heads go through the
        chunked head+loss operator so that no (S, vocab) logits tensor exists at 256K-1M tokens."""
        h = self.hidden_states(input_tokens, input_vision_masks, attention_mask, segment_ids, position_ids, layout=layout)
        tvm = target_vision_masks.to(torch.bool)
        lm = torch.ones_like(target_tokens, dtype=torch.float32) if loss_masks is None else loss_masks.float()
        zero = torch.zeros_like(target_tokens)
        v_loss, v_acc = chunked_lm_head_loss(h, self._vision_kernel().contiguous(), torch.where(tvm, target_tokens, zero),
                                             lm * tvm.float(), chunk, sp_sharded=sp_sharded)
        t_loss, t_acc = chunked_lm_head_loss(h, self.lm_head, torch.where(tvm, zero, target_tokens),
                                             lm * (~tvm).float(), chunk, sp_sharded=sp_sharded)
        return 0.5 * (v_loss + t_loss), dict(vision_loss=v_loss, vision_acc=v_acc, text_loss=t_loss, text_acc=t_acc)

    # ---- generation (lwm/vision_llama.py:447-745).  Eager, through the KV cache of lwm_amd/llama.py.
    def _prefill(self, input_ids, vision_masks, attention_mask, max_length, kv_dtype=None, prefill_chunk=None):
        """prefill_chunk=N: the prompt in blocks of N tokens (LLaMAForCausalLM.generate); only the last block's hidden
        state is kept"""
        B, S = input_ids.shape
        dev = input_ids.device
        check_prefill_chunk(prefill_chunk)
        # (the default cache through the three-argument call every stand-in model answers)
        cache = self.init_cache(B, max_length, dev, **cache_kwargs(kv_dtype, prefill_chunk))
        ext = torch.ones(B, max_length, dtype=torch.int32, device=dev)
        if attention_mask is not None:
            pos = attention_mask.to(torch.int32).cumsum(-1) - 1          # prepare_inputs_for_generation (:447-466)
            ext[:, :S] = attention_mask.to(torch.int32)
        else:
            pos = torch.arange(S, dtype=torch.int32, device=dev)[None].expand(B, S)
        pos = pos.clamp_min(0).to(torch.int32).contiguous()
        vm = torch.zeros_like(input_ids, dtype=torch.bool) if vision_masks is None else vision_masks.to(torch.bool)
        if prefill_chunk is None:
            h = self.hidden_states(input_ids, vm, ext, None, pos, cache)
        else:
            for a in range(0, max(S, 1), prefill_chunk):
                z = a + prefill_chunk
                h = self.hidden_states(input_ids[:, a:z], vm[:, a:z], ext, None, pos[:, a:z].contiguous(), cache)
        return h[:, -1], cache, ext, (pos[:, -1:] + 1).contiguous()

    def _step(self, tok, cache, ext, pos):
        h = self.hidden_states(tok, None, ext, None, pos, cache)
        return h[:, -1], (pos + 1).contiguous()

    @staticmethod
    def _pick(logits, temperature, top_k, do_sample, gen, top_p=0.0):
        """FlaxTemperatureLogitsWarper / FlaxTopKLogitsWarper / FlaxTopPLogitsWarper + categorical sampling (greedy when
        do_sample is False or temperature == 0).  top_p (0 = off) is the nucleus rule of include/lwm_hip.h, the one the
        device sampler applies: over the top-k survivors an entry stays iff the softmax mass strictly above it is below
        top_p; entries of equal value stay or go together."""
        logits = logits.float()
        if not do_sample or temperature == 0:
            return logits.argmax(-1, keepdim=True)
        logits = logits / float(temperature)
        if top_k and 0 < top_k < logits.shape[-1]:
            kth = logits.topk(int(top_k), dim=-1).values[..., -1:]
            logits = logits.masked_fill(logits < kth, float("-inf"))
        if 0.0 < top_p < 1.0:
            srt, order = logits.sort(-1, descending=True)
            w = (srt.double() - srt[..., :1].double()).exp()                 # f64: exp(s - max), 0 for filtered entries
            above = w.cumsum(-1) - w
            first = torch.ones_like(srt, dtype=torch.bool)
            first[..., 1:] = srt[..., 1:] != srt[..., :-1]
            # the mass strictly above: every member of a group of equal values takes its first member's (`above` rises)
            above = torch.where(first, above, above.new_zeros(())).cummax(-1).values
            p32 = float(torch.tensor(top_p, dtype=torch.float32))            # the float the device sampler is handed
            stay = torch.zeros_like(first).scatter(-1, order, above < p32 * w.sum(-1, keepdim=True))
            logits = logits.masked_fill(~stay, float("-inf"))
        return torch.multinomial(torch.softmax(logits, -1), 1, generator=gen)

    # seed-driven decoding: every token drawn on the device (ops.sample_tokens); `done` is read back this often
    DONE_CHECK_EVERY = 16

    @staticmethod
    def _check_seed_args(seed, graph, generator):
        if seed is not None and generator is not None:
            raise ValueError("pass generator= (the torch sampler, eager) or seed= (the device sampler), not both")
        if graph and seed is None:
            raise ValueError("graph=True draws every token on the device: it needs seed= (generator= drives the eager "
                             "torch sampler)")

    def _seeded_decode(self, input_ids, vision_masks, attention_mask, max_length, max_new_tokens, head, *, seed, graph,
                       temperature, top_k, cfg=None, force_period=0, force_token=0, eos=None, pad=0, return_logits=False,
                       kv_dtype=None, prefill_chunk=None, top_p=0.0):
        """Decoding with every token chosen by ops.sample_tokens (csrc/sample.h) from the Philox stream of `seed`: the
        sampler also writes the next step's input ids, the output column and the done flags, so no step waits for the
        host.  graph=True: the one-token step -- layers, head, sampler, cache index -- is captured ONCE in a hipGraph
        and replayed (the scaffold of LLaMAForCausalLM.generate(graph=True)).  `cfg` (B,) f32: a batch of B conditional
        prompts followed by B unconditional ones.  With `eos`, `done` is read back every DONE_CHECK_EVERY tokens.
        -> ((B, max_new_tokens) int64, logits of every step (rows, steps, V) f32 or None)."""
        rows, S = input_ids.shape
        B = rows // 2 if cfg is not None else rows
        dev = input_ids.device
        if graph:
            if self.dtype != torch.bfloat16:
                raise NotImplementedError("graph=True captures the bf16 decode kernels; a float32 model samples on the "
                                          "device eagerly (graph=False)")
            import torch.distributed as dist
            if sp_size_rank("sp")[0] > 1 or (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
                raise NotImplementedError("graph=True is single-rank (the cross-rank combine is not captured)")
        max_length = max_length or (S + max_new_tokens)
        h, cache, ext, pos = self._prefill(input_ids, vision_masks, attention_mask, max_length, kv_dtype, prefill_chunk)
        seq = torch.full((B, max_new_tokens), int(pad), dtype=torch.int64, device=dev)
        tok = torch.empty((rows, 1), dtype=torch.int64, device=dev)
        done = None if eos is None else torch.zeros(B, dtype=torch.uint8, device=dev)
        kw = dict(temperature=float(temperature), top_k=int(top_k or 0), seed=int(seed), cfg_scale=cfg,
                  force_period=force_period, force_token=force_token, done=done, eos=eos, pad=int(pad), tokens_out=tok,
                  copies=rows // B, seq_out=seq, top_p=top_p or None)           # (0.0 = off, as ops._check_top_p returns it)
        logits_out = []
        keep = (lambda lg: logits_out.append(lg.clone())) if return_logits else (lambda lg: None)
        every = self.DONE_CHECK_EVERY
        all_done = lambda i: done is not None and (i + 1) % every == 0 and bool(done.all())    # after token i

        logits = _head_logits(self, h, head)
        keep(logits)
        _ops.sample_tokens(logits, step=0, **kw)
        if not graph:
            for i in range(1, max_new_tokens):
                if all_done(i - 1):
                    break
                h, pos = self._step(tok, cache, ext, pos)
                logits = _head_logits(self, h, head)
                keep(logits)
                _ops.sample_tokens(logits, step=i, **kw)
        elif max_new_tokens > 1 and not all_done(0):
            index = int(cache[0]["cache_index"])
            idx = torch.tensor([index], dtype=torch.int32, device=dev)
            ar = torch.arange(max_length, device=dev, dtype=torch.int32)
            posd = pos.clone()
            dcache = self.device_index_cache(cache, idx)

            def step():            # token i is sampled at cache index index + i - 1
                mask = ((ar[None, :] <= idx) & (ext > 0))[:, None, None, :]
                for c in dcache:
                    c["mask_dev"] = mask
                lg = _head_logits(self, self.hidden_states(tok, None, ext, None, posd, dcache)[:, -1], head)
                _ops.sample_tokens(lg, step_dev=idx, step_base=index - 1, **kw)
                posd.add_(1)
                idx.add_(1)
                return lg

            first, g, static_logits = capture_decode_step(step, dev, capture=max_new_tokens > 2)
            keep(first)
            for i in range(2, max_new_tokens):
                if all_done(i - 1):
                    break
                g.replay()
                keep(static_logits)
        return seq, (torch.stack(logits_out, 1) if return_logits else None)

    @torch.no_grad()
    def generate(self, input_ids, vision_masks=None, attention_mask=None, max_new_tokens=16, max_length=None,
                 temperature=1.0, top_k=None, do_sample=False, eos_token_id=None, pad_token_id=0, generator=None,
                 seed=None, graph=False, return_logits=False, kv_dtype=None, prefill_chunk=None, top_p=None):
        """Text continuation of a (left-padded) vision-language prompt -- what lwm/vision_chat.py:205-227
        runs with sample_mode='text': prefill over both embedding tables, then one token at a time
        through the text head.  Returns the NEW tokens (B, max_new_tokens), pad after eos (and the f32 logits of
        every step, (B, steps, V), with return_logits).

        Sampling: generator= (or neither generator nor seed) = the torch sampler, eager, as before; seed= = every
        token drawn on the device by ops.sample_tokens from the Philox stream of `seed` (bf16 or float32 models);
        seed= with graph=True = the same one-token step captured once in a hipGraph and replayed (bf16, one rank).
        With a seed the loop reads `done` back every DONE_CHECK_EVERY tokens instead of after every token.
        top_p=p, 0 < p < 1: nucleus sampling after temperature and top-k, on every one of these routes by the one rule of
        include/lwm_hip.h (an entry stays iff the softmax mass strictly above it is below p); None or 1.0 = off, anything
        else a ValueError; greedy decoding ignores it.
        kv_dtype="fp8": the 8-bit KV cache (LLaMAModel.init_cache), on every one of these routes.  kv_dtype="fp4": the 4-bit
        MXFP4 cache, likewise (no prefill_chunk with it: a block kernel over the 4-bit cache is not built).  kv_dtype="fp6": the
        6-bit MXFP6 cache, likewise, prefill_chunk included.  prefill_chunk=N: the
        prompt in blocks of N tokens (LLaMAForCausalLM.generate), on every one of these routes too."""
        top_p = _ops._check_top_p(top_p, "generate")
        if self.cfg.sample_mode != "text":
            raise ValueError("generate() decodes text: set sample_mode='text' (scripts/run_vision_chat.sh)")
        if seed is not None or graph:
            self._check_seed_args(seed, graph, generator)
            out, logits = self._seeded_decode(input_ids, vision_masks, attention_mask, max_length, max_new_tokens,
                                              self.lm_head, seed=seed, graph=graph,
                                              temperature=temperature if do_sample else 0.0, top_k=top_k,
                                              eos=eos_token_id, pad=pad_token_id, return_logits=return_logits,
                                              kv_dtype=kv_dtype, prefill_chunk=prefill_chunk, top_p=top_p)
            out = out.to(input_ids.dtype)
            return (out, logits) if return_logits else out
        B, S = input_ids.shape
        max_length = max_length or (S + max_new_tokens)
        h, cache, ext, pos = self._prefill(input_ids, vision_masks, attention_mask, max_length, kv_dtype, prefill_chunk)
        head = self.lm_head        # (f32 logits from the bf16 kernel: llama_ops.dense)
        out = torch.full((B, max_new_tokens), int(pad_token_id), dtype=input_ids.dtype, device=input_ids.device)
        done = torch.zeros(B, dtype=torch.bool, device=input_ids.device)
        logits_out = []
        for i in range(max_new_tokens):
            logits = _head_logits(self, h, head)
            if return_logits:
                logits_out.append(logits.clone())
            tok = self._pick(logits, temperature, top_k, do_sample, generator, top_p).to(input_ids.dtype)
            out[:, i] = torch.where(done, out[:, i], tok[:, 0])
            if eos_token_id is not None:
                done |= tok[:, 0] == eos_token_id
                if bool(done.all()):
                    break
            if i + 1 < max_new_tokens:
                h, pos = self._step(tok, cache, ext, pos)
        return (out, torch.stack(logits_out, 1)) if return_logits else out

    @torch.no_grad()
    def generate_vision(self, input_ids, cfg_scales, attention_mask=None, vision_masks=None, max_new_tokens=257,
                        temperature=1.0, top_k=None, generator=None, max_length=None, seed=None, graph=False,
                        return_logits=False, kv_dtype=None, prefill_chunk=None, top_p=None):
        """FlaxVideoLLaMAForCausalLM.generate_vision / _sample_vision (lwm/vision_llama.py:476-745):
        the batch holds the conditional prompts followed by the same number of unconditional ones;
        logits = uncond + cfg * (cond - uncond) over the VISION head (sample_mode='vision'), top-k /
        temperature sampling, every 257th new token forced to the end-of-frame code 8192 (:549-552),
        the chosen token fed to both halves.  Returns the new tokens of the conditional half (and, with return_logits,
        the f32 logits of both halves at every step, (2B, steps, V)).

        Sampling as generate(): generator= = the torch sampler, eager; seed= = ops.sample_tokens on the device, which
        also mixes the halves, forces the end-of-frame code and feeds both halves; seed= with graph=True = that step
        captured once in a hipGraph and replayed (bf16, one rank).  kv_dtype="fp8" / "fp6" / "fp4": the 8-bit / 6-bit / 4-bit KV cache;
        prefill_chunk=N: the prompt in blocks of N tokens (LLaMAForCausalLM.generate).  top_p as generate()."""
        top_p = _ops._check_top_p(top_p, "generate_vision")
        if self.cfg.sample_mode != "vision":
            raise ValueError("generate_vision() needs sample_mode='vision' (scripts/run_sample_image.sh)")
        B2, S = input_ids.shape
        if B2 % 2:
            raise ValueError("generate_vision: batch = conditional prompts + as many unconditional ones")
        B = B2 // 2
        cfg = torch.as_tensor(cfg_scales, dtype=torch.float32, device=input_ids.device).reshape(-1, 1).expand(B, 1)
        if seed is not None or graph:
            self._check_seed_args(seed, graph, generator)
            out, logits = self._seeded_decode(input_ids, vision_masks, attention_mask, max_length, max_new_tokens,
                                              self._vision_kernel().contiguous(), seed=seed, graph=graph,
                                              temperature=temperature, top_k=top_k, cfg=cfg.reshape(B).contiguous(),
                                              force_period=257, force_token=8192, return_logits=return_logits,
                                              kv_dtype=kv_dtype, prefill_chunk=prefill_chunk, top_p=top_p)
            out = out.to(input_ids.dtype)
            return (out, logits) if return_logits else out
        max_length = max_length or (S + max_new_tokens)
        h, cache, ext, pos = self._prefill(input_ids, vision_masks, attention_mask, max_length, kv_dtype, prefill_chunk)
        head = self._vision_kernel().contiguous()
        out = torch.empty((B, max_new_tokens), dtype=input_ids.dtype, device=input_ids.device)
        logits_out = []
        for i in range(max_new_tokens):
            logits = _head_logits(self, h, head)
            if return_logits:
                logits_out.append(logits.clone())
            cond, uncond = logits[:B], logits[B:]
            tok = self._pick(uncond + cfg * (cond - uncond), temperature, top_k, True, generator, top_p).to(input_ids.dtype)
            if (i + 1) % 257 == 0:
                tok = torch.full_like(tok, 8192)
            out[:, i] = tok[:, 0]
            if i + 1 < max_new_tokens:
                h, pos = self._step(torch.cat([tok, tok], 0), cache, ext, pos)
        return (out, torch.stack(logits_out, 1)) if return_logits else out
