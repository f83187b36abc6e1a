"""What per-block activation recompute (LLaMAForCausalLM.remat_blocks, lwm_amd/remat.py) costs and saves on the step it was
built for: LWM-7B, all 32 layers, bf16, B = 1, forward + backward on one MI355X -- bench.py's `model_full` configuration
(scan_mlp=False, every step re-lays its kernels as a training step would).

  1. S = 32768: step time and max_memory_allocated, remat off and on in ALTERNATING steps of one process after a warm-up
     of each (the clock wanders under load: medians and ranges of the repetitions);
  2. the bytes per token and layer a step HOLDS between its forward and its backward (memory_allocated after the forward,
     over the tokens and the layers), off and on, beside remat.saved_bytes;
  3. S = 131072, remat on only -- and only when the footprint computed first is under --limit-gib: tokens/s, peak, and the
     attention kernels' share of the step (device events around the attention launches).  The off case at that length is
     computed, not run.

Every step runs under a watchdog of its own (--step-timeout seconds: a step that has not returned by then ends the
process with a traceback; nothing more is started).

    python scripts/gpu_remat_probe.py [--reps 3] [--layers 32] [--out profiles/r24_remat.md]
"""
import argparse
import faulthandler
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GIB = float(1 << 30)
UNREMAT_BYTES_PER_TOKEN_LAYER = 132e3      # the un-remat path's kept activations at LWM-7B shapes (README: model_full)


def watched(seconds, fn):
    """fn() under a watchdog of its own: past `seconds` the process ends with every thread's traceback"""
    faulthandler.dump_traceback_later(seconds, exit=True)
    try:
        return fn()
    finally:
        faulthandler.cancel_dump_traceback_later()


def predicted_gib(S, layers, cfg, n_params, remat):
    """the footprint of a step, from the formulas: kept activations (+ one live layer with remat), parameters, gradients,
    the re-laid copies of the projections (llama_ops._relayout: wt for every kernel, wcat for wq|wk|wv and w1|w3), the
    chunked head's logits"""
    from lwm_amd import remat as R
    d, F, H = cfg.hidden_size, cfg.intermediate_size, cfg.num_attention_heads
    kept = R.saved_bytes(1, S, d, H, torch.bfloat16) * layers if remat else UNREMAT_BYTES_PER_TOKEN_LAYER * S * layers
    live = 2 * UNREMAT_BYTES_PER_TOKEN_LAYER * S if remat else 0           # one layer's graph and as much again of gradients in flight
    relayout = layers * 2 * ((4 * d * d + 3 * d * F) + (3 * d * d + 2 * d * F))
    head = 3 * 8192 * cfg.vocab_size * 4
    return (kept + live + 2 * 2 * n_params + relayout + head) / GIB


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--seq", type=int, default=32768)
    ap.add_argument("--long-seq", type=int, default=131072)
    ap.add_argument("--limit-gib", type=float, default=260.0)
    ap.add_argument("--step-timeout", type=int, default=180)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gpu_remat_probe needs an MI355X: a time measured elsewhere says nothing")
    from lwm_amd import remat as R
    from lwm_amd import ring as ring_mod
    from lwm_amd.llama import LLaMAConfig, LLaMAForCausalLM
    from lwm_amd.llama_ops import use_tuned_gemms, weights_changed
    L, S = a.layers, a.seq
    cfg = LLaMAConfig.load_config("7b", num_hidden_layers=L, max_sequence_length=max(S, a.long_seq), theta=1e7, scan_mlp=False)
    torch.manual_seed(0)
    with torch.device("cuda"):
        model = LLaMAForCausalLM(cfg)
    n_params = sum(p.numel() for p in model.parameters())
    tuned = use_tuned_gemms()
    d, H = cfg.hidden_size, cfg.num_attention_heads

    # device events around the attention launches (the per-block kernels of lwm_amd.ring.HipBlockOps)
    spans = []
    for name in ("fwd", "bwd_delta", "bwd_dq", "bwd_dkdv"):
        real = getattr(ring_mod.HipBlockOps, name)

        def timed(*args, _real=real, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = _real(*args, **kw)
            e1.record()
            spans.append((e0, e1))
            return out
        setattr(ring_mod.HipBlockOps, name, staticmethod(timed))

    def step(tok, on):
        """-> (ms, held bytes after the forward, peak bytes, attention ms, loss)"""
        model.remat_blocks = on
        model.zero_grad(set_to_none=True)
        spans.clear()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        weights_changed()
        loss, _ = model.loss(tok[:, :-1], tok[:, 1:], chunk=8192)
        held = torch.cuda.memory_allocated() - base
        loss.backward()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        return ms, held, torch.cuda.max_memory_allocated(), sum(e0.elapsed_time(e1) for e0, e1 in spans), float(loss.detach())

    res = dict(parameters=n_params, layers=L, tuned_gemm_solutions=tuned, saved_bytes_per_token_layer=R.saved_bytes(1, 1, d, H, torch.bfloat16))
    tok = torch.randint(0, cfg.vocab_size, (1, S + 1), device="cuda")
    runs = {False: [], True: []}
    for on in (False, True):                       # warm-up of each: workspaces, code objects, the library's choices
        watched(a.step_timeout, lambda: step(tok, on))
    for _ in range(a.reps):
        for on in (False, True):
            runs[on].append(watched(a.step_timeout, lambda: step(tok, on)))
    short = {}
    for on, rs in runs.items():
        ms = [r[0] for r in rs]
        short["on" if on else "off"] = dict(
            ms_median=statistics.median(ms), ms_min=min(ms), ms_max=max(ms), peak_gib=max(r[2] for r in rs) / GIB,
            held_bytes_per_token_layer=statistics.median(r[1] for r in rs) / (S * L),
            attention_ms=statistics.median(r[3] for r in rs), losses=sorted({r[4] for r in rs}),
            predicted_gib=predicted_gib(S, L, cfg, n_params, on))
    short["time_ratio"] = short["on"]["ms_median"] / short["off"]["ms_median"]
    res["short"] = dict(seq=S, reps=a.reps, **short)
    print(json.dumps(res["short"]), flush=True)

    # the long sequence: computed first, run only if it fits; the dS hand-over workspace of the short steps goes first
    SL = a.long_seq
    pred_on, pred_off = predicted_gib(SL, L, cfg, n_params, True), predicted_gib(SL, L, cfg, n_params, False)
    long = dict(seq=SL, predicted_gib_on=pred_on, predicted_gib_off=pred_off, ran=False)
    if pred_on < a.limit_gib:
        del tok
        ring_mod._ds_cache.clear()
        torch.cuda.empty_cache()
        tokl = torch.randint(0, cfg.vocab_size, (1, SL + 1), device="cuda")
        watched(4 * a.step_timeout, lambda: step(tokl, True))
        ms, held, peak, attn_ms, loss = watched(4 * a.step_timeout, lambda: step(tokl, True))
        long.update(ran=True, ms=ms, tokens_per_s=SL / (ms * 1e-3), peak_gib=peak / GIB, attention_ms=attn_ms, attention_share=attn_ms / ms,
                    held_bytes_per_token_layer=held / (SL * L), loss=loss)
    res["long"] = long
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        o, n = short["off"], short["on"]
        with open(a.out, "w") as f:
            f.write(f"# Per-block activation recompute: LWM-7B, {L} layers ({n_params / 1e9:.2f} B parameters), bf16, B = 1, one MI355X\n\n"
                    f"scripts/gpu_remat_probe.py: one process, `scan_mlp=False`, every step re-lays its kernels (bench.py's `model_full`); "
                    f"remat off and on in alternating steps after a warm-up of each, {a.reps} repetitions, median (min - max); wall clock "
                    f"around a synchronised step; peak = `max_memory_allocated`; held = `memory_allocated` after the forward less before "
                    f"it, over tokens x layers; attention = device events around the attention launches.  Tuned GEMM solutions: {tuned}.\n\n"
                    f"## S = {S}\n\n| remat | ms / step | peak GiB | computed GiB | held bytes / token / layer | attention ms |\n|---|---|---|---|---|---|\n")
            for tag, r in (("off", o), ("on", n)):
                f.write(f"| {tag} | {r['ms_median']:.1f} ({r['ms_min']:.1f} - {r['ms_max']:.1f}) | {r['peak_gib']:.1f} | {r['predicted_gib']:.1f} | "
                        f"{r['held_bytes_per_token_layer']:.0f} | {r['attention_ms']:.1f} |\n")
            f.write(f"\nTime ratio on / off: **{short['time_ratio']:.3f}** (estimate from the step's shares: 1.16; measured / estimate "
                    f"{short['time_ratio'] / 1.16:.3f}).  Peak on / off: {n['peak_gib'] / o['peak_gib']:.3f} (estimate: about 70 of 166 GiB = 0.42).  "
                    f"`remat.saved_bytes` per token and layer: {res['saved_bytes_per_token_layer']} bytes; the un-remat estimate: "
                    f"{UNREMAT_BYTES_PER_TOKEN_LAYER:.0f}.  Losses of all steps: off {o['losses']}, on {n['losses']}.\n\n## S = {SL}\n\n")
            f.write("| remat | tokens / s | ms / step | peak GiB | computed GiB | attention share | held bytes / token / layer |\n|---|---|---|---|---|---|---|\n")
            f.write(f"| off | does not fit (computed) | | | {pred_off:.0f} | | |\n")
            if long["ran"]:
                f.write(f"| on | {long['tokens_per_s']:.0f} | {long['ms']:.0f} | {long['peak_gib']:.1f} | {pred_on:.0f} | {long['attention_share']:.3f} | "
                        f"{long['held_bytes_per_token_layer']:.0f} |\n")
            else:
                f.write(f"| on | not run: the computed footprint is over {a.limit_gib:.0f} GiB | | | {pred_on:.0f} | | |\n")
            f.write("\n```json\n" + json.dumps(res, indent=1) + "\n```\n")


if __name__ == "__main__":
    main()
