"""Chunked prefill over the 8-bit (e4m3) KV cache on the MI355X, measured in one process (csrc/attn_prefill_kv8.h):

  kernel   one block of Q = 4096 queries (B = 1, H = 32) appended at cache index idx, idx + Q in {32768, 131072,
           1048576}: lwm_attn_prefill_kv8 + combine on the 8-bit cache against the bf16 route,
           ringattention_inference(q, kd, vd, None, causal_offset=idx) on kv8_dequant of the same cache -- alternated
           A-B-A-B, device events, medians and spread over the rounds; executed TF/s counts 4 * D flops per visible
           (query, key) pair; the outputs of the two routes are compared at the timed size.
  model    generate(max_new_tokens=1) -- i.e. the prefill -- of a 131072-token prompt on a 4-layer slice of LWM-7B: the
           default cache and the 8-bit cache, one shot and with prefill_chunk=8192; seconds and
           torch.cuda.max_memory_allocated.

Every step runs under a time limit of its own: when one expires the process ends there and starts nothing more on the
GPU.  Results: one JSON document under out/ (and on stdout).

python scripts/gpu_kv8_prefill.py [--only kernel,model] [--out out/kv8_prefill.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gpu_kv8_decode import _events, _spread, limit      # noqa: E402  (the same step limits and timers)


def kernel_step(torch, Sk, Q=4096, H=32, rounds=5):
    from lwm_amd import kv8, ops
    from lwm_amd.ring import _pick_splits
    from lwm_amd.ringattention import ringattention_inference
    idx = Sk - Q
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=g, device="cuda", dtype=torch.float32).to(torch.bfloat16)
    q = rnd(1, Q, H, 128)
    kq, vq = (torch.empty(1, Sk, H, 128, dtype=torch.uint8, device="cuda") for _ in range(2))
    ks, vs = (torch.empty(1, Sk, H, dtype=torch.float32, device="cuda") for _ in range(2))
    step = 65536
    for a in range(0, Sk, step):                                          # (the bf16 source a piece at a time)
        n = min(step, Sk - a)
        ops.kv8_cache_write(kq, ks, rnd(1, n, H, 128), dst_row0=a)
        ops.kv8_cache_write(vq, vs, rnd(1, n, H, 128), dst_row0=a)
    kd, vd = torch.empty(1, Sk, H, 128, dtype=torch.bfloat16, device="cuda"), torch.empty(1, Sk, H, 128, dtype=torch.bfloat16, device="cuda")
    for a in range(0, Sk, step):
        kd[:, a:a + step] = ops.kv8_dequant(kq[:, a:a + step], ks[:, a:a + step])
        vd[:, a:a + step] = ops.kv8_dequant(vq[:, a:a + step], vs[:, a:a + step])
    ns = _pick_splits(1, Q, H, Sk)
    fp8 = lambda: ops.attn_combine(*kv8.attn_prefill_kv8(q, kq, ks, vq, vs, q_start=idx, k_splits=ns), want_bf16=True)[0]
    bf16 = lambda: ringattention_inference(q, kd, vd, None, axis_name="sp", causal_offset=idx)
    o8, ob = fp8(), bf16()
    diff = (o8.float() - ob.float()).abs().max().item() / ob.float().abs().max().item()
    pairs = Q * idx + Q * (Q + 1) // 2
    flops = 4 * 128 * pairs * H
    iters = max(2, min(20, int(1e15 / flops)))
    for f in (bf16, fp8):
        _events(torch, f, 2)                                              # warm
    t = {"bf16": [], "fp8": []}
    for _ in range(rounds):                                               # A-B-A-B
        t["bf16"].append(_events(torch, bf16, iters))
        t["fp8"].append(_events(torch, fp8, iters))
    out = {"shape": f"B=1 H={H} Q={Q} idx={idx} Sk={Sk}, {ns} piece(s); fp8: kernel + combine; bf16: ringattention_inference",
           "rounds": rounds, "iters_per_round": iters, "executed_flops": flops, "out_diff_of_max": diff}
    for n in t:
        out[n] = dict(ms=_spread([x * 1e3 for x in t[n]]), tf_per_s=flops / statistics.median(t[n]) * 1e-12)
    out["fp8_over_bf16_time"] = out["fp8"]["ms"]["median"] / out["bf16"]["ms"]["median"]
    # where the difference sits: the new kernel without its combine, and the SAME kernel class on bf16 operands -- the
    # split-K kernel of attn_fwd.h, which needs two pieces to be chosen -- beside the new kernel at two pieces
    parts = {"fp8 kernel alone (no combine)": lambda: kv8.attn_prefill_kv8(q, kq, ks, vq, vs, q_start=idx, k_splits=ns),
             "fp8 kernel + cast of its one piece (what the model runs at one piece)":
                 lambda: ops.cast_f32_to_bf16(kv8.attn_prefill_kv8(q, kq, ks, vq, vs, q_start=idx, k_splits=1)[0][0]),
             "fp8, 2 pieces + combine": lambda: ops.attn_combine(*kv8.attn_prefill_kv8(q, kq, ks, vq, vs, q_start=idx, k_splits=2)),
             "bf16 split-K kernel (attn_fwd.h), 2 pieces + combine":
                 lambda: ops.attn_combine(*ops.attn_fwd_splitk(q, kd, vd, k_splits=2, q_start=idx, causal=True))}
    out["breakdown_ms"] = {}
    for n, f in parts.items():
        _events(torch, f, 2)
        out["breakdown_ms"][n] = statistics.median(_events(torch, f, iters) * 1e3 for _ in range(3))
    return out


def model_prefill(torch, prompt=131072, chunk=8192, layers=4, reps=2):
    from lwm_amd.llama import LLaMAConfig, LLaMAForCausalLM
    cfg = LLaMAConfig.load_config("7b", num_hidden_layers=layers, max_sequence_length=prompt + 8, theta=1e7)
    torch.manual_seed(0)
    with torch.device("cuda"):
        model = LLaMAForCausalLM(cfg)
    ids = torch.randint(0, cfg.vocab_size, (1, prompt), device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
    weights = torch.cuda.memory_allocated()

    def run(kv, pc):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        toks, logits = model.generate(ids, max_new_tokens=1, max_length=prompt + 8, kv_dtype=kv, prefill_chunk=pc, return_logits=True)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, torch.cuda.max_memory_allocated(), logits

    configs = [("default cache, one shot", None, None), (f"default cache, prefill_chunk={chunk}", None, chunk),
               ("fp8 cache, one shot", "fp8", None), (f"fp8 cache, prefill_chunk={chunk}", "fp8", chunk)]
    out = {"workload": f"generate(max_new_tokens=1) = the prefill of a {prompt}-token prompt, {layers}-layer slice of LWM-7B, B=1, "
                       f"random weights; best of {reps} after one warm run; peak = torch.cuda.max_memory_allocated",
           "weights_and_prompt_bytes": weights}
    ref = None
    for name, kv, pc in configs:
        run(kv, pc)                                                       # warm
        ts, peak, logits = [], 0, None
        for _ in range(reps):
            t, p, logits = run(kv, pc)
            ts.append(t)
            peak = max(peak, p)
        ref = logits if ref is None else ref
        out[name] = dict(seconds=min(ts), peak_bytes=peak, peak_gib=peak / 2 ** 30,
                         logits_diff_vs_default_one_shot_of_max=(logits - ref).abs().max().item() / ref.abs().max().item())
    del model
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="kernel,model")
    ap.add_argument("--out", default=os.path.join(ROOT, "out", "kv8_prefill.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("needs the MI355X")
    want = set(a.only.split(","))
    res = {"device": torch.cuda.get_device_name(0)}
    with torch.no_grad():
        if "kernel" in want:
            for Sk in (32768, 131072, 1048576):
                with limit(f"kernel Sk={Sk}", 180):
                    res[f"kernel_Sk{Sk}"] = kernel_step(torch, Sk)
                torch.cuda.empty_cache()
        if "model" in want:
            with limit("model", 420):
                res["model"] = model_prefill(torch)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
