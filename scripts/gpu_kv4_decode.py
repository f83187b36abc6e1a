"""What the 4-bit (MXFP4) KV cache buys and costs on the MI355X, measured in one process (csrc/attn_decode_kv4.h), beside
the bf16 and the 8-bit caches of the same build:

  attention   one decode attention step (Q = 1, B = 1, H = 32, Sk = 131072 fully visible, _pick_splits pieces): kernel +
              combine for bf16, fp8 and fp4, alternated A-B-C-A-B-C, device events, medians and spread over the rounds;
              achieved TB/s over the bytes the algorithm needs: 2 * Sk * H * (256 | 132 | 68) + Sk (rows, scales, mask).
  write       the one-row cache write (lwm_kv_cache_write_at, lwm_kv8_cache_write_at, lwm_kv4_cache_write_at):
              microseconds per call over a train of launches.
  generate    LLaMAForCausalLM.generate(graph=True) milliseconds per token on the 4-layer LWM-7B slice of bench.py's
              generate_leg (prompt 2048, max_length 32768) and with a 131072-row cache that the prompt nearly fills, for the
              three caches, alternated; per-token time = (long run - short run) / extra tokens.
  footprint   bytes of one layer's cache tensors at LWM-7B shapes for max_length = 1,048,576, times 32 layers.
  needle      the induction needle of tests/_induction.py at 2^20 tokens: the prompt up to the final token is prefilled
              into the cache, the final token is a decode step over it; argmax and margin over the runner-up per cache.

Every step runs under a time limit of its own: when one expires the process ends there and starts nothing more on the
GPU.  Results: one JSON document (rewritten after every step) and the table profiles/r14_kv4_decode.md is made from.

python scripts/gpu_kv4_decode.py [--only attention,write,generate,footprint,needle] [--out out/kv4_decode.json] [--md FILE]"""
import argparse
import contextlib
import json
import os
import signal
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KINDS = (("bf16", None), ("fp8", "fp8"), ("fp4", "fp4"))


@contextlib.contextmanager
def limit(name, seconds):
    """a time limit for one GPU step: on expiry the process ends (status 124) with nothing further started"""
    def expired(signum, frame):
        print(f"step {name!r} exceeded {seconds} s: stopping", file=sys.stderr, flush=True)
        os._exit(124)
    signal.signal(signal.SIGALRM, expired)
    signal.alarm(seconds)
    try:
        yield
    finally:
        signal.alarm(0)


def _events(torch, fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e-3          # seconds per call


def _spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), n=len(xs))


def attention_step(torch, Sk=131072, H=32, rounds=7, iters=20):
    from lwm_amd import kv4, ops
    from lwm_amd.ring import _pick_splits
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=g, device="cuda", dtype=torch.float32).to(torch.bfloat16)
    q, k, v = rnd(1, 1, H, 128), rnd(1, Sk, H, 128), rnd(1, Sk, H, 128)
    k8, v8 = (torch.empty(1, Sk, H, 128, dtype=torch.uint8, device="cuda") for _ in range(2))
    ks8, vs8 = (torch.empty(1, Sk, H, dtype=torch.float32, device="cuda") for _ in range(2))
    ops.kv8_cache_write(k8, ks8, k, dst_row0=0)
    ops.kv8_cache_write(v8, vs8, v, dst_row0=0)
    k4, v4 = (torch.empty(1, Sk, H, 64, dtype=torch.uint8, device="cuda") for _ in range(2))
    ks4, vs4 = (torch.empty(1, Sk, H, 4, dtype=torch.uint8, device="cuda") for _ in range(2))
    kv4.kv4_cache_write(k4, ks4, k, dst_row0=0)
    kv4.kv4_cache_write(v4, vs4, v, dst_row0=0)
    mask = torch.ones(1, 1, Sk, dtype=torch.uint8, device="cuda")
    ns = _pick_splits(1, 1, H, Sk)
    fns = {"bf16": lambda: ops.attn_combine(*ops.attn_fwd_splitk(q, k, v, k_splits=ns, dense_mask=mask)),
           "fp8": lambda: ops.attn_combine(*ops.attn_decode_kv8(q, k8, ks8, v8, vs8, k_splits=ns, dense_mask=mask)),
           "fp4": lambda: ops.attn_combine(*kv4.attn_decode_kv4(q, k4, ks4, v4, vs4, k_splits=ns, dense_mask=mask))}
    # same numbers in both caches for the output comparison: the bf16 kernel on the dequantised 4-bit cache
    ob, _ = ops.attn_combine(*ops.attn_fwd_splitk(q, kv4.kv4_dequant(k4, ks4), kv4.kv4_dequant(v4, vs4), k_splits=ns,
                                                  dense_mask=mask))
    o4, _ = fns["fp4"]()
    diff = (o4.float() - ob.float()).abs().max().item() / ob.float().abs().max().item()
    del ob
    for f in fns.values():
        _events(torch, f, 5)                                              # warm
    t = {n: [] for n in fns}
    for _ in range(rounds):                                               # A-B-C-A-B-C
        for n, f in fns.items():
            t[n].append(_events(torch, f, iters))
    per_head = {"bf16": 256, "fp8": 132, "fp4": 68}
    out = {"shape": f"Q=1 B=1 H={H} Sk={Sk} fully visible, {ns} pieces, kernel + combine", "rounds": rounds,
           "iters_per_round": iters, "fp4_out_diff_vs_bf16_kernel_on_dequantised_cache_of_max": diff}
    for n in t:
        nb = 2 * Sk * H * per_head[n] + Sk
        out[n] = dict(us=_spread([x * 1e6 for x in t[n]]), bytes=nb, tb_per_s=nb / statistics.median(t[n]) * 1e-12)
    for n in ("bf16", "fp8"):
        out[f"fp4_over_{n}_time"] = out["fp4"]["us"]["median"] / out[n]["us"]["median"]
        out[f"fp4_over_{n}_bytes"] = out["fp4"]["bytes"] / out[n]["bytes"]
    return out


def write_step(torch, H=32, rows=32768, rounds=5, iters=500):
    from lwm_amd import kv4, ops
    x = torch.randn(1, 1, H, 128, device="cuda").to(torch.bfloat16)
    cb = torch.zeros(1, rows, H, 128, dtype=torch.bfloat16, device="cuda")
    c8 = torch.zeros(1, rows, H, 128, dtype=torch.uint8, device="cuda")
    s8 = torch.ones(1, rows, H, dtype=torch.float32, device="cuda")
    c4 = torch.zeros(1, rows, H, 64, dtype=torch.uint8, device="cuda")
    s4 = torch.zeros(1, rows, H, 4, dtype=torch.uint8, device="cuda")
    idx = torch.tensor([1234], dtype=torch.int32, device="cuda")
    fns = {"bf16": lambda: ops.kv_cache_write_at(cb, x, idx), "fp8": lambda: ops.kv8_cache_write_at(c8, s8, x, idx),
           "fp4": lambda: kv4.kv4_cache_write_at(c4, s4, x, idx)}
    for f in fns.values():
        _events(torch, f, 50)
    t = {n: [] for n in fns}
    for _ in range(rounds):
        for n, f in fns.items():
            t[n].append(_events(torch, f, iters) * 1e6)
    return {"shape": f"one row, H={H}, launches issued back to back", **{n + "_us": _spread(t[n]) for n in t}}


def generate_ms(torch, prompt, max_length, new, short=8, layers=4, reps=2):
    from lwm_amd.llama import LLaMAConfig, LLaMAForCausalLM
    cfg = LLaMAConfig.load_config("7b", num_hidden_layers=layers, max_sequence_length=max_length, theta=1e7)
    torch.manual_seed(0)
    with torch.device("cuda"):
        model = LLaMAForCausalLM(cfg)
    ids = torch.randint(0, cfg.vocab_size, (1, prompt), device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))

    def run(n, kv):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        toks = model.generate(ids, max_new_tokens=n, max_length=max_length, graph=True, kv_dtype=kv)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, toks

    for _, kv in KINDS:
        run(3, kv)                                                        # warm
    ts, tl = {n: [] for n, _ in KINDS}, {n: [] for n, _ in KINDS}
    for _ in range(reps):                                                 # alternated
        for n, kv in KINDS:
            ts[n].append(run(short, kv)[0])
        for n, kv in KINDS:
            tl[n].append(run(new, kv)[0])
    out = {"workload": f"generate(graph=True), {layers}-layer slice of LWM-7B, prompt {prompt}, cache max_length {max_length}, "
                       f"B=1, random weights; (run of {new} tokens - run of {short}) / {new - short}, best of {reps}"}
    for n, _ in KINDS:
        out[n + "_ms_per_token"] = (min(tl[n]) - min(ts[n])) / (new - short) * 1e3
    for n in ("bf16", "fp8"):
        out[f"fp4_over_{n}"] = out["fp4_ms_per_token"] / out[n + "_ms_per_token"]
    del model
    torch.cuda.empty_cache()
    return out


def footprint(torch, max_length=1 << 20):
    from lwm_amd.llama import LLaMAConfig, LLaMAForCausalLM
    cfg = LLaMAConfig.load_config("7b", num_hidden_layers=1, max_sequence_length=max_length, theta=5e7)
    with torch.device("cuda"):
        model = LLaMAForCausalLM(cfg)
    out = {"max_length": max_length, "layers": 32}
    for name, kv in reversed(KINDS):
        layer = model.init_cache(1, max_length, kv_dtype=kv)[0]
        b = sum(t.numel() * t.element_size() for t in layer.values() if torch.is_tensor(t))
        out[name] = dict(bytes_one_layer=b, gib_32_layers=b * 32 / 2 ** 30, kib_per_token=b * 32 / max_length / 1024)
        del layer
        torch.cuda.empty_cache()
    return out


def needle(torch, S=1 << 20, theta=5e7, depth=0.35):
    from lwm_amd.llama import LLaMAConfig, LLaMAForCausalLM
    from lwm_amd.weights import load_params
    from tests import _induction as I
    cfg_kw, st = I.build(theta, S)
    cfg = LLaMAConfig(**cfg_kw, scan_mlp_chunk_size=(S - 1) // 25)
    with torch.device("cuda"):
        model = load_params(LLaMAForCausalLM(cfg), st)
    toks, pos = I.haystack(S, depth)
    toks = toks.cuda()
    ar = torch.arange(S, dtype=torch.int32, device="cuda")[None]
    out = {"tokens": S, "depth": depth, "needle_at": int(pos), "value_token": int(I.VALUE_TOKEN)}
    for name, kv in KINDS:
        cache = model.init_cache(1, S, kv_dtype=kv)
        model.hidden_states(toks[:, :S - 1], None, None, ar[:, :S - 1].contiguous(), cache)
        h = model.hidden_states(toks[:, S - 1:], None, None, ar[:, S - 1:].contiguous(), cache)
        logits = (h[0, -1].float() @ model.lm_head.float()).cpu()
        top = logits.topk(2)
        out[name] = dict(argmax=top.indices[0].item(), margin=(top.values[0] - top.values[1]).item(),
                         on_value=bool(top.indices[0].item() == I.VALUE_TOKEN))
        del cache, h
        torch.cuda.empty_cache()
    return out


def markdown(res):
    """the table of profiles/r14_kv4_decode.md from the JSON document"""
    L = [f"# The 4-bit (MXFP4) KV cache beside the bf16 and the 8-bit cache ({res.get('device', '?')})", "",
         "Made by `scripts/gpu_kv4_decode.py`; every figure below is from one run of it.", ""]
    if "attention" in res:
        a = res["attention"]
        L += [f"## One decode attention step: {a['shape']}", "", f"{a['rounds']} alternated rounds of {a['iters_per_round']} calls; "
              "median (min .. max) microseconds per call; TB/s over the algorithmic bytes.", "",
              "| cache | us per step | bytes | TB/s |", "|---|---|---|---|"]
        for n in ("bf16", "fp8", "fp4"):
            u = a[n]["us"]
            L.append(f"| {n} | {u['median']:.1f} ({u['min']:.1f} .. {u['max']:.1f}) | {a[n]['bytes']} | {a[n]['tb_per_s']:.2f} |")
        L += ["", f"fp4 / bf16: time {a['fp4_over_bf16_time']:.3f}, bytes {a['fp4_over_bf16_bytes']:.3f}.  "
              f"fp4 / fp8: time {a['fp4_over_fp8_time']:.3f}, bytes {a['fp4_over_fp8_bytes']:.3f}.  "
              f"fp4 output against the bf16 kernel on the dequantised cache: {a['fp4_out_diff_vs_bf16_kernel_on_dequantised_cache_of_max']:.2e} of max.", ""]
    if "write" in res:
        w = res["write"]
        L += [f"## The one-row write ({w['shape']})", "", "| cache | us per call, median (min .. max) |", "|---|---|"]
        L += [f"| {n} | {w[n + '_us']['median']:.2f} ({w[n + '_us']['min']:.2f} .. {w[n + '_us']['max']:.2f}) |" for n in ("bf16", "fp8", "fp4")]
        L.append("")
    for key in sorted(k for k in res if k.startswith("generate_")):
        gm = res[key]
        L += [f"## {gm['workload']}", "", "| cache | ms per token |", "|---|---|"]
        L += [f"| {n} | {gm[n + '_ms_per_token']:.3f} |" for n in ("bf16", "fp8", "fp4")]
        L += ["", f"fp4 / bf16 {gm['fp4_over_bf16']:.3f}; fp4 / fp8 {gm['fp4_over_fp8']:.3f}.", ""]
    if "footprint" in res:
        fp = res["footprint"]
        L += [f"## Footprint at max_length {fp['max_length']}, LWM-7B shapes, {fp['layers']} layers", "",
              "| cache | KiB per token | GiB |", "|---|---|---|"]
        L += [f"| {n} | {fp[n]['kib_per_token']:.0f} | {fp[n]['gib_32_layers']:.0f} |" for n in ("bf16", "fp8", "fp4")]
        L.append("")
    if "needle" in res:
        nd = res["needle"]
        L += [f"## Induction needle at {nd['tokens']} tokens (depth {nd['depth']}, needle at {nd['needle_at']}, planted value token "
              f"{nd['value_token']})", "", "| cache | argmax | on the planted value | margin over the runner-up |", "|---|---|---|---|"]
        L += [f"| {n} | {nd[n]['argmax']} | {'yes' if nd[n]['on_value'] else '**no**'} | {nd[n]['margin']:.3f} |" for n in ("bf16", "fp8", "fp4")]
        L.append("")
    return "\n".join(L)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="attention,write,generate,footprint,needle")
    ap.add_argument("--out", default=os.path.join(ROOT, "out", "kv4_decode.json"))
    ap.add_argument("--md", default=None, help="also write the markdown table here")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("needs the MI355X")
    want = set(a.only.split(","))
    res = {"device": torch.cuda.get_device_name(0)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def save():
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        if a.md:
            with open(a.md, "w") as f:
                f.write(markdown(res))

    with torch.no_grad():
        if "attention" in want:
            with limit("attention", 150):
                res["attention"] = attention_step(torch)
            save()
        if "write" in want:
            with limit("write", 60):
                res["write"] = write_step(torch)
            save()
        if "footprint" in want:
            with limit("footprint", 60):
                res["footprint"] = footprint(torch)
            save()
        if "generate" in want:
            with limit("generate short prompt", 300):
                res["generate_prompt2048_cache32768"] = generate_ms(torch, 2048, 32768, 136)
            save()
            with limit("generate long prompt", 540):
                res["generate_prompt130048_cache131072"] = generate_ms(torch, 131072 - 1024, 131072, 72)
            save()
        if "needle" in want:
            with limit("needle", 540):
                res["needle"] = needle(torch)
            save()
    save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
