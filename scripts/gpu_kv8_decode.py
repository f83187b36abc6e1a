"""What the 8-bit (e4m3) KV cache buys on the MI355X, measured in one process (csrc/attn_decode_kv8.h):

  attention   one decode attention step (Q = 1, B = 1, H = 32, Sk = 131072 fully visible, _pick_splits pieces): the
              8-bit kernel + combine against the bf16 kernel + combine, alternated A-B-A-B, device events, medians
              and spread over the rounds; achieved TB/s with the bytes the algorithm needs counted as
              2 * Sk * (4096 + 128) + Sk (rows, scales, mask) against 2 * Sk * 8192 + Sk.
  write       the quantising write of one row (lwm_kv8_cache_write_at) against the bf16 copy (lwm_kv_cache_write_at):
              microseconds per call over a train of launches (both are launch-bound; a decode step issues 64 of them).
  generate    LLaMAForCausalLM.generate(graph=True) milliseconds per token on the 4-layer LWM-7B slice of bench.py's
              generate_leg (prompt 2048, max_length 32768) and with a 131072-row cache that the prompt nearly fills,
              bf16 cache against kv_dtype="fp8", alternated; per-token time = (long run - short run) / extra tokens.
  footprint   bytes of one layer's cache tensors at LWM-7B shapes for max_length = 1,048,576, times 32 layers.

Every step runs under a time limit of its own: when one expires the process ends there and starts nothing more on the
GPU.  Results: one JSON document under out/ (and on stdout).

python scripts/gpu_kv8_decode.py [--only attention,write,generate,footprint] [--out out/kv8_decode.json]"""
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
    from lwm_amd import ops
    from lwm_amd.ring import _pick_splits
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=g, device="cuda", dtype=torch.float32).to(torch.bfloat16)
    q, k, v = rnd(1, 1, H, 128), rnd(1, Sk, H, 128), rnd(1, Sk, H, 128)
    kq, vq = (torch.empty(1, Sk, H, 128, dtype=torch.uint8, device="cuda") for _ in range(2))
    ks, vs = (torch.empty(1, Sk, H, dtype=torch.float32, device="cuda") for _ in range(2))
    ops.kv8_cache_write(kq, ks, k, dst_row0=0)
    ops.kv8_cache_write(vq, vs, v, dst_row0=0)
    mask = torch.ones(1, 1, Sk, dtype=torch.uint8, device="cuda")
    ns = _pick_splits(1, 1, H, Sk)
    bf16 = lambda: ops.attn_combine(*ops.attn_fwd_splitk(q, k, v, k_splits=ns, dense_mask=mask))
    fp8 = lambda: ops.attn_combine(*ops.attn_decode_kv8(q, kq, ks, vq, vs, k_splits=ns, dense_mask=mask))
    # same numbers in both caches for the output comparison: the bf16 kernel on the dequantised cache
    ob, _ = ops.attn_combine(*ops.attn_fwd_splitk(q, ops.kv8_dequant(kq, ks), ops.kv8_dequant(vq, vs), k_splits=ns,
                                                  dense_mask=mask))
    o8, _ = fp8()
    diff = (o8.float() - ob.float()).abs().max().item() / ob.float().abs().max().item()
    for f in (bf16, fp8):
        _events(torch, f, 5)                                              # warm
    t = {"bf16": [], "fp8": []}
    for _ in range(rounds):                                               # A-B-A-B
        t["bf16"].append(_events(torch, bf16, iters))
        t["fp8"].append(_events(torch, fp8, iters))
    row = H * 128
    nbytes = {"bf16": 2 * Sk * 2 * row + Sk, "fp8": 2 * Sk * (row + 4 * H) + Sk}
    out = {"shape": f"Q=1 B=1 H={H} Sk={Sk} fully visible, {ns} pieces, kernel + combine", "rounds": rounds,
           "iters_per_round": iters, "out_diff_vs_bf16_kernel_on_dequantised_cache_of_max": diff}
    for n in t:
        out[n] = dict(us=_spread([x * 1e6 for x in t[n]]), bytes=nbytes[n], tb_per_s=nbytes[n] / statistics.median(t[n]) * 1e-12)
    out["fp8_over_bf16_time"] = out["fp8"]["us"]["median"] / out["bf16"]["us"]["median"]
    out["fp8_over_bf16_bytes"] = nbytes["fp8"] / nbytes["bf16"]
    return out


def write_step(torch, H=32, rows=32768, rounds=5, iters=500):
    from lwm_amd import ops
    x = torch.randn(1, 1, H, 128, device="cuda").to(torch.bfloat16)
    cb = torch.zeros(1, rows, H, 128, dtype=torch.bfloat16, device="cuda")
    c8 = torch.zeros(1, rows, H, 128, dtype=torch.uint8, device="cuda")
    s8 = torch.ones(1, rows, H, dtype=torch.float32, device="cuda")
    idx = torch.tensor([1234], dtype=torch.int32, device="cuda")
    bf16 = lambda: ops.kv_cache_write_at(cb, x, idx)
    fp8 = lambda: ops.kv8_cache_write_at(c8, s8, x, idx)
    for f in (bf16, fp8):
        _events(torch, f, 50)
    t = {"bf16": [], "fp8": []}
    for _ in range(rounds):
        t["bf16"].append(_events(torch, bf16, iters) * 1e6)
        t["fp8"].append(_events(torch, fp8, iters) * 1e6)
    return {"shape": f"one row, H={H}, launches issued back to back", "bf16_us": _spread(t["bf16"]), "fp8_us": _spread(t["fp8"])}


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

    kinds = (("bf16", None), ("fp8", "fp8"))
    for _, kv in kinds:
        run(3, kv)                                                        # warm
    ts, tl = {n: [] for n, _ in kinds}, {n: [] for n, _ in kinds}
    for _ in range(reps):                                                 # alternated
        for n, kv in kinds:
            ts[n].append(run(short, kv)[0])
        for n, kv in kinds:
            tl[n].append(run(new, kv)[0])
    out = {"workload": f"generate(graph=True), {layers}-layer slice of LWM-7B, prompt {prompt}, cache max_length {max_length}, "
                       f"B=1, random weights; (run of {new} tokens - run of {short}) / {new - short}, best of {reps}"}
    for n, _ in kinds:
        out[n + "_ms_per_token"] = (min(tl[n]) - min(ts[n])) / (new - short) * 1e3
    out["fp8_over_bf16"] = out["fp8_ms_per_token"] / out["bf16_ms_per_token"]
    del model
    torch.cuda.empty_cache()
    return out


def footprint(torch, max_length=1 << 20):
    from lwm_amd.llama import LLaMAConfig, LLaMAForCausalLM
    cfg = LLaMAConfig.load_config("7b", num_hidden_layers=1, max_sequence_length=max_length, theta=5e7)
    with torch.device("cuda"):
        model = LLaMAForCausalLM(cfg)
    out = {"max_length": max_length, "layers": 32}
    for name, kv in (("fp8", "fp8"), ("bf16", None)):
        layer = model.init_cache(1, max_length, kv_dtype=kv)[0]
        b = sum(t.numel() * t.element_size() for t in layer.values() if torch.is_tensor(t))
        out[name] = dict(bytes_one_layer=b, gib_32_layers=b * 32 / 2 ** 30, kib_per_token=b * 32 / max_length / 1024)
        del layer
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="attention,write,generate,footprint")
    ap.add_argument("--out", default=os.path.join(ROOT, "out", "kv8_decode.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("needs the MI355X")
    want = set(a.only.split(","))
    res = {"device": torch.cuda.get_device_name(0)}
    with torch.no_grad():
        if "attention" in want:
            with limit("attention", 120):
                res["attention"] = attention_step(torch)
        if "write" in want:
            with limit("write", 60):
                res["write"] = write_step(torch)
        if "generate" in want:
            with limit("generate short prompt", 240):
                res["generate_prompt2048_cache32768"] = generate_ms(torch, 2048, 32768, 136)
            with limit("generate long prompt", 420):
                res["generate_prompt130048_cache131072"] = generate_ms(torch, 131072 - 1024, 131072, 72)
        if "footprint" in want:
            with limit("footprint", 60):
                res["footprint"] = footprint(torch)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
