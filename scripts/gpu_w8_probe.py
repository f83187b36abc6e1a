"""Time of the 8-bit (e4m3) decode weights against bf16 weight streaming, one process, the two versions alternated.

  gemv      lwm_gemv_fused_w8 against lwm_gemv_fused_bf16 per LWM-7B projection group (wq|wk|wv and w1|w3 with the RMSNorm
            on load, wo and w2 with the residual and ss_out, lm_head with f32 logits) for 1, 2 and 4 rows.  Every group is
            a RING of copies whose 8-bit packs alone exceed the 256 MiB of last-level cache, walked once per pass inside a
            captured hipGraph (a Python call costs more than a launch pair), device events around whole passes, the two
            versions in alternating windows; median (min - max) of the windows.  Bytes from shapes: weights (+ scales) read
            once, f32 partials written and read once.
  generate  LLaMAForCausalLM.generate(graph=True) milliseconds per token on the 4-layer LWM-7B slice the README quotes
            (scripts/gpu_kv8_decode.py): short prompt / 131072-row cache, bf16 / fp8 weights, bf16 / fp8 cache, two runs each.
  quality   how far the logits of that slice move when its RANDOM weights are rounded to e4m3, and the share of greedy
            tokens kept over 64 steps -- a property of the format on random weights, recorded, not asserted.

    python scripts/gpu_w8_probe.py [--only gemv,generate,quality] [--out profiles/r12_w8_decode.md]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LLC_BYTES = 256 << 20
HID, INTER, VOCAB = 4096, 11008, 32000
GROUPS = (("wq|wk|wv", HID, (HID, HID, HID), "norm"), ("wo", HID, (HID,), "res"), ("w1|w3", HID, (INTER, INTER), "norm"),
          ("w2", INTER, (HID,), "res"), ("lm_head", HID, (VOCAB,), "f32"))


def _spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs))


def gemv_group(name, K, Ns, kind, rows, windows, target_ms):
    from lwm_amd import llama_ops as LO, w8
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    pack_bytes = sum(K * N + ((K + 127) // 128) * N * 4 for N in Ns)
    copies = max(2, -(-2 * LLC_BYTES // pack_bytes))
    ring, packs = [], []
    for _ in range(copies):
        ws = [(torch.randn(K, N, device=dev, generator=gen) * 0.02).to(torch.bfloat16) for N in Ns]
        packs.append([w8.quantise_weight(w) for w in ws])       # (rounds ws in place: both versions stream the same numbers)
        ring.append(ws)
    x = torch.randn(rows, K, device=dev, generator=gen).to(torch.bfloat16)
    kw = {}
    if kind == "norm":
        ss = torch.zeros(rows, 32, device=dev)
        ss[:, 0] = x.float().pow(2).sum(-1)
        kw = dict(norm=(ss, torch.ones(K, device=dev, dtype=torch.bfloat16), 1e-6))
    elif kind == "res":
        kw = dict(residual=torch.randn(rows, Ns[0], device=dev, generator=gen).to(torch.bfloat16), want_ss=True)
    else:
        kw = dict(out_dtype=torch.float32)

    def one_pass(fp8):
        for ws, ps in zip(ring, packs):
            (w8.gemv_fused_w8(x, ps, **kw) if fp8 else LO.gemv_fused(x, ws, **kw))

    graphs = {}
    for fp8 in (False, True):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            one_pass(fp8)                                       # warm: code objects, workspaces
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            one_pass(fp8)
        graphs[fp8] = g
    ms = {False: [], True: []}
    for g in graphs.values():
        g.replay()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    graphs[False].replay()
    torch.cuda.synchronize()
    passes = max(1, int(target_ms / 1e3 / max(time.perf_counter() - t0, 1e-6)))
    for _ in range(windows):
        for fp8 in (False, True):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(passes):
                graphs[fp8].replay()
            e1.record()
            torch.cuda.synchronize()
            ms[fp8].append(e0.elapsed_time(e1) / (passes * copies))
    KS = (K + 127) // 128
    part = sum(2 * KS * rows * N * 4 for N in Ns)
    by = {False: sum(2 * K * N for N in Ns) + part, True: pack_bytes + part}
    out = dict(group=name, rows=rows, K=K, N=list(Ns), copies=copies, passes_per_window=passes)
    for fp8, tag in ((False, "bf16"), (True, "fp8")):
        s = _spread(ms[fp8])
        out[tag] = dict(us=round(s["median"] * 1e3, 2), us_min=round(s["min"] * 1e3, 2), us_max=round(s["max"] * 1e3, 2),
                        mbytes=round(by[fp8] / 1e6, 2), tb_per_s=round(by[fp8] / s["median"] / 1e9, 3))
    out["fp8_over_bf16_time"] = round(out["fp8"]["us"] / out["bf16"]["us"], 3)
    del graphs, ring, packs
    torch.cuda.empty_cache()
    return out


def _slice(max_length, layers=4):
    from lwm_amd.llama import LLaMAConfig, LLaMAForCausalLM
    cfg = LLaMAConfig.load_config("7b", num_hidden_layers=layers, max_sequence_length=max_length, theta=1e7)
    torch.manual_seed(0)
    with torch.device("cuda"):
        return cfg, LLaMAForCausalLM(cfg)


def generate_ms(prompt, max_length, new, short=8, reps=2):
    cfg, model = _slice(max_length)
    model.quantize_decode_weights("fp8")                        # the rounded model, for every leg
    ids = torch.randint(0, cfg.vocab_size, (1, prompt), device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))

    def run(n, weights, kv):
        model.quantize_decode_weights(weights)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        toks = model.generate(ids, max_new_tokens=n, max_length=max_length, graph=True, kv_dtype=kv)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, toks

    legs = [(w, kv) for kv in (None, "fp8") for w in ("bf16", "fp8")]
    for leg in legs:
        run(3, *leg)                                            # warm
    ts, tl, toks = {l: [] for l in legs}, {l: [] for l in legs}, {}
    for _ in range(reps):                                       # alternated
        for leg in legs:
            ts[leg].append(run(short, *leg)[0])
        for leg in legs:
            t, toks[leg] = run(new, *leg)
            tl[leg].append(t)
    out = {"workload": f"generate(graph=True), 4-layer slice of LWM-7B, prompt {prompt}, cache max_length {max_length}, B=1, random "
                       f"weights rounded to e4m3; (run of {new} tokens - run of {short}) / {new - short}, per run and best of {reps}"}
    for w, kv in legs:
        key = f"weights_{w}_cache_{kv or 'bf16'}"
        out[key] = dict(ms_per_token_runs=[round((a - min(ts[(w, kv)])) / (new - short) * 1e3, 3) for a in tl[(w, kv)]],
                        ms_per_token=round((min(tl[(w, kv)]) - min(ts[(w, kv)])) / (new - short) * 1e3, 3))
    out["same_tokens_fp8_vs_bf16_weights"] = {str(kv or "bf16"): bool(torch.equal(toks[("bf16", kv)], toks[("fp8", kv)])) for kv in (None, "fp8")}
    del model
    torch.cuda.empty_cache()
    return out


def quality(steps=64, prompt=512):
    cfg, model = _slice(4096)
    ids = torch.randint(0, cfg.vocab_size, (1, prompt), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    t0, l0 = model.generate(ids, max_new_tokens=steps, return_logits=True)
    model.quantize_decode_weights("fp8")
    t1, l1 = model.generate(ids, max_new_tokens=steps, return_logits=True)
    new0, new1 = t0[0, prompt:], t1[0, prompt:]
    same = (new0 == new1)
    first = int((~same).nonzero()[0]) if not bool(same.all()) else steps
    n = max(first, 1)                                           # the steps that saw the same context (step 0 always does)
    d = (l1[0, :n] - l0[0, :n]).abs()
    del model
    torch.cuda.empty_cache()
    return dict(workload=f"4-layer slice of LWM-7B, RANDOM weights, prompt {prompt}, {steps} greedy steps, unrounded against rounded",
                greedy_tokens_kept=round(float(same.float().mean()), 4), steps_before_first_difference=first,
                max_abs_dlogit=float(d.max()), mean_abs_dlogit=float(d.mean()), max_abs_logit=float(l0[0, :n].abs().max()))


def write_md(path, res):
    with open(path, "w") as f:
        f.write("# 8-bit (e4m3) decode weights against bf16 weight streaming\n\nscripts/gpu_w8_probe.py on " + res["device"] +
                ": one process, the two versions alternated.\n\n")
        if "gemv" in res:
            f.write("## lwm_gemv_fused_w8 against lwm_gemv_fused_bf16 per LWM-7B projection group\n\nEach group is a ring of copies "
                    "(the 8-bit packs alone exceed 256 MiB) walked inside a captured graph; µs per launch pair, median (min - max) of "
                    "the alternating windows; MB = weights (+ scales) + f32 partials written and read, from shapes.\n\n"
                    "| group | rows | bf16 µs | bf16 MB | bf16 TB/s | fp8 µs | fp8 MB | fp8 TB/s | fp8 / bf16 time |\n|---|---|---|---|---|---|---|---|---|\n")
            for r in res["gemv"]:
                b, q = r["bf16"], r["fp8"]
                f.write(f"| {r['group'].replace('|', ', ')} | {r['rows']} | {b['us']} ({b['us_min']} - {b['us_max']}) | {b['mbytes']} | {b['tb_per_s']} | "
                        f"{q['us']} ({q['us_min']} - {q['us_max']}) | {q['mbytes']} | {q['tb_per_s']} | {r['fp8_over_bf16_time']} |\n")
            f.write("\nThe byte ratio allows 0.516.\n\n")
        for key in [k for k in res if k.startswith("generate")]:
            g = res[key]
            f.write(f"## {g['workload']}\n\n| weights | cache | ms / token (runs) | best |\n|---|---|---|---|\n")
            for k, v in g.items():
                if k.startswith("weights_"):
                    _, w, _, kv = k.split("_")
                    f.write(f"| {w} | {kv} | {' / '.join(str(x) for x in v['ms_per_token_runs'])} | {v['ms_per_token']} |\n")
            f.write(f"\nSame tokens with fp8 and bf16 weights (per cache): {g['same_tokens_fp8_vs_bf16_weights']}\n\n")
        if "quality" in res:
            q = res["quality"]
            f.write(f"## Quality on RANDOM weights (recorded, not asserted)\n\n{q['workload']}: greedy tokens kept {q['greedy_tokens_kept']}, "
                    f"{q['steps_before_first_difference']} steps before the first difference; over the steps that saw the same context "
                    f"({max(q['steps_before_first_difference'], 1)}) max |dlogit| "
                    f"{q['max_abs_dlogit']:.4g}, mean |dlogit| {q['mean_abs_dlogit']:.4g} (max |logit| {q['max_abs_logit']:.4g}).\n")
        for k, v in res.get("not_run", {}).items():
            f.write(f"\n**Not run**: {k}: {v}\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="gemv,generate,quality")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--target_ms", type=float, default=60.0, help="device time per window")
    ap.add_argument("--out", default="")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gpu_w8_probe needs an MI355X: a time measured elsewhere says nothing")
    want = set(a.only.split(","))
    res = {"device": torch.cuda.get_device_name(0)}
    with torch.no_grad():
        if "gemv" in want:
            res["gemv"] = []
            for name, K, Ns, kind in GROUPS:
                for rows in (1, 2, 4):
                    res["gemv"].append(gemv_group(name, K, Ns, kind, rows, a.windows, a.target_ms))
                    print(json.dumps(res["gemv"][-1]), flush=True)
        if "generate" in want:
            res["generate_prompt2048_cache32768"] = generate_ms(2048, 32768, 136)
            print(json.dumps(res["generate_prompt2048_cache32768"]), flush=True)
            res["generate_prompt130048_cache131072"] = generate_ms(131072 - 1024, 131072, 72)
            print(json.dumps(res["generate_prompt130048_cache131072"]), flush=True)
        if "quality" in want:
            res["quality"] = quality()
            print(json.dumps(res["quality"]), flush=True)
    for path, dump in ((a.json, lambda f: json.dump(res, f, indent=1)), (a.out, None)):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            if dump:
                with open(path, "w") as f:
                    dump(f)
            else:
                write_md(path, res)


if __name__ == "__main__":
    main()
