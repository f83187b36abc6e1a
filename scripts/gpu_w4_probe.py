"""Time of the 4-bit (MXFP4) decode weights against the 8-bit packs and bf16 weight streaming, one process, the three versions
alternated.  The protocol and the machinery are scripts/gpu_w8_probe.py's.

  gemv      lwm_gemv_fused_w4 / lwm_gemv_fused_w8 / lwm_gemv_fused_bf16 per LWM-7B projection group (wq|wk|wv and w1|w3 with
            the RMSNorm on load, wo and w2 with the residual and ss_out, lm_head with f32 logits) for 1 and 4 rows.  Every
            group is a RING of copies whose 4-bit packs alone exceed the 256 MiB of last-level cache, walked once per pass
            inside a captured hipGraph, device events around whole passes, the three versions in alternating windows; median
            (min - max) of the windows.  Bytes from shapes: weights (+ scales) read once, f32 partials written and read once.
            The kernels are rounded to MXFP4 first and to e4m3 after: with one magnitude per kernel the 4-bit values are e4m3
            values, so the three versions stream the same numbers.
  generate  LLaMAForCausalLM.generate(graph=True) milliseconds per token on the 4-layer LWM-7B slice the README quotes:
            short prompt / 131072-row cache, bf16 / fp8 / fp4 weights, bf16 cache, two runs each.
  quality   how far the logits of that slice move when its RANDOM weights are rounded to MXFP4, and the share of greedy
            tokens kept over 64 steps -- a property of the format on random weights, recorded, not asserted.

    python scripts/gpu_w4_probe.py [--only gemv,generate,quality] [--out profiles/r18_w4_decode.md]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gpu_w8_probe import GROUPS, LLC_BYTES, _slice, _spread  # noqa: E402

FORMATS = ("bf16", "fp8", "fp4")


def gemv_group(name, K, Ns, kind, rows, windows, target_ms):
    from lwm_amd import llama_ops as LO, w4, w8
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    wbytes = {"bf16": sum(2 * K * N for N in Ns), "fp8": sum(K * N + ((K + 127) // 128) * N * 4 for N in Ns),
              "fp4": sum(K * N // 2 + (K // 32) * N for N in Ns)}
    copies = max(2, -(-2 * LLC_BYTES // wbytes["fp4"]))
    ring, packs8, packs4 = [], [], []
    for _ in range(copies):
        ws = [(torch.randn(K, N, device=dev, generator=gen) * 0.02).to(torch.bfloat16) for N in Ns]
        packs4.append([w4.quantise_weight(w) for w in ws])      # (rounds ws in place ...
        packs8.append([w8.quantise_weight(w) for w in ws])      # ... and MXFP4 values of one magnitude are e4m3 values)
        ring.append(ws)
    same_numbers = all(torch.equal(w4.w4_dequant(p.q, p.scale, p.shape), w) for p, w in zip(packs4[0], ring[0]))
    x = torch.randn(rows, K, device=dev, generator=gen).to(torch.bfloat16)
    if kind == "norm":
        ss = torch.zeros(rows, 32, device=dev)
        ss[:, 0] = x.float().pow(2).sum(-1)
        kw = dict(norm=(ss, torch.ones(K, device=dev, dtype=torch.bfloat16), 1e-6))
    elif kind == "res":
        kw = dict(residual=torch.randn(rows, Ns[0], device=dev, generator=gen).to(torch.bfloat16), want_ss=True)
    else:
        kw = dict(out_dtype=torch.float32)

    def one_pass(fmt):
        for ws, p8, p4 in zip(ring, packs8, packs4):
            if fmt == "fp4":
                w4.gemv_fused_w4(x, p4, **kw)
            elif fmt == "fp8":
                w8.gemv_fused_w8(x, p8, **kw)
            else:
                LO.gemv_fused(x, ws, **kw)

    graphs = {}
    for fmt in FORMATS:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            one_pass(fmt)                                       # warm: code objects, workspaces
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            one_pass(fmt)
        graphs[fmt] = g
    ms = {fmt: [] for fmt in FORMATS}
    for g in graphs.values():
        g.replay()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    graphs["bf16"].replay()
    torch.cuda.synchronize()
    passes = max(1, int(target_ms / 1e3 / max(time.perf_counter() - t0, 1e-6)))
    for _ in range(windows):
        for fmt in FORMATS:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(passes):
                graphs[fmt].replay()
            e1.record()
            torch.cuda.synchronize()
            ms[fmt].append(e0.elapsed_time(e1) / (passes * copies))
    part = sum(2 * ((K + 127) // 128) * rows * N * 4 for N in Ns)
    out = dict(group=name, rows=rows, K=K, N=list(Ns), copies=copies, passes_per_window=passes, same_numbers=bool(same_numbers))
    for fmt in FORMATS:
        s = _spread(ms[fmt])
        by = wbytes[fmt] + part
        out[fmt] = dict(us=round(s["median"] * 1e3, 2), us_min=round(s["min"] * 1e3, 2), us_max=round(s["max"] * 1e3, 2),
                        mbytes=round(by / 1e6, 2), tb_per_s=round(by / s["median"] / 1e9, 3))
    out["fp4_over_fp8_time"] = round(out["fp4"]["us"] / out["fp8"]["us"], 3)
    out["fp4_over_bf16_time"] = round(out["fp4"]["us"] / out["bf16"]["us"], 3)
    # beyond the probe's own spread: the whole min - max range of one version lies on one side of the other's
    out["fp4_beats_fp8_beyond_spread"] = bool(out["fp4"]["us_max"] < out["fp8"]["us_min"])
    out["fp8_beats_fp4_beyond_spread"] = bool(out["fp8"]["us_max"] < out["fp4"]["us_min"])
    del graphs, ring, packs8, packs4
    torch.cuda.empty_cache()
    return out


def generate_ms(prompt, max_length, new, short=8, reps=2):
    cfg, model = _slice(max_length)
    model.quantize_decode_weights("fp4").quantize_decode_weights("fp8")       # the rounded model, for every leg
    ids = torch.randint(0, cfg.vocab_size, (1, prompt), device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))

    def run(n, weights):
        model.quantize_decode_weights(weights)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        toks = model.generate(ids, max_new_tokens=n, max_length=max_length, graph=True)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, toks

    for w in FORMATS:
        run(3, w)                                               # warm
    ts, tl, toks = {w: [] for w in FORMATS}, {w: [] for w in FORMATS}, {}
    for _ in range(reps):                                       # alternated
        for w in FORMATS:
            ts[w].append(run(short, w)[0])
        for w in FORMATS:
            t, toks[w] = run(new, w)
            tl[w].append(t)
    out = {"workload": f"generate(graph=True), 4-layer slice of LWM-7B, prompt {prompt}, cache max_length {max_length}, B=1, bf16 "
                       f"cache, random weights rounded to MXFP4; (run of {new} tokens - run of {short}) / {new - short}, per run "
                       f"and best of {reps}"}
    for w in FORMATS:
        out[f"weights_{w}"] = dict(ms_per_token_runs=[round((a - min(ts[w])) / (new - short) * 1e3, 3) for a in tl[w]],
                                   ms_per_token=round((min(tl[w]) - min(ts[w])) / (new - short) * 1e3, 3))
    out["same_tokens_as_bf16_weights"] = {w: bool(torch.equal(toks["bf16"], toks[w])) for w in ("fp8", "fp4")}
    del model
    torch.cuda.empty_cache()
    return out


def quality(steps=64, prompt=512):
    cfg, model = _slice(4096)
    ids = torch.randint(0, cfg.vocab_size, (1, prompt), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    t0, l0 = model.generate(ids, max_new_tokens=steps, return_logits=True)
    model.quantize_decode_weights("fp4")
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
        f.write("# 4-bit (MXFP4) decode weights against the 8-bit packs and bf16 weight streaming\n\nscripts/gpu_w4_probe.py on " +
                res["device"] + ": one process, the three versions alternated.\n\n")
        if "gemv" in res:
            f.write("## lwm_gemv_fused_w4 / _w8 / _bf16 per LWM-7B projection group\n\nEach group is a ring of copies (the 4-bit packs "
                    "alone exceed 256 MiB) walked inside a captured graph; µs per launch pair, median (min - max) of the alternating "
                    "windows; MB = weights (+ scales) + f32 partials written and read, from shapes.  A difference counts only "
                    "beyond the min - max spread of both versions.\n\n"
                    "| group | rows | bf16 µs | bf16 TB/s | fp8 µs | fp8 TB/s | fp4 µs | fp4 MB | fp4 TB/s | fp4 / fp8 time | fp4 / bf16 time | "
                    "beyond the spread |\n|---|---|---|---|---|---|---|---|---|---|---|---|\n")
            for r in res["gemv"]:
                b, q, h = r["bf16"], r["fp8"], r["fp4"]
                verdict = "fp4 faster than fp8" if r["fp4_beats_fp8_beyond_spread"] else \
                    "**fp4 slower than fp8**" if r["fp8_beats_fp4_beyond_spread"] else "no difference from fp8"
                f.write(f"| {r['group'].replace('|', ', ')} | {r['rows']} | {b['us']} ({b['us_min']} - {b['us_max']}) | {b['tb_per_s']} | "
                        f"{q['us']} ({q['us_min']} - {q['us_max']}) | {q['tb_per_s']} | {h['us']} ({h['us_min']} - {h['us_max']}) | "
                        f"{h['mbytes']} | {h['tb_per_s']} | {r['fp4_over_fp8_time']} | {r['fp4_over_bf16_time']} | {verdict} |\n")
            f.write("\nThe byte ratio allows 0.515 of the fp8 time and 0.266 of the bf16 time.\n\n")
        for key in [k for k in res if k.startswith("generate")]:
            g = res[key]
            f.write(f"## {g['workload']}\n\n| weights | ms / token (runs) | best |\n|---|---|---|\n")
            for k, v in g.items():
                if k.startswith("weights_"):
                    f.write(f"| {k.split('_')[1]} | {' / '.join(str(x) for x in v['ms_per_token_runs'])} | {v['ms_per_token']} |\n")
            f.write(f"\nSame tokens as with bf16 weights: {g['same_tokens_as_bf16_weights']}\n\n")
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
        raise SystemExit("gpu_w4_probe needs an MI355X: a time measured elsewhere says nothing")
    want = set(a.only.split(","))
    res = {"device": torch.cuda.get_device_name(0)}
    with torch.no_grad():
        if "gemv" in want:
            res["gemv"] = []
            for name, K, Ns, kind in GROUPS:
                for rows in (1, 4):
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
