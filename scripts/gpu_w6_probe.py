"""Time of the 6-bit (MXFP6) decode weights against the 8-bit and 4-bit packs and bf16 weight streaming, one process, the
versions alternated.  The protocol and the machinery are scripts/gpu_w8_probe.py's and scripts/gpu_w4_probe.py's.

  proj      per LWM-7B projection group (wq|wk|wv and w1|w3 with the RMSNorm on load, wo and w2 with the residual and ss_out,
            lm_head with f32 logits): 1 and 4 rows through lwm_gemv_fused_w6 / _w8 / _w4 / _bf16, and 8, 16 and 32 rows through
            lwm_gemm_rows_fused_w6 / _w8 / _bf16 (there is no 4-bit rows entry).  Every group is a RING of copies whose 4-bit
            packs alone exceed the 256 MiB of last-level cache, walked once per pass inside a captured hipGraph, device events
            around whole passes, the versions in alternating windows; median (min - max) of the windows.  Bytes from shapes:
            weights (+ scales) read once, f32 partials written and read once.  The kernels are rounded to MXFP4 first, then
            to MXFP6 and to e4m3: with one magnitude per kernel the 4-bit values are e2m3 and e4m3 values, so all versions
            stream the same numbers.
  generate  LLaMAForCausalLM.generate(graph=True) milliseconds per token on the 4-layer LWM-7B slice the README quotes, fp6 /
            fp8 / fp4 / bf16 weights alternated: a short prompt, and a 131072-row cache as bf16 and as fp6.
  quality   how far the logits of that slice move when its RANDOM weights are rounded to e4m3, MXFP6 and MXFP4, and the share
            of greedy tokens kept over 64 steps -- a property of the formats on random weights, recorded, not asserted.

    python scripts/gpu_w6_probe.py [--only proj,generate_short,generate_long,generate_long_kv6,quality] [--json piece.json]
    python scripts/gpu_w6_probe.py --merge a.json,b.json --out profiles/r26_w6_decode.md      (no device needed)
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

FORMATS = ("fp6", "fp8", "fp4", "bf16")
LEGS = ("proj", "generate_short", "generate_long", "generate_long_kv6", "quality")
GEMV_ROWS, ROWS_ROWS = (1, 4), (8, 16, 32)


def _spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs))


def proj_group(name, K, Ns, kind, windows, target_ms):
    """one projection group at every row count, over one ring of copies"""
    import torch
    from gpu_w8_probe import LLC_BYTES
    from lwm_amd import llama_ops as LO, w4, w6, w8
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    wbytes = {"bf16": sum(2 * K * N for N in Ns), "fp8": sum(K * N + ((K + 127) // 128) * N * 4 for N in Ns),
              "fp6": sum(3 * K * N // 4 + (K // 32) * N for N in Ns), "fp4": sum(K * N // 2 + (K // 32) * N for N in Ns)}
    copies = max(2, -(-2 * LLC_BYTES // wbytes["fp4"]))
    ring, packs = [], {f: [] for f in ("fp8", "fp6", "fp4")}
    for _ in range(copies):
        ws = [(torch.randn(K, N, device=dev, generator=gen) * 0.02).to(torch.bfloat16) for N in Ns]
        packs["fp4"].append([w4.quantise_weight(w) for w in ws])      # (rounds ws in place; MXFP4 values of one magnitude
        packs["fp6"].append([w6.quantise_weight(w) for w in ws])      # are e2m3 values ...
        packs["fp8"].append([w8.quantise_weight(w) for w in ws])      # ... and e4m3 values)
        ring.append(ws)
    same_numbers = all(torch.equal(w6.w6_dequant(p.q, p.scale, p.shape), w) and torch.equal(w4.w4_dequant(q.q, q.scale, q.shape), w)
                       for p, q, w in zip(packs["fp6"][0], packs["fp4"][0], ring[0]))
    out = []
    for rows in GEMV_ROWS + ROWS_ROWS:
        gemv = rows <= 4
        fmts = FORMATS if gemv else ("fp6", "fp8", "bf16")
        fn = {"fp6": w6.gemv_fused_w6 if gemv else w6.gemm_rows_fused_w6, "fp8": w8.gemv_fused_w8 if gemv else w8.gemm_rows_fused_w8,
              "fp4": w4.gemv_fused_w4, "bf16": LO.gemv_fused if gemv else LO.gemm_rows_fused}
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
            for mats in (ring if fmt == "bf16" else packs[fmt]):
                fn[fmt](x, mats, **kw)

        graphs = {}
        for fmt in fmts:
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
        ms = {fmt: [] for fmt in fmts}
        for g in graphs.values():
            g.replay()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        graphs["bf16"].replay()
        torch.cuda.synchronize()
        passes = max(1, int(target_ms / 1e3 / max(time.perf_counter() - t0, 1e-6)))
        for _ in range(windows):
            for fmt in fmts:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(passes):
                    graphs[fmt].replay()
                e1.record()
                torch.cuda.synchronize()
                ms[fmt].append(e0.elapsed_time(e1) / (passes * copies))
        part = sum(2 * ((K + 127) // 128) * rows * N * 4 for N in Ns)
        r = dict(group=name, rows=rows, entry="gemv" if gemv else "rows", K=K, N=list(Ns), copies=copies, passes_per_window=passes,
                 same_numbers=bool(same_numbers))
        for fmt in fmts:
            s = _spread(ms[fmt])
            by = wbytes[fmt] + part
            r[fmt] = dict(us=round(s["median"] * 1e3, 2), us_min=round(s["min"] * 1e3, 2), us_max=round(s["max"] * 1e3, 2),
                          mbytes=round(by / 1e6, 2), tb_per_s=round(by / s["median"] / 1e9, 3))
        r["fp6_over_fp8_time"] = round(r["fp6"]["us"] / r["fp8"]["us"], 3)
        r["fp6_over_bf16_time"] = round(r["fp6"]["us"] / r["bf16"]["us"], 3)
        # beyond the probe's own spread: the whole min - max range of one version lies on one side of the other's
        r["fp6_beats_fp8_beyond_spread"] = bool(r["fp6"]["us_max"] < r["fp8"]["us_min"])
        r["fp8_beats_fp6_beyond_spread"] = bool(r["fp8"]["us_max"] < r["fp6"]["us_min"])
        out.append(r)
        print(json.dumps(r), flush=True)
        del graphs
    del ring, packs
    torch.cuda.empty_cache()
    return out


def generate_ms(prompt, max_length, new, kv=None, short=8, reps=3):
    import torch
    from gpu_w8_probe import _slice
    cfg, model = _slice(max_length)
    model.quantize_decode_weights("fp4").quantize_decode_weights("fp6").quantize_decode_weights("fp8")   # the rounded model, for every leg
    ids = torch.randint(0, cfg.vocab_size, (1, prompt), device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))

    def run(n, weights):
        model.quantize_decode_weights(weights)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        toks = model.generate(ids, max_new_tokens=n, max_length=max_length, graph=True, kv_dtype=kv)
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
    out = {"workload": f"generate(graph=True), 4-layer slice of LWM-7B, prompt {prompt}, cache max_length {max_length}, B=1, "
                       f"{kv or 'bf16'} cache, random weights rounded to MXFP4; (run of {new} tokens - run of {short}) / {new - short}: "
                       f"median (min - max) of {reps} alternated runs"}
    for w in FORMATS:
        per = [(a - min(ts[w])) / (new - short) * 1e3 for a in tl[w]]
        s = _spread(per)
        out[f"weights_{w}"] = dict(ms_per_token=round(s["median"], 3), ms_min=round(s["min"], 3), ms_max=round(s["max"], 3))
    a, b = out["weights_fp6"], out["weights_fp8"]
    out["fp6_over_fp8_time"] = round(a["ms_per_token"] / b["ms_per_token"], 3)
    out["fp6_beats_fp8_beyond_spread"] = bool(a["ms_max"] < b["ms_min"])
    out["fp8_beats_fp6_beyond_spread"] = bool(b["ms_max"] < a["ms_min"])
    out["same_tokens_as_bf16_weights"] = {w: bool(torch.equal(toks["bf16"], toks[w])) for w in ("fp8", "fp6", "fp4")}
    del model
    torch.cuda.empty_cache()
    return out


def quality(steps=64, prompt=512):
    import torch
    from gpu_w8_probe import _slice
    out = dict(workload=f"4-layer slice of LWM-7B, RANDOM weights, prompt {prompt}, {steps} greedy steps, unrounded against rounded")
    base = None
    for fmt in ("bf16", "fp8", "fp6", "fp4"):
        cfg, model = _slice(4096)                               # (the same seed: the same unrounded weights every time)
        ids = torch.randint(0, cfg.vocab_size, (1, prompt), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
        model.quantize_decode_weights(fmt)
        t, l = model.generate(ids, max_new_tokens=steps, return_logits=True)
        del model
        torch.cuda.empty_cache()
        if fmt == "bf16":
            base = (t, l)
            continue
        new0, new1 = base[0][0, prompt:], t[0, prompt:]
        same = (new0 == new1)
        first = int((~same).nonzero()[0]) if not bool(same.all()) else steps
        n = max(first, 1)                                       # the steps that saw the same context (step 0 always does)
        d = (l[0, :n] - base[1][0, :n]).abs()
        out[fmt] = dict(greedy_tokens_kept=round(float(same.float().mean()), 4), steps_before_first_difference=first,
                        max_abs_dlogit=float(d.max()), mean_abs_dlogit=float(d.mean()), max_abs_logit=float(base[1][0, :n].abs().max()))
    return out


def _cell(d):
    return f"{d['us']} ({d['us_min']} - {d['us_max']})"


def _verdict(r):
    return "fp6 faster than fp8" if r["fp6_beats_fp8_beyond_spread"] else \
        "**fp6 slower than fp8**" if r["fp8_beats_fp6_beyond_spread"] else "no difference from fp8"


def write_md(path, res):
    with open(path, "w") as f:
        f.write("# 6-bit (MXFP6) decode weights against the 8-bit and 4-bit packs and bf16 weight streaming\n\nscripts/gpu_w6_probe.py on " +
                res.get("device", "?") + ": one process per section, the versions alternated inside it.  A difference counts only "
                "beyond the min - max spread of both versions.\n\n")
        if "proj" in res:
            f.write("## Per launch pair at the LWM-7B projection groups\n\nEach group is a ring of copies (the 4-bit packs alone exceed "
                    "256 MiB) walked inside a captured graph; µs per launch pair, median (min - max) of the alternating windows; MB = "
                    "weights (+ scales) + f32 partials written and read, from shapes.  1 and 4 rows: lwm_gemv_fused_*; 8, 16 and 32 "
                    "rows: lwm_gemm_rows_fused_* (no 4-bit rows entry exists).\n\n"
                    "| group | rows | bf16 µs | fp8 µs | fp4 µs | fp6 µs | fp6 MB | fp6 TB/s | fp6 / fp8 time | fp6 / bf16 time | "
                    "beyond the spread |\n|---|---|---|---|---|---|---|---|---|---|---|\n")
            for r in res["proj"]:
                h = r["fp6"]
                f.write(f"| {r['group'].replace('|', ', ')} | {r['rows']} | {_cell(r['bf16'])} | {_cell(r['fp8'])} | "
                        f"{_cell(r['fp4']) if 'fp4' in r else '-'} | {_cell(h)} | {h['mbytes']} | {h['tb_per_s']} | "
                        f"{r['fp6_over_fp8_time']} | {r['fp6_over_bf16_time']} | {_verdict(r)} |\n")
            f.write("\nThe weight bytes allow 0.757 of the fp8 time and 0.391 of the bf16 time.\n\n")
        for key in [k for k in res if k.startswith("generate")]:
            g = res[key]
            f.write(f"## {g['workload']}\n\n| weights | ms / token |\n|---|---|\n")
            for k, v in g.items():
                if k.startswith("weights_"):
                    f.write(f"| {k.split('_')[1]} | {v['ms_per_token']} ({v['ms_min']} - {v['ms_max']}) |\n")
            f.write(f"\nfp6 / fp8 time {g['fp6_over_fp8_time']}: {_verdict(g)}.  Same tokens as with bf16 weights: "
                    f"{g['same_tokens_as_bf16_weights']}\n\n")
        if "quality" in res:
            q = res["quality"]
            f.write(f"## Quality on RANDOM weights (recorded, not asserted)\n\n{q['workload']}.\n\n| weights | greedy tokens kept | steps "
                    "before the first difference | max \\|dlogit\\| | mean \\|dlogit\\| | max \\|logit\\| |\n|---|---|---|---|---|---|\n")
            for fmt in ("fp8", "fp6", "fp4"):
                v = q[fmt]
                f.write(f"| {fmt} | {v['greedy_tokens_kept']} | {v['steps_before_first_difference']} | {v['max_abs_dlogit']:.4g} | "
                        f"{v['mean_abs_dlogit']:.4g} | {v['max_abs_logit']:.4g} |\n")
            f.write("\n|dlogit| over the steps that saw the same context (at least the first).\n")
        for k in LEGS:
            if k not in res:
                f.write(f"\n**{k}: not measured** -- {res.get('not_run', {}).get(k, 'the leg was not run')}\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=",".join(LEGS))
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--target_ms", type=float, default=60.0, help="device time per window")
    ap.add_argument("--out", default="")
    ap.add_argument("--json", default="")
    ap.add_argument("--merge", default="", help="comma-separated JSON pieces of earlier runs: write --out from them, run nothing")
    a = ap.parse_args()
    if a.merge:
        res = {}
        for p in a.merge.split(","):
            with open(p) as f:
                res.update(json.load(f))
        write_md(a.out, res)
        return
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("gpu_w6_probe needs an MI355X: a time measured elsewhere says nothing")
    from gpu_w8_probe import GROUPS
    want = set(a.only.split(","))
    res = {"device": torch.cuda.get_device_name(0)}
    with torch.no_grad():
        if "proj" in want:
            res["proj"] = []
            for name, K, Ns, kind in GROUPS:
                res["proj"] += proj_group(name, K, Ns, kind, a.windows, a.target_ms)
        for leg, args in (("generate_short", (2048, 32768, 136)), ("generate_long", (131072 - 1024, 131072, 72)),
                          ("generate_long_kv6", (131072 - 1024, 131072, 72, "fp6"))):
            if leg in want:
                res[leg] = generate_ms(*args)
                print(json.dumps(res[leg]), flush=True)
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
