"""Time of the 5..32-row decode route (LWM_DECODE_ROWS / model.decode_rows: lwm_gemm_rows_fused_bf16 / _w8, csrc/gemm_rows.h)
against what runs without it, one process, the versions alternated.

  pairs     per LWM-7B projection group (wq|wk|wv and w1|w3 with the RMSNorm on load, wo and w2 with the residual and
            ss_out, lm_head with f32 logits) and for 8, 16 and 32 rows: `library` = llama_ops.dense_multi with the option
            off -- `x @ k` per kernel through the library GEMM, the head as x.float() @ the kept f32 copy of the kernel, and
            NOT the norm / residual launches around it --, `bf16` = lwm_gemm_rows_fused_bf16, `fp8` = lwm_gemm_rows_fused_w8,
            both with their fusions.  Every group is a RING of copies whose 8-bit packs alone exceed the 256 MiB of
            last-level cache, walked once per pass inside a captured hipGraph, device events around whole passes, the
            versions in alternating windows; median (min - max) of the windows.
  generate  LLaMAForCausalLM.generate(graph=True) milliseconds per token on the 4-layer LWM-7B slice at 8 and 32 rows,
            decode_rows off against on, short prompt and (8 rows; 32 rows of a 131072-row bf16 cache do not fit one device:
            --long32 runs them over the 8-bit cache with a chunked prefill) a 131072-row cache, two runs each.

    python scripts/gpu_decode_rows_probe.py [--only pairs,generate] [--out profiles/r13_decode_rows.md]
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
LEGS = ("library", "bf16", "fp8")


def pair_group(name, K, Ns, kind, rows, windows, target_ms):
    from lwm_amd import llama_ops as LO, w8
    assert LO.decode_rows_limit() is None, "unset LWM_DECODE_ROWS: the library leg is the route with the option off"
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    pack_bytes = sum(K * N + ((K + 127) // 128) * N * 4 for N in Ns)
    copies = max(2, -(-2 * LLC_BYTES // pack_bytes))
    ring, packs = [], []
    for _ in range(copies):
        ws = [(torch.randn(K, N, device=dev, generator=gen) * 0.02).to(torch.bfloat16) for N in Ns]
        packs.append([w8.quantise_weight(w) for w in ws])       # (rounds ws in place: every leg streams the same numbers)
        ring.append(ws)
    x = torch.randn(rows, K, device=dev, generator=gen).to(torch.bfloat16)
    out_dtype = torch.float32 if kind == "f32" else None
    if kind == "norm":
        ss = torch.zeros(rows, 32, device=dev)
        ss[:, 0] = x.float().pow(2).sum(-1)
        kw = dict(norm=(ss, torch.ones(K, device=dev, dtype=torch.bfloat16), 1e-6))
    elif kind == "res":
        kw = dict(residual=torch.randn(rows, Ns[0], device=dev, generator=gen).to(torch.bfloat16), want_ss=True)
    else:
        kw = dict(out_dtype=torch.float32)

    def one_pass(leg):
        for ws, ps in zip(ring, packs):
            if leg == "library":
                LO.dense_multi(x, ws, out_dtype)
            elif leg == "bf16":
                LO.gemm_rows_fused(x, ws, **kw)
            else:
                w8.gemm_rows_fused_w8(x, ps, **kw)

    graphs = {}
    for leg in LEGS:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            one_pass(leg)                                       # warm: code objects, workspaces, the head's f32 copies
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            one_pass(leg)
        graphs[leg] = g
    ms = {leg: [] for leg in LEGS}
    for g in graphs.values():
        g.replay()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    graphs["bf16"].replay()
    torch.cuda.synchronize()
    passes = max(1, int(target_ms / 1e3 / max(time.perf_counter() - t0, 1e-6)))
    for _ in range(windows):
        for leg in LEGS:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(passes):
                graphs[leg].replay()
            e1.record()
            torch.cuda.synchronize()
            ms[leg].append(e0.elapsed_time(e1) / (passes * copies))
    KS = (K + 127) // 128
    part = sum(2 * KS * rows * N * 4 for N in Ns)
    by = dict(library=sum((4 if kind == "f32" else 2) * K * N for N in Ns), bf16=sum(2 * K * N for N in Ns) + part, fp8=pack_bytes + part)
    out = dict(group=name, rows=rows, K=K, N=list(Ns), copies=copies, passes_per_window=passes)
    for leg in LEGS:
        m = ms[leg]
        out[leg] = dict(us=round(statistics.median(m) * 1e3, 2), us_min=round(min(m) * 1e3, 2), us_max=round(max(m) * 1e3, 2),
                        mbytes=round(by[leg] / 1e6, 2), tb_per_s=round(by[leg] / statistics.median(m) / 1e9, 3))
    out["bf16_over_library_time"] = round(out["bf16"]["us"] / out["library"]["us"], 3)
    out["fp8_over_library_time"] = round(out["fp8"]["us"] / out["library"]["us"], 3)
    del graphs, ring, packs
    torch.cuda.empty_cache()
    return out


def _slice(max_length, layers=4):
    from lwm_amd.llama import LLaMAConfig, LLaMAForCausalLM
    cfg = LLaMAConfig.load_config("7b", num_hidden_layers=layers, max_sequence_length=max_length, theta=1e7)
    torch.manual_seed(0)
    with torch.device("cuda"):
        return cfg, LLaMAForCausalLM(cfg)


def generate_ms(rows, prompt, max_length, new, short=8, reps=2, **gen_kw):
    cfg, model = _slice(max_length)
    ids = torch.randint(0, cfg.vocab_size, (rows, prompt), device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))

    def run(n, option):
        model.decode_rows = option
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        toks = model.generate(ids, max_new_tokens=n, max_length=max_length, graph=True, **gen_kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, toks

    legs = (None, 32)
    for leg in legs:
        run(3, leg)                                             # warm
    ts, tl = {l: [] for l in legs}, {l: [] for l in legs}
    for _ in range(reps):                                       # alternated
        for leg in legs:
            ts[leg].append(run(short, leg)[0])
        for leg in legs:
            tl[leg].append(run(new, leg)[0])
    out = {"workload": f"generate(graph=True{''.join(f', {k}={v!r}' for k, v in gen_kw.items())}), 4-layer slice of LWM-7B, {rows} rows, prompt "
                       f"{prompt}, cache max_length {max_length}, random weights; (run of {new} tokens - run of {short}) / {new - short}, "
                       f"per run and best of {reps}"}
    for leg in legs:
        out["decode_rows_" + ("off" if leg is None else "on")] = dict(
            ms_per_token_runs=[round((a - min(ts[leg])) / (new - short) * 1e3, 3) for a in tl[leg]],
            ms_per_token=round((min(tl[leg]) - min(ts[leg])) / (new - short) * 1e3, 3))
    out["on_over_off_time"] = round(out["decode_rows_on"]["ms_per_token"] / out["decode_rows_off"]["ms_per_token"], 3)
    del model
    torch.cuda.empty_cache()
    return out


def write_md(path, res):
    with open(path, "w") as f:
        f.write("# Decode at 5..32 rows: lwm_gemm_rows_fused_* against the library route\n\nscripts/gpu_decode_rows_probe.py on " +
                res["device"] + ": one process, the versions alternated.\n\n")
        if "pairs" in res:
            f.write("## Per LWM-7B projection group\n\n`library` = `x @ k` per kernel as the route without the option runs it (the head: "
                    "x.float() @ the kept f32 copy; the norm / residual launches around the GEMM are NOT in this leg); `bf16` / `fp8` = one "
                    "launch pair of lwm_gemm_rows_fused_bf16 / _w8 with its fusions.  Each group is a ring of copies (the 8-bit packs "
                    "alone exceed 256 MiB) walked inside a captured graph; µs per group, median (min - max) of the alternating windows; "
                    "MB from shapes (weights read once; the new entries also write and read their f32 partials).\n\n"
                    "| group | rows | library µs | bf16 µs | bf16 MB | bf16 TB/s | fp8 µs | fp8 MB | fp8 TB/s | bf16 / library | fp8 / library |\n"
                    "|---|---|---|---|---|---|---|---|---|---|---|\n")
            for r in res["pairs"]:
                l, b, q = r["library"], r["bf16"], r["fp8"]
                f.write(f"| {r['group'].replace('|', ', ')} | {r['rows']} | {l['us']} ({l['us_min']} - {l['us_max']}) | "
                        f"{b['us']} ({b['us_min']} - {b['us_max']}) | {b['mbytes']} | {b['tb_per_s']} | "
                        f"{q['us']} ({q['us_min']} - {q['us_max']}) | {q['mbytes']} | {q['tb_per_s']} | "
                        f"{r['bf16_over_library_time']} | {r['fp8_over_library_time']} |\n")
            f.write("\n")
        for key in [k for k in res if k.startswith("generate")]:
            g = res[key]
            f.write(f"## {g['workload']}\n\n| decode_rows | ms / token (runs) | best |\n|---|---|---|\n")
            for k in ("decode_rows_off", "decode_rows_on"):
                f.write(f"| {k[12:]} | {' / '.join(str(x) for x in g[k]['ms_per_token_runs'])} | {g[k]['ms_per_token']} |\n")
            f.write(f"\non / off time: {g['on_over_off_time']}\n\n")
        for k, v in res.get("not_run", {}).items():
            f.write(f"\n**Not run**: {k}: {v}\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="pairs,generate")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--target_ms", type=float, default=60.0, help="device time per window")
    ap.add_argument("--long32", action="store_true", help="32 rows of a 131072-row cache: over the 8-bit cache, prefill in blocks")
    ap.add_argument("--out", default="")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gpu_decode_rows_probe needs an MI355X: a time measured elsewhere says nothing")
    os.environ.pop("LWM_DECODE_ROWS", None)
    want = set(a.only.split(","))
    res = {"device": torch.cuda.get_device_name(0), "not_run": {}}

    def save():
        for path, as_json in ((a.json, True), (a.out, False)):
            if path:
                os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
                if as_json:
                    with open(path, "w") as f:
                        json.dump(res, f, indent=1)
                else:
                    write_md(path, res)

    with torch.no_grad():
        if "pairs" in want:
            res["pairs"] = []
            for name, K, Ns, kind in GROUPS:
                for rows in (8, 16, 32):
                    res["pairs"].append(pair_group(name, K, Ns, kind, rows, a.windows, a.target_ms))
                    print(json.dumps(res["pairs"][-1]), flush=True)
                    save()
        if "generate" in want:
            for rows in (8, 32):
                key = f"generate_rows{rows}_prompt512_cache4096"
                res[key] = generate_ms(rows, 512, 4096, 136)
                print(json.dumps(res[key]), flush=True)
                save()
            key = "generate_rows8_prompt130048_cache131072"
            res[key] = generate_ms(8, 131072 - 1024, 131072, 72, prefill_chunk=8192)
            print(json.dumps(res[key]), flush=True)
            save()
            if a.long32:
                key = "generate_rows32_prompt130048_cache131072_fp8cache"
                res[key] = generate_ms(32, 131072 - 1024, 131072, 72, kv_dtype="fp8", prefill_chunk=8192)
                print(json.dumps(res[key]), flush=True)
            else:
                res["not_run"]["generate, 32 rows, 131072-row cache"] = (
                    "a bf16 cache of 32 x 131072 rows x 4 layers is 275 GB; --long32 runs it over the 8-bit cache with prefill_chunk=8192")
            save()
    save()


if __name__ == "__main__":
    main()
