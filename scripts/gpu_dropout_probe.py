"""What the dropout of the training path (lwm_amd.llama_ops.dropout_add, csrc/dropout.h) costs on one MI355X.

  1. Kernel time: lwm_dropout_add_bf16 on (rows, C) = (32768, 4096) and (32768, 11008), ALTERNATED in one process with
     lwm_swiglu_fwd_bf16 on tensors of the same size -- the same three streams (two read, one written) and the same
     bytes, no random numbers: what the pass costs when only memory is in the way.  Device events around a batch of
     launches; median and min - max of the repetitions; bytes / s from the bytes the pass has to move (3 * rows * C * 2).
     The kernel counts as memory-bound when it takes no longer than the gate does (within the spread of the two).
  2. Step time: a 4-layer slice of LWM-7B, bf16, B = 1, S = 8192, forward + backward, resid_pdrop = embd_pdrop = 0
     against 0.1 in alternating steps of one process after a warm-up of each.

    python scripts/gpu_dropout_probe.py [--reps 7] [--out profiles/r27_dropout.md]
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

HBM_PEAK = 8.0e12          # bytes / s, the part's specification


def kernel_times(rows, Cc, reps, launches):
    from lwm_amd import dropout as D, llama_ops as O
    x, r = (torch.randn(1, rows, Cc, device="cuda").to(torch.bfloat16) for _ in range(2))
    y = torch.empty_like(x)
    thr16, inv = D.dropout_threshold(0.1)
    sc = (thr16, inv, 42, 7, 3, 0)
    legs = {"dropout_add": lambda: D._dropout_launch("add", x, r, y, sc),
            "dropout_add_no_res": lambda: D._dropout_launch("add", x, None, y, sc),
            "swiglu_fwd": lambda: O._capi.check(O.lib(), O.lib().lwm_swiglu_fwd_bf16(x.data_ptr(), r.data_ptr(), y.data_ptr(), x.numel(),
                                                                                   O._stream_ptr()), "lwm_swiglu_fwd_bf16")}
    us = {k: [] for k in legs}
    for fn in legs.values():                   # warm-up: code objects, clocks
        for _ in range(launches):
            fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        for name, fn in legs.items():          # the legs alternate within every repetition
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches):
                fn()
            e1.record()
            torch.cuda.synchronize()
            us[name].append(e0.elapsed_time(e1) * 1e3 / launches)
    out = {}
    for name, v in us.items():
        streams = 2 if name == "dropout_add_no_res" else 3
        med = statistics.median(v)
        out[name] = dict(us_median=med, us_min=min(v), us_max=max(v), bytes=streams * rows * Cc * 2,
                         tb_per_s=streams * rows * Cc * 2 / (med * 1e-6) / 1e12)
    return out


def step_times(reps, layers, S, timeout):
    from lwm_amd.llama import LLaMAConfig, LLaMAForCausalLM
    from lwm_amd.llama_ops import use_tuned_gemms, weights_changed
    cfg = LLaMAConfig.load_config("7b", num_hidden_layers=layers, max_sequence_length=S, theta=1e7)
    torch.manual_seed(0)
    with torch.device("cuda"):
        model = LLaMAForCausalLM(cfg).train()
    tuned = use_tuned_gemms()
    tok = torch.randint(0, cfg.vocab_size, (1, S + 1), device="cuda")
    count = [0]

    def step(rate):
        cfg.resid_pdrop = cfg.embd_pdrop = rate
        count[0] += 1
        model.set_dropout_rng(42, count[0])
        model.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        faulthandler.dump_traceback_later(timeout, exit=True)      # a step that does not return ends the process
        try:
            t0 = time.perf_counter()
            weights_changed()
            loss, _ = model.loss(tok[:, :-1], tok[:, 1:])
            loss.backward()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, float(loss.detach())
        finally:
            faulthandler.cancel_dump_traceback_later()

    runs = {0.0: [], 0.1: []}
    for rate in runs:
        step(rate)
    for _ in range(reps):
        for rate in runs:
            runs[rate].append(step(rate))
    out = dict(layers=layers, seq=S, reps=reps, tuned_gemm_solutions=tuned, scan_mlp_chunk=cfg.scan_mlp_chunk_size)
    for rate, rs in runs.items():
        ms = [r[0] for r in rs]
        out[f"rate_{rate}"] = dict(ms_median=statistics.median(ms), ms_min=min(ms), ms_max=max(ms), losses=[r[1] for r in rs])
    out["ratio"] = out["rate_0.1"]["ms_median"] / out["rate_0.0"]["ms_median"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--rows", type=int, default=32768)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--seq", type=int, default=8192)
    ap.add_argument("--step-reps", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=120)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gpu_dropout_probe needs an MI355X: a time measured elsewhere says nothing")
    from lwm_amd._lib import lib
    res = dict(device=torch.cuda.get_device_name(0), lwm_version=int(lib().lwm_version()), rows=a.rows, reps=a.reps, launches=a.launches,
               kernels={})
    for Cc in (4096, 11008):
        res["kernels"][str(Cc)] = kernel_times(a.rows, Cc, a.reps, a.launches)
        print(json.dumps({Cc: res["kernels"][str(Cc)]}), flush=True)
    res["step"] = None if a.no_step else step_times(a.step_reps, a.layers, a.seq, a.step_timeout)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(f"# Residual and embedding dropout: what the pass costs on one MI355X\n\n"
                    f"`scripts/gpu_dropout_probe.py --reps {a.reps} --launches {a.launches}` on {res['device']}, `lwm_version()` {res['lwm_version']}: one "
                    f"process, one warm-up of every leg, then the legs alternating within each of {a.reps} repetitions; device events around "
                    f"{a.launches} launches, µs per launch: median (min–max). bf16, rows = {a.rows}, p = 0.1 (thr16 = 6554). TB/s = the bytes the "
                    f"pass has to move (two or three streams of rows × C × 2) over the median; share = of the {HBM_PEAK / 1e12:.0f} TB/s specification.\n\n"
                    f"## 1. Kernel time: `lwm_dropout_add_bf16` beside `lwm_swiglu_fwd_bf16` (the same three streams, no random numbers)\n\n"
                    f"| C | leg | µs / launch | TB/s | share of HBM peak | over the gate |\n|---|---|---|---|---|---|\n")
            verdicts = []
            for Cc, legs in res["kernels"].items():
                gate = legs["swiglu_fwd"]
                for name, r in legs.items():
                    f.write(f"| {Cc} | `{name}` | {r['us_median']:.1f} ({r['us_min']:.1f}–{r['us_max']:.1f}) | {r['tb_per_s']:.2f} | "
                            f"{r['tb_per_s'] * 1e12 / HBM_PEAK:.2f} | {r['us_median'] / gate['us_median']:.3f} |\n")
                d = legs["dropout_add"]
                bound = d["us_median"] <= gate["us_max"] * 1.02
                verdicts.append(f"C = {Cc}: `dropout_add` takes {d['us_median'] / gate['us_median']:.3f} of the gate's time -- "
                                + ("**memory-bound** (no slower than a pass that only moves the same bytes)" if bound else
                                   "**NOT memory-bound**: the Philox rounds and the index arithmetic show above the memory time"))
            f.write("\n" + "\n\n".join(verdicts) + "\n\n")
            st = res["step"]
            if st is None:
                f.write("## 2. Step time\n\n**Not run** (`--no-step`).\n")
            else:
                f.write(f"## 2. Step time: {st['layers']}-layer slice of LWM-7B, bf16, B = 1, S = {st['seq']}, forward + backward\n\n"
                        f"Rates 0 and 0.1 (`resid_pdrop = embd_pdrop`) in alternating steps of one process after a warm-up of each, "
                        f"{st['reps']} repetitions; host clock around a synchronised step (kernels re-laid every step, as a training step "
                        f"does); `scan_mlp` chunks of {st['scan_mlp_chunk']} rows; tuned GEMM solutions: {st['tuned_gemm_solutions']}.\n\n"
                        f"| rates | ms / step |\n|---|---|\n")
                for rate in ("0.0", "0.1"):
                    r = st[f"rate_{rate}"]
                    f.write(f"| {rate} | {r['ms_median']:.1f} ({r['ms_min']:.1f}–{r['ms_max']:.1f}) |\n")
                f.write(f"\nRatio 0.1 / 0: **{st['ratio']:.3f}**. With dropout on, `wo` and `w2` lose their residual epilogue and one "
                        f"`dropout_add` pass per site takes its place ({2 * st['layers'] + 1} sites forward, as many backward).\n")
            f.write("\n```json\n" + json.dumps(res, indent=1) + "\n```\n")


if __name__ == "__main__":
    main()
