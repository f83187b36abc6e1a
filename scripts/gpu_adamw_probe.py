"""Time of the optimiser phase of a training step on the parameter shapes of a 4-layer LWM-7B slice (1.07e9 parameters):
clip_grad_norm_ + torch.optim.AdamW(foreach=True) -- what lwm_amd.cli.train does without --lwm_fused_optimizer -- against
lwm_amd.optim.FusedAdamW, each for bf16 and f32 parameters.  One process, device events, the four legs in alternating
windows after a warm-up (the clock wanders under load: a leg's figure is the median of its windows, the spread is printed).

Bytes: what each leg's ALGORITHM must move per parameter, not what its kernels do move --
  fused, bf16 parameters   g 2 (norm) + g 2, p m v 12 read + p m v 12, copy 2 written            = 30
  fused, f32 parameters    g 4 (norm) + g 4, p m v 12 read + p m v 12 written                    = 32
  torch, f32               g 4 (norm) + g 4 + 4 (scaled in place) + g p m v 16 read + p m v 12   = 40
  torch, bf16              the same in 2-byte elements                                           = 20
so a leg's TB/s is its useful traffic over its time; the fused legs' is also their achieved bandwidth.

    python scripts/gpu_adamw_probe.py [--layers 4] [--windows 5] [--steps 5] [--out profiles/r11_fused_adamw.md]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STREAM_TBS = 6.3        # the streaming figure of the MI355X's HBM (MI355X_MICROARCH.md)


def shapes(layers, hidden=4096, inter=11008, vocab=32000):
    out = [(vocab, hidden)]
    for _ in range(layers):
        out += [(hidden, hidden)] * 4 + [(hidden, inter), (inter, hidden), (hidden, inter), (hidden,), (hidden,)]
    return out + [(hidden,), (hidden, vocab)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gpu_adamw_probe needs an MI355X: a time measured elsewhere says nothing")
    from lwm_amd.optim import FusedAdamW
    dev = torch.device("cuda", 0)
    hp = dict(lr=8e-5, betas=(0.9, 0.95), eps=1e-8, weight_decay=1e-4)
    gen = torch.Generator(device=dev).manual_seed(0)
    shp = shapes(a.layers)
    n_params = sum(torch.Size(s).numel() for s in shp)

    def params(dtype):
        ps = [torch.nn.Parameter((torch.randn(s, device=dev, generator=gen) * 0.02).to(dtype)) for s in shp]
        for p in ps:
            p.grad = (torch.randn(p.shape, device=dev, generator=gen) * 1e-3).to(dtype)
        return ps

    legs = {}
    for name, dtype, fused, bytes_per in (("torch_bf16", torch.bfloat16, False, 20), ("torch_f32", torch.float32, False, 40),
                                          ("fused_bf16_master", torch.bfloat16, True, 30), ("fused_f32", torch.float32, True, 32)):
        ps = params(dtype)
        if fused:
            opt = FusedAdamW(ps, max_grad_norm=1.0, **hp)
            step = opt.step
        else:
            opt = torch.optim.AdamW(ps, foreach=True, **hp)

            def step(ps=ps, opt=opt):
                torch.nn.utils.clip_grad_norm_(ps, 1.0)
                opt.step()
        legs[name] = dict(step=step, keep=(ps, opt), bytes=bytes_per * n_params, ms=[])
    for leg in legs.values():           # warm-up: state allocation, code objects, the library's algorithm choices
        for _ in range(3):
            leg["step"]()
    torch.cuda.synchronize()
    for _ in range(a.windows):
        for leg in legs.values():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                leg["step"]()
            e1.record()
            torch.cuda.synchronize()
            leg["ms"].append(e0.elapsed_time(e1) / a.steps)
    rows = []
    for name, leg in legs.items():
        ms = statistics.median(leg["ms"])
        rows.append(dict(leg=name, ms_per_step=round(ms, 3), ms_min=round(min(leg["ms"]), 3), ms_max=round(max(leg["ms"]), 3),
                         gbytes=round(leg["bytes"] / 1e9, 2), tb_per_s=round(leg["bytes"] / ms / 1e9, 3),
                         share_of_stream=round(leg["bytes"] / ms / 1e9 / STREAM_TBS, 3)))
    res = dict(parameters=n_params, layers=a.layers, windows=a.windows, steps_per_window=a.steps, legs=rows)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(f"# Optimiser phase: clip + AdamW, {n_params / 1e9:.3f}e9 parameters ({a.layers}-layer LWM-7B slice)\n\n"
                    f"scripts/gpu_adamw_probe.py: device events, {a.windows} alternating windows of {a.steps} steps per leg after a warm-up; "
                    f"median (min - max) of the windows.  GB = the traffic the leg's algorithm needs (the script's docstring), TB/s = GB over "
                    f"the time, share = TB/s over the {STREAM_TBS} TB/s streaming figure of the HBM.\n\n"
                    "| leg | ms / step | GB | TB/s | share of streaming |\n|---|---|---|---|---|\n")
            for r in rows:
                f.write(f"| {r['leg']} | {r['ms_per_step']} ({r['ms_min']} - {r['ms_max']}) | {r['gbytes']} | {r['tb_per_s']} | {r['share_of_stream']} |\n")


if __name__ == "__main__":
    main()
