"""What the opt-in bf16 convolution route of the VQGAN buys and costs, beside the f32 route of the same commit: one process
on one MI355X, the two precisions alternating within each of --reps repetitions after one warm-up each, every figure the
median with min-max.

  layers   the layer shapes of the table in profiles/r06_conv_persistent.md at batch --batch, ops.conv2d_nhwc against
           ops.conv2d_nhwc_bf16 (bias, and the residual where the layer has one); --calls calls back to back per timing
  model    VQGAN.encode and VQGAN.decode (default configuration, seeded random weights) of --frames frames of 256x256,
           U(-1, 1); decode runs on the f32 route's codes
  movement on those frames: how many codes of the bf16 route equal the f32 route's, and how far its decoded pixels lie
           from the f32 route's on the same (f32) codes, on a [-1, 1] scale

ms = host clock around work that ends in a device synchronise.  Writes the tables as markdown (--out), prints them as JSON.

python scripts/gpu_vqgan_bf16_probe.py [--frames 64] [--batch 32] [--reps 5] [--out profiles/r22_vqgan_bf16.md]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (name, H, W, Cin, Cout, options, residual): the table of profiles/r06_conv_persistent.md
LAYERS = [
    ("256², 128→128 + residual", 256, 256, 128, 128, {}, True),
    ("128²→256² upsample, 128→128", 128, 128, 128, 128, dict(up_shift=1), False),
    ("128², 128→128 + residual", 128, 128, 128, 128, {}, True),
    ("128², 256→128", 128, 128, 256, 128, {}, False),
    ("64²→128² upsample, 256→256", 64, 64, 256, 256, dict(up_shift=1), False),
    ("64², 256→256 + residual", 64, 64, 256, 256, {}, True),
    ("64², 128→256", 64, 64, 128, 256, {}, False),
    ("32², 256→256 + residual", 32, 32, 256, 256, {}, True),
    ("32², 512→512 + residual", 32, 32, 512, 512, {}, True),
    ("32²→64² upsample, 512→512", 32, 32, 512, 512, dict(up_shift=1), False),
    ("64², 512→256", 64, 64, 512, 256, {}, False),
    ("16², 768→768 + residual", 16, 16, 768, 768, {}, True),
    ("256², 256→128", 256, 256, 256, 128, {}, False),
    ("Downsample 256²→128², 128→128", 256, 256, 128, 128, dict(stride=2, pad=0, out_hw=(128, 128)), False),
]


def stats(v):
    v = sorted(v)
    return dict(median=v[len(v) // 2], min=v[0], max=v[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_vqgan_bf16.md"))
    a = ap.parse_args()
    if a.reps < 5:
        raise SystemExit("--reps: at least 5 alternated repetitions")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("needs the MI355X")
    from lwm_amd import ops
    from lwm_amd._lib import lib
    from lwm_amd.vqgan import VQGAN, VQGANConfig, random_params

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def alternate(legs):
        """{name: fn} -> {name: stats of ms}, one warm-up each, then the legs alternating within each repetition"""
        for fn in legs.values():
            timed(fn)
        per = {name: [] for name in legs}
        for _ in range(a.reps):
            for name, fn in legs.items():
                per[name].append(timed(fn)[0])
        return {name: stats(v) for name, v in per.items()}

    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *shape: torch.randn(*shape, generator=g, device="cuda")
    res = dict(device=torch.cuda.get_device_name(), lwm_version=int(lib().lwm_version()), frames=a.frames, batch=a.batch,
               reps=a.reps, calls=a.calls, layers=[], model={})
    for name, H, W, Cin, Cout, kw, has_res in LAYERS:
        x, w, b = rnd(a.batch, H, W, Cin), rnd(3, 3, Cin, Cout) / (9 * Cin) ** 0.5, rnd(Cout)
        pack = ops.conv_pack_bf16(w)
        y = ops.conv2d_nhwc(x, w, b, **kw)
        r = torch.randn_like(y) if has_res else None
        y2 = torch.empty_like(y)

        def many(fn):
            return lambda: [fn() for _ in range(a.calls)]
        ms = alternate({"f32": many(lambda: ops.conv2d_nhwc(x, w, b, r, out=y, **kw)),
                        "bf16": many(lambda: ops.conv2d_nhwc_bf16(x, pack, b, r, out=y2, **kw))})
        ms = {k: {s: v / a.calls for s, v in st.items()} for k, st in ms.items()}
        flop = 2.0 * y.numel() * 9 * Cin
        res["layers"].append(dict(layer=name, ms=ms, tflops={k: flop / (st["median"] * 1e-3) / 1e12 for k, st in ms.items()},
                                  max_abs_diff=float((y - y2).abs().max())))
        del x, w, b, pack, y, y2, r
        torch.cuda.empty_cache()

    cfg = VQGANConfig.get_default_config()
    params = random_params(cfg, 0)
    vq = {p: VQGAN(params=params, config=cfg, precision=p) for p in ("f32", "bf16")}
    frames = torch.rand(a.frames, 256, 256, 3, generator=g, device="cuda") * 2 - 1
    codes = {p: v.encode(frames)[1] for p, v in vq.items()}
    res["model"]["encode"] = alternate({p: (lambda v=v: v.encode(frames)) for p, v in vq.items()})
    res["model"]["decode"] = alternate({p: (lambda v=v: v.decode(codes["f32"])) for p, v in vq.items()})
    d = (vq["bf16"].decode(codes["f32"]) - vq["f32"].decode(codes["f32"])).abs()
    res["movement"] = dict(codes_equal=int((codes["f32"] == codes["bf16"]).sum()), codes=int(codes["f32"].numel()),
                           pixel_mean=float(d.mean()), pixel_max=float(d.max()))

    fmt = lambda s: f"{s['median']:.3f} ({s['min']:.3f}–{s['max']:.3f})"
    beyond = lambda m: ("faster" if m["bf16"]["max"] < m["f32"]["min"] else "slower" if m["bf16"]["min"] > m["f32"]["max"] else "within the spread")
    lines = ["# The VQGAN's bf16 convolution route beside its f32 route", "",
             f"`scripts/gpu_vqgan_bf16_probe.py --frames {a.frames} --batch {a.batch} --reps {a.reps}` on {res['device']}, `lwm_version()` "
             f"{res['lwm_version']}: one process, both precisions of the same commit, one warm-up each, then alternating within each of "
             f"{a.reps} repetitions. ms, host clock around work that ends in a device synchronise: median (min–max). Random operands.", "",
             f"## Layers (batch {a.batch}, {a.calls} calls back to back per timing, ms per call)", "",
             "`ops.conv2d_nhwc` (exact-f32 MFMA, the kernels of `vqgan_conv.h`) against `ops.conv2d_nhwc_bf16` (`vqgan_conv_bf16.h`, "
             "f32 activations in memory, rounded on the way into LDS). TF/s = 2·M·Cout·9·Cin over the median.", "",
             "| layer | f32, ms | bf16, ms | f32, TF/s | bf16, TF/s | f32 / bf16 | bf16 is |", "|---|---|---|---|---|---|---|"]
    for L in res["layers"]:
        m = L["ms"]
        lines.append(f"| {L['layer']} | {fmt(m['f32'])} | {fmt(m['bf16'])} | {L['tflops']['f32']:.0f} | {L['tflops']['bf16']:.0f} | "
                     f"{m['f32']['median'] / m['bf16']['median']:.2f}x | {beyond(m)} |")
    lines += ["", f"## `VQGAN.encode` and `VQGAN.decode`, {a.frames} frames of 256x256 (default configuration, seeded random weights)", "",
              "| call | f32, ms | bf16, ms | f32, µs per frame | bf16, µs per frame | f32 / bf16 | bf16 is |", "|---|---|---|---|---|---|---|"]
    for call, m in res["model"].items():
        lines.append(f"| {call} | {fmt(m['f32'])} | {fmt(m['bf16'])} | {m['f32']['median'] / a.frames * 1e3:.0f} | "
                     f"{m['bf16']['median'] / a.frames * 1e3:.0f} | {m['f32']['median'] / m['bf16']['median']:.2f}x | {beyond(m)} |")
    mv = res["movement"]
    lines += ["", "GroupNorm + SiLU, the quantiser and the two 3-channel convolutions are the same f32 kernels in both columns.", "",
              "## Movement against the f32 route on those frames (random weights)", "",
              f"- codes: {mv['codes_equal']} of {mv['codes']} equal ({100.0 * mv['codes_equal'] / mv['codes']:.2f} %)",
              f"- decoded pixels on the f32 route's codes, [-1, 1] scale: mean |Δ| {mv['pixel_mean']:.4f}, max |Δ| {mv['pixel_max']:.4f}", "",
              "Random weights say little about a trained codebook: quality on a real checkpoint has not been measured.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
