"""What the frame preprocessor costs beside the stage it feeds: one process on one MI355X, --frames frames of 1280x720 and of
1920x1080 -> 256x256, the legs alternating within each of --reps repetitions after one warm-up each, reported as median and
min-max.

  hip_device  lwm_amd.frames.process_frames on frames already in device memory
  hip_host    the same from pageable host memory (numpy), the upload included
  pil_host    the host route: lwm_amd.cli.vision_chat._process_frame (Pillow, Image.fromarray included), one frame at a time
  encode      VQGAN.encode (default configuration, seeded random weights) of the preprocessed frames: the stage behind

ms = host clock around work that ends in a device synchronise.  The device result is compared with the host route's, bit
for bit, on the frames that are timed.  Writes the table as markdown (--out) and prints it as JSON.

python scripts/gpu_frames_probe.py [--frames 64] [--reps 5] [--out profiles/r20_frames.md]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(v):
    v = sorted(v)
    return dict(median=v[len(v) // 2], min=v[0], max=v[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_frames.md"))
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("needs the MI355X")
    import PIL
    from PIL import Image
    from lwm_amd._lib import lib
    from lwm_amd.cli import _common as C
    from lwm_amd.cli.vision_chat import _process_frame
    from lwm_amd.frames import process_frames
    vq = C.load_vqgan("", 0)
    T = a.frames

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    res = dict(device=torch.cuda.get_device_name(), lwm_version=int(lib().lwm_version()), pillow=PIL.__version__, frames=T,
               reps=a.reps, shapes={})
    for h, w in ((720, 1280), (1080, 1920)):
        host = np.random.default_rng(h).integers(0, 256, (T, h, w, 3), dtype=np.uint8)
        dev = torch.from_numpy(host).cuda()
        pixels = process_frames(dev, 256)
        legs = {
            "hip_device": lambda: process_frames(dev, 256),
            "hip_host": lambda: process_frames(host, 256),
            "pil_host": lambda: np.stack([_process_frame(Image.fromarray(f), 256) for f in host]),
            "encode": lambda: vq.encode(pixels),
        }
        outs = {name: timed(fn)[1] for name, fn in legs.items()}             # warm-up
        equal = bool(np.array_equal(outs["hip_device"].cpu().numpy(), outs["pil_host"]) and
                     np.array_equal(outs["hip_host"].cpu().numpy(), outs["pil_host"]))
        del outs
        per = {name: [] for name in legs}
        for _ in range(a.reps):
            for name, fn in legs.items():
                per[name].append(timed(fn)[0])
        res["shapes"][f"{w}x{h}"] = dict(ms={name: stats(v) for name, v in per.items()}, hip_equals_pil_bit_for_bit=equal)

    fmt = lambda s: f"{s['median']:.2f} ({s['min']:.2f}–{s['max']:.2f})"
    lines = [f"# Frame preprocessor on the device: {T} frames -> 256x256, beside the host route and the tokeniser", "",
             f"`scripts/gpu_frames_probe.py --frames {T} --reps {a.reps}` on {res['device']}, `lwm_version()` {res['lwm_version']}, Pillow "
             f"{res['pillow']}: one process, one warm-up per leg, then the legs alternating within each of {a.reps} repetitions. ms for "
             f"all {T} frames, host clock around work that ends in a device synchronise: median (min–max).", "",
             "- **hip, device**: `lwm_amd.frames.process_frames` on frames already in device memory.",
             "- **hip, host**: the same from pageable host memory, the upload included.",
             "- **Pillow, host**: `_process_frame` per frame on one host thread (`Image.fromarray` included), the `LWM_FRAMES=pil` route.",
             "- **encode**: `VQGAN.encode` (default configuration, seeded random weights) of the same frames, preprocessed.", "",
             "| frames | hip, device | hip, host | Pillow, host | encode | hip, device, µs per frame | encode, µs per frame | Pillow / hip, host | bit for bit |",
             "|---|---|---|---|---|---|---|---|---|"]
    for shape, r in res["shapes"].items():
        m = r["ms"]
        lines.append(f"| {shape} | {fmt(m['hip_device'])} | {fmt(m['hip_host'])} | {fmt(m['pil_host'])} | {fmt(m['encode'])} | "
                     f"{m['hip_device']['median'] / T * 1e3:.1f} | {m['encode']['median'] / T * 1e3:.1f} | "
                     f"{m['pil_host']['median'] / m['hip_host']['median']:.1f}x | {'equal' if r['hip_equals_pil_bit_for_bit'] else 'DIFFERENT'} |")
    lines += ["", "bit for bit: the device result of the timed frames against the host route's, `np.array_equal`.", ""]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
