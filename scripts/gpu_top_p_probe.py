"""What nucleus (top-p) sampling costs, and that a launch with it off costs what it did: two measurements in one process,
the legs of each alternating within every repetition, reported as median and min-max.

  sampler   lwm_sample_tokens alone (ops.sample_tokens into preallocated outputs), V = 32000 and 8448, rows 1 / 2 / 4, T = 1:
            top-p off and on (p = 0.9), each without top-k and with k = 1000.  us per launch = the time between two device
            events around the replay of a hipGraph that holds --calls launches in a row (no host in the loop) / --calls.
  generate  VideoLLaMAForCausalLM.generate(do_sample=True, seed=, graph=True) on a --layers slice of LWM-7B (d_model 4096,
            32 heads, FFN 11008, vocab 32000), one row, prompt --prompt, T = 1, no top-k: top_p off and 0.9.  ms per token =
            (long run - short run) / extra tokens (bench.py generate_leg's method), host clock around runs that end in a
            device synchronise.

--other-lib PATH: a second build of liblwm_hip.so with the same ABI -- the parent commit's, say -- whose top-p-OFF legs are
timed in the same alternation ("other_off"): the comparison that says whether the new phase slowed the old path.

python scripts/gpu_top_p_probe.py [--other-lib build/parent/liblwm_hip.so] [--layers 4] [--reps 5] [--out out/top_p_probe.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(v):
    v = sorted(v)
    return dict(median=round(v[len(v) // 2], 4), min=round(v[0], 4), max=round(v[-1], 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other-lib", default="")
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--short", type=int, default=16)
    ap.add_argument("--long", type=int, default=272)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--skip-generate", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "out", "top_p_probe.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("needs the MI355X")
    from lwm_amd import _capi, _lib, ops
    libs = {"this": _lib.lib()}
    if a.other_lib:
        libs["other"] = _capi.bind(C.CDLL(os.path.abspath(a.other_lib)))
    versions = {k: int(v.lwm_version()) for k, v in libs.items()}

    def use(which):                 # every op of lwm_amd asks _lib.lib() for the library at each call
        _lib._lib = libs[which]

    # ---- the sampler launch alone
    g = torch.Generator(device="cuda").manual_seed(0)
    sampler = {}
    for V in (32000, 8448):
        for rows in (1, 2, 4):
            lg = torch.randn(rows, V, device="cuda", generator=g) * 3
            tok = torch.empty(rows, 1, dtype=torch.int64, device="cuda")
            legs = {"off_k0": ("this", 0, None), "off_k1000": ("this", 1000, None), "on_k0": ("this", 0, 0.9),
                    "on_k1000": ("this", 1000, 0.9)}
            if a.other_lib:
                legs.update({"other_off_k0": ("other", 0, None), "other_off_k1000": ("other", 1000, None)})

            def capture(which, k, p, lg=lg, tok=tok):
                use(which)
                kw = dict(temperature=1.0, top_k=k, top_p=p, seed=1, tokens_out=tok)
                ops.sample_tokens(lg, step=0, **kw)
                torch.cuda.synchronize()
                gr = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gr):
                    for i in range(a.calls):
                        ops.sample_tokens(lg, step=i, **kw)
                return gr

            def leg(gr):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                gr.replay()
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) * 1e3 / a.calls

            graphs = {name: capture(*spec) for name, spec in legs.items()}
            for gr in graphs.values():
                leg(gr)                                         # warm
            per = {name: [] for name in legs}
            for _ in range(a.reps):
                for name, gr in graphs.items():
                    per[name].append(leg(gr))
            sampler[f"V{V}_rows{rows}"] = {name: stats(v) for name, v in per.items()}
    use("this")
    res = dict(device=torch.cuda.get_device_name(), lwm_version=versions, calls=a.calls, reps=a.reps, sampler_us_per_launch=sampler)

    # ---- the captured one-token step
    if not a.skip_generate:
        from lwm_amd.llama import LLAMA_STANDARD_CONFIGS
        from lwm_amd.vision_llama import VideoLLaMAConfig, VideoLLaMAForCausalLM
        cfg = VideoLLaMAConfig(**dict(LLAMA_STANDARD_CONFIGS["7b"], num_hidden_layers=a.layers, max_sequence_length=4096,
                                      theta=1e7, sample_mode="text"))
        torch.manual_seed(0)
        with torch.device("cuda"):
            model = VideoLLaMAForCausalLM(cfg)
        ids = torch.randint(3, 32000, (1, a.prompt), device="cuda", generator=g)
        am = torch.ones(1, a.prompt, dtype=torch.int32, device="cuda")
        legs = {"off": ("this", None), "on_p0.9": ("this", 0.9)}
        if a.other_lib:
            legs["other_off"] = ("other", None)

        def run(which, p, n):
            use(which)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = model.generate(ids, attention_mask=am, max_new_tokens=n, max_length=a.prompt + a.long, temperature=1.0,
                                 do_sample=True, seed=1, graph=True, top_p=p)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, out

        for spec in legs.values():
            run(*spec, 4)
        per = {name: [] for name in legs}
        toks = {}
        for _ in range(a.reps):
            for name, spec in legs.items():
                t_short = run(*spec, a.short)[0]
                t_long, toks[name] = run(*spec, a.long)
                per[name].append((t_long - t_short) / (a.long - a.short) * 1e3)
        use("this")
        res["generate_ms_per_token"] = {name: stats(v) for name, v in per.items()}
        res["generate"] = (f"generate(do_sample=True, seed=, graph=True), {a.layers}-layer LWM-7B slice, bf16, 1 row, prompt "
                           f"{a.prompt}, T 1, no top-k, tokens {a.short} -> {a.long}")
        if a.other_lib:
            res["other_off_tokens_equal_off"] = bool(torch.equal(toks["other_off"], toks["off"]))
        res["on_tokens_differ_from_off"] = not bool(torch.equal(toks["on_p0.9"], toks["off"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
