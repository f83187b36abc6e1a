"""ms per sampled token of VideoLLaMAForCausalLM.generate_vision on an LWM-7B-shaped vision model (d_model 4096, 32 heads,
FFN 11008, text vocab 32000, vision vocab 8448), classifier-free guidance over one conditional + one unconditional prompt
(B = 2 rows), top-k 8192, T = 1, in three forms measured alternately in one process:
  eager_torch   generator=: the torch sampler, eager one-token steps (the default path of the entry points)
  eager_device  seed=, graph=False: ops.sample_tokens, eager one-token steps
  graph         seed=, graph=True: the one-token step with the sampler captured once in a hipGraph
Per-token time = (long run - short run) / extra tokens (bench.py generate_leg's method: prefill, capture and the first
tokens cancel), host clock around runs that end in a device synchronise.

--kernel-only: just the sampler kernel, at (rows 2, V 8448, k 8192, guided) and (rows 1, V 32000, k 0), for a
`rocprofv3 --kernel-trace --stats` pass of its own.

python scripts/gpu_sample_decode.py [--layers 4] [--prompt 512] [--reps 3] [--out out/sample_decode.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def kernel_only(torch, n=200):
    from lwm_amd import ops
    g = torch.Generator(device="cuda").manual_seed(0)
    lv = torch.randn(2, 8448, device="cuda", generator=g) * 3
    lt = torch.randn(1, 32000, device="cuda", generator=g) * 3
    cfg = torch.tensor([5.0], device="cuda")
    tv = torch.empty(2, 1, dtype=torch.int64, device="cuda")
    tt = torch.empty(1, 1, dtype=torch.int64, device="cuda")
    for i in range(n):
        ops.sample_tokens(lv, temperature=1.0, top_k=8192, seed=1, step=i, cfg_scale=cfg, force_period=257,
                          force_token=8192, tokens_out=tv, copies=2)
        ops.sample_tokens(lt, temperature=0.2, top_k=0, seed=1, step=i, tokens_out=tt)
    torch.cuda.synchronize()
    print(json.dumps({"kernel_only_calls": 2 * n}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--short", type=int, default=16)
    ap.add_argument("--long", type=int, default=514)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "out", "sample_decode.json"))
    ap.add_argument("--kernel-only", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("needs the MI355X")
    if a.kernel_only:
        return kernel_only(torch)
    from lwm_amd.llama import LLAMA_STANDARD_CONFIGS
    from lwm_amd.vision_llama import VideoLLaMAConfig, VideoLLaMAForCausalLM
    cfg = VideoLLaMAConfig(**dict(LLAMA_STANDARD_CONFIGS["7b"], num_hidden_layers=a.layers, max_sequence_length=4096,
                                  theta=1e7, sample_mode="vision"))
    torch.manual_seed(0)
    with torch.device("cuda"):
        model = VideoLLaMAForCausalLM(cfg)
    g = torch.Generator(device="cuda").manual_seed(0)
    ids = torch.randint(0, 8192, (2, a.prompt), device="cuda", generator=g)
    am = torch.ones(2, a.prompt, dtype=torch.int32, device="cuda")
    vm = torch.zeros_like(ids, dtype=torch.bool)
    max_length = a.prompt + a.long
    forms = {
        "eager_torch": lambda n: model.generate_vision(ids, [5.0], attention_mask=am, vision_masks=vm, max_new_tokens=n,
                                                       temperature=1.0, top_k=8192, max_length=max_length,
                                                       generator=torch.Generator(device="cuda").manual_seed(1)),
        "eager_device": lambda n: model.generate_vision(ids, [5.0], attention_mask=am, vision_masks=vm, max_new_tokens=n,
                                                        temperature=1.0, top_k=8192, max_length=max_length, seed=1),
        "graph": lambda n: model.generate_vision(ids, [5.0], attention_mask=am, vision_masks=vm, max_new_tokens=n,
                                                 temperature=1.0, top_k=8192, max_length=max_length, seed=1, graph=True),
    }

    def run(f, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = f(n)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    for f in forms.values():
        run(f, 4)                                           # warm every form
    per = {k: [] for k in forms}
    toks = {}
    for _ in range(a.reps):
        for name, f in forms.items():                      # alternating: one long-minus-short pair per form per rep
            t_short = run(f, a.short)[0]
            t_long, out = run(f, a.long)
            per[name].append((t_long - t_short) / (a.long - a.short) * 1e3)
            toks[name] = out
    res = dict(workload=f"generate_vision, {a.layers}-layer LWM-7B-shaped vision model, bf16, B = 2 rows (1 conditional + 1 "
                        f"unconditional, cfg 5.0), prompt {a.prompt}, top-k 8192, T 1, tokens {a.short} -> {a.long}",
               ms_per_token={k: sorted(v) for k, v in per.items()},
               ms_per_token_median={k: sorted(v)[len(v) // 2] for k, v in per.items()},
               graph_tokens_equal_eager_device=bool(torch.equal(toks["graph"], toks["eager_device"])),
               forced_codes_ok=bool((toks["graph"][:, 256] == 8192).all()),
               device=torch.cuda.get_device_name())
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
