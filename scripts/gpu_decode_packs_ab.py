"""Host-side cost of the decode-weight route, one TREE per process (profiles/r28_decode_packs.md, section 3): run it on the
parent's tree and on the change's in alternation (P C P C P C) and compare the medians against the parent's own spread.

  generate   ms per token of generate(graph=False) and generate(graph=True) on the 4-layer LWM-7B slice of
             scripts/gpu_w6_probe.py (short prompt, B = 1, bf16 cache) with bf16, fp8, fp6 and fp4 decode weights: (run of
             `new` tokens - run of `short`) / (new - short), median of `reps` alternated runs.  The eager path is launch-bound:
             what a change of the Python route costs per step shows there.
  quantise   device time of w8 / w6 / w4 quantise_weight at 4096 x 11008 (events around `calls` calls, median of `reps`).

    python scripts/gpu_decode_packs_ab.py --tree PATH [--json OUT.json]
"""
import argparse
import json
import os
import statistics
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", required=True, help="the checkout whose lwm_amd (built) is measured")
    ap.add_argument("--json", default="")
    ap.add_argument("--new", type=int, default=136)
    ap.add_argument("--short", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    tree = os.path.abspath(a.tree)
    sys.path.insert(0, tree)
    import torch
    import lwm_amd
    assert os.path.dirname(os.path.abspath(lwm_amd.__file__)) == os.path.join(tree, "lwm_amd"), lwm_amd.__file__
    from lwm_amd import w4, w6, w8
    from lwm_amd.llama import LLaMAConfig, LLaMAForCausalLM

    modes = ("bf16", "fp8", "fp6", "fp4")
    cfg = LLaMAConfig.load_config("7b", num_hidden_layers=4, max_sequence_length=4096, theta=1e7)
    torch.manual_seed(0)
    with torch.device("cuda"):
        model = LLaMAForCausalLM(cfg)
    model.quantize_decode_weights("fp4").quantize_decode_weights("fp6").quantize_decode_weights("fp8")   # the rounded model, for every leg
    ids = torch.randint(0, cfg.vocab_size, (1, 64), device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))

    def run(n, mode, graph):
        model.quantize_decode_weights(mode)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model.generate(ids, max_new_tokens=n, max_length=4096, graph=graph)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    out = {"tree": tree, "version": lwm_amd._lib.lib().lwm_version()}
    for graph in (False, True):
        for m in modes:
            run(3, m, graph)                                    # warm
        ts, tl = {m: [] for m in modes}, {m: [] for m in modes}
        for _ in range(a.reps):                                 # alternated
            for m in modes:
                ts[m].append(run(a.short, m, graph))
            for m in modes:
                tl[m].append(run(a.new, m, graph))
        for m in modes:
            per = [(t - min(ts[m])) / (a.new - a.short) * 1e3 for t in tl[m]]
            out[f"generate graph={graph} {m} ms/token"] = round(statistics.median(per), 4)
    del model
    torch.cuda.empty_cache()
    w0 = (torch.randn(4096, 11008, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1)) * 0.02).to(torch.bfloat16)
    for mod in (w8, w6, w4):
        w = w0.clone()
        mod.quantise_weight(w)                                  # warm
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(10):
                mod.quantise_weight(w)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / 10)
        out[f"{mod.__name__.split('.')[-1]} quantise 4096x11008 ms"] = round(statistics.median(ms), 4)
    print(json.dumps(out), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f)


if __name__ == "__main__":
    main()
