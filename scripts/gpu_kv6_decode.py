"""What the 6-bit (MXFP6 e2m3) KV cache buys and costs on the MI355X, measured in one process (csrc/attn_decode_kv6.h,
csrc/attn_prefill_kv6.h), beside the bf16, the 8-bit and the 4-bit caches of the same build:

  attention   one decode attention step (Q = 1, B = 1, H = 32, Sk = 131072 fully visible, _pick_splits pieces): kernel +
              combine for bf16, fp8, fp6 and fp4 -- and, with --parent-lib, the fp8 and fp4 kernels of a liblwm_hip.so built
              from the parent commit (the shared skeleton changed; did it cost them time?) -- alternated within every
              round, device events, median and min .. max over the rounds; achieved TB/s over the bytes the algorithm
              needs: 2 * Sk * H * (256 | 132 | 100 | 68) + Sk (rows, scales, mask).
  block       4096 queries at the end of 131072 keys (B = 1, H = 32, _pick_splits pieces), kernel + combine: the fp6 block
              kernel, the fp8 block kernel, and the bf16 split-K kernel over a bf16 cache, alternated likewise.
  generate    LLaMAForCausalLM.generate(graph=True) milliseconds per token on the 4-layer LWM-7B slice (prompt 2048,
              max_length 32768) and with a 131072-row cache that the prompt nearly fills, for the four caches, alternated;
              per-token time = (long run - short run) / extra tokens.
  prefill     a 131072-token prompt through the same slice in blocks of 8192 with the fp6, the fp8 and the default cache:
              seconds and peak bytes (in all, and above what was allocated before the prefill).
  movement    the tiny HF fixture, teacher forced: per-step logit movement against the bf16 cache (of the largest logit)
              and changed greedy tokens for fp8, fp6 and fp4.

Every step runs under a time limit of its own: when one expires the process ends there and starts nothing more on the
GPU.  Results: one JSON document (rewritten after every step) and the tables of profiles/r23_kv6_decode.md.

python scripts/gpu_kv6_decode.py [--only attention,block,movement,generate,prefill] [--parent-lib SO] [--out JSON] [--md FILE]
(generate = generate_short,generate_long; --merge JSON carries the steps of an earlier run over, so that a run can be split)"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scripts.gpu_kv4_decode import _events, _spread, limit  # noqa: E402

KINDS = (("bf16", None), ("fp8", "fp8"), ("fp6", "fp6"), ("fp4", "fp4"))
PER_HEAD = {"bf16": 256, "fp8": 132, "fp6": 100, "fp4": 68}


def _formats():
    from lwm_amd import kv4, kv6, ops
    return {"fp8": ops.KV8, "fp6": kv6.KV6, "fp4": kv4.KV4}


def _quantised(torch, f, x):
    from lwm_amd import ops
    B, S, H, _ = x.shape
    c = torch.empty(B, S, H, f.head_bytes, dtype=torch.uint8, device="cuda")
    s = torch.empty((B, S, H) + f.scale_tail, dtype=f.scale_dtype, device="cuda")
    ops._kvq_cache_write(f, c, s, x, dst_row0=0)
    return c, s


def _parent_decode(torch, so, f, q, ck, ks, cv, vs, mask, ns):
    """a decode call of format f through another liblwm_hip.so (the parent commit's): the partials only, as the kernel is
    what is compared; the argument struct is laid out as in this tree (LwmKv8DecodeArgs / LwmKv4DecodeArgs did not change)"""
    from lwm_amd import _capi, ops
    fn = getattr(so, f.decode)
    fn.restype, fn.argtypes = _capi.PROTOTYPES[f.decode]
    B, _, H, D = q.shape
    a = f.decode_args()
    a.q = ops._t4(q, "q", torch.bfloat16)
    a.k, a.v, a.k_scale, a.v_scale = ck.data_ptr(), cv.data_ptr(), ks.data_ptr(), vs.data_ptr()
    a.k_stride_b, a.k_stride_s, a.k_stride_h = ck.stride()[:3]
    a.v_stride_b, a.v_stride_s, a.v_stride_h = cv.stride()[:3]
    a.k_scale_stride_b, a.k_scale_stride_s = ks.stride()[:2]
    a.v_scale_stride_b, a.v_scale_stride_s = vs.stride()[:2]
    a.dense_mask, a.mask_stride_b = mask.data_ptr(), mask.stride(0)
    a.B, a.Sk, a.H, a.D, a.scale, a.k_splits = B, ck.shape[1], H, D, 1.0 / math.sqrt(D), ns
    o = torch.empty((ns, B, 1, H, D), dtype=torch.float32, device="cuda")
    l = torch.empty((ns, B, H, 1), dtype=torch.float32, device="cuda")
    a.out_acc, a.lse_acc = o.data_ptr(), l.data_ptr()

    def call():
        rc = fn(C.byref(a), ops._stream_ptr())
        if rc:
            raise RuntimeError(f"{f.decode} of the parent library: code {rc}")
        return ops.attn_combine(o, l)
    return call, (o, l)


def attention_step(torch, parent_so, Sk=131072, H=32, rounds=7, iters=20):
    from lwm_amd import ops
    from lwm_amd.ring import _pick_splits
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=g, device="cuda", dtype=torch.float32).to(torch.bfloat16)
    q, k, v = rnd(1, 1, H, 128), rnd(1, Sk, H, 128), rnd(1, Sk, H, 128)
    mask = torch.ones(1, 1, Sk, dtype=torch.uint8, device="cuda")
    ns = _pick_splits(1, 1, H, Sk)
    fns = {"bf16": lambda: ops.attn_combine(*ops.attn_fwd_splitk(q, k, v, k_splits=ns, dense_mask=mask))}
    caches = {}
    for n, f in _formats().items():
        caches[n] = _quantised(torch, f, k) + _quantised(torch, f, v)
        fns[n] = (lambda f=f, c=caches[n]: ops.attn_combine(*ops._kvq_attn_decode(f, q, *c, k_splits=ns, dense_mask=mask)))
    out = {"shape": f"Q=1 B=1 H={H} Sk={Sk} fully visible, {ns} pieces, kernel + combine", "rounds": rounds, "iters_per_round": iters}
    if parent_so is not None:
        so = C.CDLL(parent_so)
        so.lwm_version.restype = C.c_int
        out["parent_lwm_version"] = int(so.lwm_version())
        for n in ("fp8", "fp4"):
            f = _formats()[n]
            call, parts = _parent_decode(torch, so, f, q, *caches[n], mask[:, 0], ns)
            call()
            mine = ops._kvq_attn_decode(f, q, *caches[n], k_splits=ns, dense_mask=mask)
            torch.cuda.synchronize()
            out[f"{n}_partials_torch_equal_parent"] = bool(torch.equal(parts[0].view(torch.int32), mine[0].view(torch.int32)) and
                                                           torch.equal(parts[1].view(torch.int32), mine[1].view(torch.int32)))
            fns[f"{n} (parent)"] = call
    for f in fns.values():
        _events(torch, f, 5)                                              # warm
    t = {n: [] for n in fns}
    for _ in range(rounds):                                               # alternated within every round
        for n, f in fns.items():
            t[n].append(_events(torch, f, iters))
    for n in t:
        nb = 2 * Sk * H * PER_HEAD[n.split()[0]] + Sk
        out[n] = dict(us=_spread([x * 1e6 for x in t[n]]), bytes=nb, tb_per_s=nb / statistics.median(t[n]) * 1e-12)
    out["order"] = list(t)
    return out


def block_step(torch, Sq=4096, Sk=131072, H=32, rounds=5, iters=3):
    from lwm_amd import kv6, kv8, ops
    from lwm_amd.ring import _pick_splits
    g = torch.Generator(device="cuda").manual_seed(1)
    rnd = lambda *s: torch.randn(*s, generator=g, device="cuda", dtype=torch.float32).to(torch.bfloat16)
    q, k, v = rnd(1, Sq, H, 128), rnd(1, Sk, H, 128), rnd(1, Sk, H, 128)
    ns, idx = _pick_splits(1, Sq, H, Sk), Sk - Sq
    c8 = _quantised(torch, _formats()["fp8"], k) + _quantised(torch, _formats()["fp8"], v)
    c6 = _quantised(torch, _formats()["fp6"], k) + _quantised(torch, _formats()["fp6"], v)
    fin = lambda parts: ops.cast_f32_to_bf16(parts[0][0]) if parts[0].shape[0] == 1 else ops.attn_combine(*parts, want_bf16=True)[0]
    fns = {"bf16": lambda: fin(ops.attn_fwd_splitk(q, k, v, k_splits=ns, q_start=idx, causal=True)),
           "fp8": lambda: fin(kv8.attn_prefill_kv8(q, *c8, q_start=idx, k_splits=ns)),
           "fp6": lambda: fin(kv6.attn_prefill_kv6(q, *c6, q_start=idx, k_splits=ns))}
    # the fp6 block kernel against the bf16 kernel on a bf16 copy of the dequantised cache: the same partials
    kd, vd = kv6.kv6_dequant(c6[0], c6[1]), kv6.kv6_dequant(c6[2], c6[3])
    same = None
    if ns >= 2:
        a, b = kv6.attn_prefill_kv6(q, *c6, q_start=idx, k_splits=ns), ops.attn_fwd_splitk(q, kd, vd, k_splits=ns, q_start=idx, causal=True)
        same = bool(torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)))
        del a, b
    del kd, vd
    for f in fns.values():
        _events(torch, f, 1)
    t = {n: [] for n in fns}
    for _ in range(rounds):
        for n, f in fns.items():
            t[n].append(_events(torch, f, iters))
    out = {"shape": f"Sq={Sq} at the end of Sk={Sk}, B=1 H={H}, {ns} pieces, kernel + combine (or cast)", "rounds": rounds,
           "iters_per_round": iters, "fp6_partials_torch_equal_bf16_kernel_on_dequantised_cache": same}
    for n in t:
        out[n] = dict(ms=_spread([x * 1e3 for x in t[n]]))
    for n in ("fp8", "fp6"):
        out[f"bf16_over_{n}_time"] = out["bf16"]["ms"]["median"] / out[n]["ms"]["median"]
    return out


def _slice(torch, max_length, layers=4):
    from lwm_amd.llama import LLaMAConfig, LLaMAForCausalLM
    cfg = LLaMAConfig.load_config("7b", num_hidden_layers=layers, max_sequence_length=max_length, theta=1e7)
    torch.manual_seed(0)
    with torch.device("cuda"):
        return cfg, LLaMAForCausalLM(cfg)


def generate_ms(torch, prompt, max_length, new, short=8, layers=4, reps=2):
    cfg, model = _slice(torch, max_length, layers)
    ids = torch.randint(0, cfg.vocab_size, (1, prompt), device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))

    def run(n, kv):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model.generate(ids, max_new_tokens=n, max_length=max_length, graph=True, kv_dtype=kv)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    for _, kv in KINDS:
        run(3, kv)                                                        # warm
    ts, tl = {n: [] for n, _ in KINDS}, {n: [] for n, _ in KINDS}
    for _ in range(reps):                                                 # alternated
        for n, kv in KINDS:
            ts[n].append(run(short, kv))
        for n, kv in KINDS:
            tl[n].append(run(new, kv))
    out = {"workload": f"generate(graph=True), {layers}-layer slice of LWM-7B, prompt {prompt}, cache max_length {max_length}, "
                       f"B=1, random weights; (run of {new} tokens - run of {short}) / {new - short}",
           "reps": reps}
    for n, _ in KINDS:
        per = [(l - s) / (new - short) * 1e3 for l, s in zip(tl[n], ts[n])]
        out[n + "_ms_per_token"] = dict(best=(min(tl[n]) - min(ts[n])) / (new - short) * 1e3, each_rep=per)
    del model
    torch.cuda.empty_cache()
    return out


def chunked_prefill(torch, S=131072, chunk=8192, layers=4):
    cfg, model = _slice(torch, S + 8, layers)
    ids = torch.randint(0, cfg.vocab_size, (1, S), device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
    pos = torch.arange(S, dtype=torch.int32, device="cuda")[None]
    out = {"workload": f"{S}-token prompt in blocks of {chunk}, {layers}-layer slice of LWM-7B, B=1, random weights; one run each, "
                       "after two warm-up blocks through a throwaway cache (the first call's one-time allocations)"}
    warm = model.init_cache(1, 2 * chunk, kv_dtype="fp6", chunked_prefill=True)
    for a in (0, chunk):
        model.hidden_states(ids[:, a:a + chunk], None, None, pos[:, a:a + chunk].contiguous(), warm)
    del warm
    torch.cuda.empty_cache()
    for name, kv in (("fp6", "fp6"), ("fp8", "fp8"), ("bf16", None)):
        cache = model.init_cache(1, S + 8, **({} if kv is None else dict(kv_dtype=kv, chunked_prefill=True)))
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        t0 = time.perf_counter()
        for a in range(0, S, chunk):
            h = model.hidden_states(ids[:, a:a + chunk], None, None, pos[:, a:a + chunk].contiguous(), cache)
        torch.cuda.synchronize()
        out[name] = dict(seconds=time.perf_counter() - t0, peak_bytes=torch.cuda.max_memory_allocated(),
                         peak_above_start_bytes=torch.cuda.max_memory_allocated() - base,
                         cache_bytes=sum(t.numel() * t.element_size() for c in cache for t in c.values() if torch.is_tensor(t)))
        del cache, h
        torch.cuda.empty_cache()
    del model
    torch.cuda.empty_cache()
    return out


def movement(torch):
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import hf_fixture as F
    from lwm_amd import weights as W
    from lwm_amd.llama import LLaMAForCausalLM
    cfg = W.config_from_hf(F.HF_CONFIG)
    model = LLaMAForCausalLM(cfg).cuda()
    W.load_params(model, W.hf_to_lwm(F.state_dict(), cfg.num_attention_heads))
    gold = np.load(os.path.join(ROOT, "tests", "golden", "hf_llama_tiny.npz"))
    seq, mask = torch.from_numpy(gold["gen_tokens"]).cuda(), torch.from_numpy(gold["gen_mask"]).cuda()
    PL, NEW = mask.shape[1], gold["gen_scores"].shape[1]
    L = PL + NEW
    ext = torch.ones(1, L, dtype=torch.int32, device="cuda")
    ext[:, :PL] = mask

    def run(kind):
        cache = model.init_cache(1, L, **({} if kind is None else dict(kv_dtype=kind)))
        pos = (mask.cumsum(-1) - 1).clamp_min(0).to(torch.int32).contiguous()
        step_in, logits = seq[:, :PL], []
        for t in range(NEW):
            h = model.hidden_states(step_in, ext, None, pos, cache)
            logits.append((h[:, -1].float() @ model.lm_head.float()).cpu())
            step_in, pos = seq[:, PL + t:PL + t + 1], (pos[:, -1:] + 1).contiguous()
        return torch.stack(logits, 1)
    lb = run(None)
    out = {"workload": f"tiny HF fixture, prompt {PL}, {NEW} teacher-forced steps; step 0 is the prompt's own (unquantised) attention"}
    for kind in ("fp8", "fp6", "fp4"):
        lq = run(kind)
        d = ((lq - lb).abs().amax(-1) / lb.abs().max()).flatten().tolist()
        out[kind] = dict(per_step_of_max=d, min_after_prompt=min(d[1:]), max_after_prompt=max(d[1:]),
                         changed_greedy_tokens=int((lq.argmax(-1) != lb.argmax(-1)).sum().item()), steps=NEW)
    return out


def markdown(res):
    """the tables of profiles/r23_kv6_decode.md from the JSON document"""
    sp = lambda u, f: f"{u['median']:{f}} ({u['min']:{f}} .. {u['max']:{f}})"
    L = [f"# The 6-bit (MXFP6 e2m3) KV cache beside the bf16, the 8-bit and the 4-bit cache ({res.get('device', '?')})", "",
         f"Made by `scripts/gpu_kv6_decode.py`, `lwm_version()` {res.get('lwm_version', '?')}; every figure below is from one run of it, one process, "
         "the variants alternated within each round.", ""]
    if "attention" in res:
        a = res["attention"]
        L += [f"## One decode attention step: {a['shape']}", "", f"{a['rounds']} alternated rounds of {a['iters_per_round']} calls; "
              "median (min .. max) microseconds per call; TB/s over the algorithmic bytes.", "",
              "| cache | us per step | bytes | TB/s |", "|---|---|---|---|"]
        L += [f"| {n} | {sp(a[n]['us'], '.1f')} | {a[n]['bytes']} | {a[n]['tb_per_s']:.2f} |" for n in a["order"]]
        L.append("")
        if "parent_lwm_version" in a:
            L += [f"\"(parent)\": the same call through a library built from the parent commit (`lwm_version()` {a['parent_lwm_version']}), "
                  f"before the shared skeleton was generalised.  Partials of the two libraries on these inputs `torch.equal`: "
                  f"fp8 {a['fp8_partials_torch_equal_parent']}, fp4 {a['fp4_partials_torch_equal_parent']}.", ""]
    if "block" in res:
        b = res["block"]
        L += [f"## A block of queries: {b['shape']}", "", f"{b['rounds']} alternated rounds of {b['iters_per_round']} calls; median (min .. max) "
              "milliseconds per call.", "", "| route | ms per block |", "|---|---|"]
        L += [f"| {n} | {sp(b[n]['ms'], '.2f')} |" for n in ("bf16", "fp8", "fp6")]
        eq = b["fp6_partials_torch_equal_bf16_kernel_on_dequantised_cache"]
        L += ["", f"bf16 / fp8 time {b['bf16_over_fp8_time']:.3f}; bf16 / fp6 time {b['bf16_over_fp6_time']:.3f}.  " +
              ("One piece at this shape, and the bf16 entry has a partials form from two pieces on: the bit-for-bit comparison of the fp6 "
               "partials with the bf16 split-K kernel is `tests/test_gpu_kv6.py`'s, at 2 to 4 pieces." if eq is None else
               f"fp6 partials `torch.equal` with the bf16 split-K kernel on a bf16 copy of the dequantised cache: {eq}."), ""]
    for key in sorted(k for k in res if k.startswith("generate_")):
        gm = res[key]
        L += [f"## {gm['workload']}", "", f"| cache | ms per token, best of {gm['reps']} | each repetition |", "|---|---|---|"]
        L += [f"| {n} | {gm[n + '_ms_per_token']['best']:.3f} | {', '.join(f'{x:.3f}' for x in gm[n + '_ms_per_token']['each_rep'])} |" for n, _ in KINDS]
        L.append("")
    if "prefill" in res:
        p = res["prefill"]
        L += [f"## Chunked prefill: {p['workload']}", "", "| cache | seconds | peak GiB | peak above the start GiB | cache GiB |", "|---|---|---|---|---|"]
        L += [f"| {n} | {p[n]['seconds']:.2f} | {p[n]['peak_bytes'] / 2 ** 30:.2f} | {p[n]['peak_above_start_bytes'] / 2 ** 30:.2f} | "
              f"{p[n]['cache_bytes'] / 2 ** 30:.2f} |" for n in ("fp6", "fp8", "bf16")]
        L.append("")
    if "movement" in res:
        m = res["movement"]
        L += [f"## Logit movement against the bf16 cache: {m['workload']}", "",
              "| cache | movement after the prompt, of the largest logit (min .. max) | changed greedy tokens |", "|---|---|---|"]
        L += [f"| {n} | {m[n]['min_after_prompt']:.3f} .. {m[n]['max_after_prompt']:.3f} | {m[n]['changed_greedy_tokens']} of {m[n]['steps']} |"
              for n in ("fp8", "fp6", "fp4")]
        L.append("")
    return "\n".join(L)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="attention,block,movement,generate,prefill")
    ap.add_argument("--parent-lib", default=None, help="a liblwm_hip.so built from the parent commit: its fp8 / fp4 decode kernels are timed too")
    ap.add_argument("--out", default=os.path.join(ROOT, "out", "kv6_decode.json"))
    ap.add_argument("--md", default=None, help="also write the markdown tables here")
    ap.add_argument("--merge", default=None, help="the JSON document of an earlier run: its steps are kept unless this run repeats them")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("needs the MI355X")
    from lwm_amd._lib import lib
    want = set(a.only.split(","))
    res = {}
    if a.merge:
        with open(a.merge) as f:
            res = json.load(f)
    res.update(device=torch.cuda.get_device_name(0), lwm_version=int(lib().lwm_version()))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def save():
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        if a.md:
            with open(a.md, "w") as f:
                f.write(markdown(res))

    with torch.no_grad():
        if "attention" in want:
            with limit("attention", 150):
                res["attention"] = attention_step(torch, a.parent_lib)
            save()
        if "block" in want:
            with limit("block", 150):
                res["block"] = block_step(torch)
            save()
        if "movement" in want:
            with limit("movement", 60):
                res["movement"] = movement(torch)
            save()
        if want & {"generate", "generate_short"}:
            with limit("generate short prompt", 300):
                res["generate_prompt2048_cache32768"] = generate_ms(torch, 2048, 32768, 136)
            save()
        if want & {"generate", "generate_long"}:
            with limit("generate long prompt", 540):
                res["generate_prompt130048_cache131072"] = generate_ms(torch, 131072 - 1024, 131072, 72)
            save()
        if "prefill" in want:
            with limit("prefill", 300):
                res["prefill"] = chunked_prefill(torch)
            save()
    save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
