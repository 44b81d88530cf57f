"""Greedy decoding, measured: Whisper small-ref, B = 8, features [8, 80, 3000], bf16, EOS disabled (eos_id -1) so that
all 448 steps run.  Prints ONE JSON line: the encoder time (encoder + cross-attention k|v), the whole decode and its
per-step mean, tokens / s, and tmi_lm_head_argmax alone at M = 8 (d 768 and 1280, the bf16 LM head [d, 51904]) in us and
GB/s of weight stream (device time: launches captured in a graph and replayed) beside the per-call time from Python.
bench.py measures training and stays as it is; this is the inference counterpart.

--num_beams K > 1: beam search (B*K decoder rows, EOS disabled so that all steps run), and tmi_lm_head_topk (N = 2K)
against tmi_lm_head_argmax at equal M (8 and 40, d 768 and 1280), both measured in this run, with their time ratio.

--do_sample: sampled decoding (--top_k 50 --top_p 0.9 by default; --top_k 0: Gumbel-max over the vocabulary), EOS disabled,
and tmi_lm_head_sample at M = 8 in both modes beside tmi_lm_head_argmax (M = 8) and tmi_lm_head_topk (M = 8, N = 16),
all measured in this run.

--constrained: decode constraints, all in ONE run (a JSON file, --out): the three constrained LM heads
(tmi_lm_head_argmax_c / _topk_c / _sample_c, sets with 100 seen and 93 banned columns a row) against their originals at
equal M, original and constrained alternating, every pair repeated (median, and the repeats' own spread);
tmi_decode_constraints alone; and greedy, beam-4 and sampled ``generate`` with and without no_repeat_ngram_size 3,
repetition_penalty 1.2 and 90 suppressed ids, alternating too.

--segment_timestamps: the timestamp grammar, all in ONE run (a JSON file, --out): tmi_lm_head_timestamp_gate beside
tmi_lm_head_argmax at equal M, alternating (device time); tmi_timestamp_rules alone; and greedy, beam-4 and sampled
``generate`` with and without ``segment_timestamps=True``, alternating too.

usage: python tools/generate_bench.py [--steps 448] [--batch 8] [--reps 2] [--num_beams 1] [--do_sample [--top_k K] [--top_p P]]
       python tools/generate_bench.py --constrained [--steps 448] [--batch 8] [--reps 3] [--out profiles/r19_generate_constrained.json]
       python tools/generate_bench.py --segment_timestamps [--steps 448] [--batch 8] [--reps 3] [--out profiles/r22_generate_timestamps.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import tethys_speech_amd  # noqa: E402,F401
from tethys_speech_amd import ops, whisper  # noqa: E402


def timed_us(fn, iters=50, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def constraint_sets(dev, M, V=51865, n_seen=100, n_banned=93, seed=0):
    """Bit sets as a decoding step has them: ``n_seen`` seen and ``n_banned`` banned columns a row."""
    g = torch.Generator().manual_seed(seed)
    sets = []
    for n in (n_seen, n_banned):
        rows = [whisper.token_bitset(torch.randperm(V, generator=g)[:n].tolist(), V) for _ in range(M)]
        sets.append(torch.from_numpy(np.stack(rows)).to(dev))
    return sets


def argmax_alone(dev, d, M=8, V=51865, Vp=51904, topk_n=0, sample=None, constrained=False):
    """tmi_lm_head_argmax (topk_n = 0), tmi_lm_head_topk with N = topk_n, or tmi_lm_head_sample with ``sample`` =
    (top_k, top_p), alone on M rows; ``constrained``: the _c entry point on ``constraint_sets`` with penalty 1.2."""
    g = torch.Generator(device=dev).manual_seed(d)
    x = torch.randn(M, d, device=dev, generator=g).to(torch.bfloat16)
    w = (torch.randn(d, Vp, device=dev, generator=g) * 0.03).to(torch.bfloat16)
    gamma, beta = torch.ones(d, device=dev), torch.zeros(d, device=dev)
    cons = {}
    if constrained:
        seen, banned = constraint_sets(dev, M, V)
        cons = dict(seen=seen, banned=banned, penalty=1.2)
    if sample is not None:
        ids, lp = torch.empty(M, dtype=torch.int32, device=dev), torch.empty(M, device=dev)
        fin, cnt = torch.zeros(M, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
        ws = torch.zeros(ops.lm_head_sample_workspace_elems(M, V, sample[0]), dtype=torch.int64, device=dev)
        head = ops.lm_head_sample_c if constrained else ops.lm_head_sample
        call = lambda: head(x, d, w, Vp, M, d, V, ids, 1, fin, cnt, ws, temperature=0.8,  # noqa: E731
                            top_k=sample[0], top_p=sample[1], seed=1, logprob=lp, gamma=gamma, beta=beta, **cons)
    elif topk_n:
        ids = torch.empty(M, topk_n, dtype=torch.int32, device=dev)
        lp = torch.empty(M, topk_n, device=dev)
        ws = torch.zeros(ops.lm_head_topk_workspace_elems(M, V, topk_n), dtype=torch.int64, device=dev)
        head = ops.lm_head_topk_c if constrained else ops.lm_head_topk
        call = lambda: head(x, d, w, Vp, M, d, V, topk_n, ids, lp, ws, gamma=gamma, beta=beta, **cons)  # noqa: E731
    else:
        ids = torch.empty(M, dtype=torch.int32, device=dev)
        cnt = torch.empty(1, dtype=torch.int32, device=dev)
        ws = torch.zeros(M + 1, dtype=torch.int64, device=dev)
        head = ops.lm_head_argmax_c if constrained else ops.lm_head_argmax
        call = lambda: head(x, d, w, Vp, M, d, V, ids, 1, ws, gamma=gamma, beta=beta, eos_id=2,  # noqa: E731
                            eos_count=cnt, **cons)
    eager = timed_us(call)  # per call from Python: host-bound (ctypes + wrapper) at this size
    # device time: n back-to-back launches captured once and replayed (no host in between)
    n = 20
    call()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(n):
            call()
    us = timed_us(graph.replay, iters=10, warm=2) / n
    return {"us": round(us, 2), "GBps": round(d * Vp * 2 / (us * 1e-6) / 1e9, 1), "us_eager_call": round(eager, 2)}


def graph_us(call, n=20):
    """Device time of one ``call``: n launches captured once, the replay timed."""
    call()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(n):
            call()
    return timed_us(graph.replay, iters=10, warm=2) / n


def _stats(vals):
    vals = sorted(vals)
    med = vals[len(vals) // 2]
    return {"median": round(med, 3), "min": round(vals[0], 3), "max": round(vals[-1], 3),
            "spread": round((vals[-1] - vals[0]) / med, 4)}


def constrained_report(args):
    """The --constrained run: see the module docstring."""
    dev, B, reps = "cuda:0", args.batch, max(3, args.reps)
    out = {"what": "tools/generate_bench.py --constrained on one MI355X, one process: originals and constrained forms "
                   "alternating, every figure the median of the repeats with their min, max and (max - min) / median",
           "batch": B, "steps": args.steps, "reps": reps, "precision": "bf16"}
    heads = {}
    for M in (B, 4 * B):
        for name, kw in (("argmax", {}), ("topk_N8", dict(topk_n=8)), ("sample_k50_p0.9", dict(sample=(50, 0.9)))):
            runs = {"original": [], "constrained": []}
            for _ in range(reps):
                for which in ("original", "constrained"):
                    runs[which].append(argmax_alone(dev, 768, M, constrained=which == "constrained", **kw)["us"])
            o, c = _stats(runs["original"]), _stats(runs["constrained"])
            heads[f"M{M}_d768_{name}"] = {"original_us": o, "constrained_us": c,
                                          "constrained_over_original": round(c["median"] / o["median"], 4)}
    out["lm_head"] = heads
    V = 51865
    static = torch.from_numpy(whisper.token_bitset(range(1, 91), V)).to(dev)
    builder = {}
    for M in (B, 4 * B):
        for t in (1, 224, 448):
            prefix = torch.randint(0, V, (M, 449), dtype=torch.int32, device=dev)
            sets = torch.empty(2, M, ops.constraint_words(V), dtype=torch.int32, device=dev)
            call = lambda: ops.decode_constraints(prefix, 449, M, t, V, sets[0], sets[1], ngram=3, static_banned=static)  # noqa: E731
            builder[f"M{M}_t{t}"] = _stats([graph_us(call) for _ in range(reps)])
    out["decode_constraints_us"] = builder
    model = whisper.create_whisper_model("small", device=dev, precision="bf16")
    feats = torch.randn(B, 80, 3000, generator=torch.Generator().manual_seed(0)).to(dev)
    cons = dict(no_repeat_ngram_size=3, repetition_penalty=1.2, suppress_tokens=list(range(1, 91)))
    gen = {}
    for name, mode in (("greedy", {}), ("beam_K4", dict(num_beams=4)),
                       ("sample_k50_p0.9", dict(do_sample=True, top_k=50, top_p=0.9, temperature=0.8, seed=1))):
        runs = {"plain": [], "constrained": []}
        for kw in ({}, cons):
            model.generate(feats, max_length=4, eos_token_id=-1, **mode, **kw)  # warm-up: workspace, kernels
        torch.cuda.synchronize()
        for _ in range(reps):
            for which, kw in (("plain", {}), ("constrained", cons)):
                t0 = time.perf_counter()
                ids = model.generate(feats, max_length=args.steps, eos_token_id=-1, **mode, **kw)
                torch.cuda.synchronize()
                runs[which].append((time.perf_counter() - t0) * 1e3 / args.steps)
                assert ids.shape[1] == 1 + args.steps, ids.shape
        p, c = _stats(runs["plain"]), _stats(runs["constrained"])
        gen[name] = {"plain_per_step_ms": p, "constrained_per_step_ms": c,
                     "constrained_over_plain": round(c["median"] / p["median"], 4),
                     "added_per_step_us": round((c["median"] - p["median"]) * 1e3, 1)}
    out["generate"] = gen
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({"wrote": args.out, "generate": {k: v["constrained_over_plain"] for k, v in gen.items()},
                      "lm_head": {k: v["constrained_over_original"] for k, v in heads.items()}}), flush=True)


def gate_alone(dev, d, M=8, V=51865, Vp=51904, tb=50364):
    """tmi_lm_head_timestamp_gate alone on M rows (``constraint_sets``, penalty 1.2): device time per launch.  The banned
    set is restored by nothing between launches: a row that fired keeps its below columns banned, which changes no work."""
    g = torch.Generator(device=dev).manual_seed(d)
    x = torch.randn(M, d, device=dev, generator=g).to(torch.bfloat16)
    w = (torch.randn(d, Vp, device=dev, generator=g) * 0.03).to(torch.bfloat16)
    gamma, beta = torch.ones(d, device=dev), torch.zeros(d, device=dev)
    seen, banned = constraint_sets(dev, M, V)
    fired = torch.zeros(M, dtype=torch.int32, device=dev)
    ws = torch.zeros(ops.lm_head_timestamp_gate_workspace_elems(M, V), dtype=torch.int64, device=dev)
    call = lambda: ops.lm_head_timestamp_gate(x, d, w, Vp, M, d, V, tb, fired, ws, seen=seen, banned=banned,  # noqa: E731
                                              penalty=1.2, gamma=gamma, beta=beta)
    us = graph_us(call)
    return {"us": round(us, 2), "GBps": round(d * Vp * 2 / (us * 1e-6) / 1e9, 1)}


def timestamps_report(args):
    """The --segment_timestamps run: see the module docstring."""
    dev, B, reps = "cuda:0", args.batch, max(3, args.reps)
    out = {"what": "tools/generate_bench.py --segment_timestamps on one MI355X, one process: the two forms alternating, "
                   "every figure the median of the repeats with their min, max and (max - min) / median",
           "batch": B, "steps": args.steps, "reps": reps, "precision": "bf16"}
    heads = {}
    for M in (B, 4 * B):
        runs = {"argmax": [], "gate": []}
        for _ in range(reps):
            runs["argmax"].append(argmax_alone(dev, 768, M)["us"])
            runs["gate"].append(gate_alone(dev, 768, M)["us"])
        a, g = _stats(runs["argmax"]), _stats(runs["gate"])
        heads[f"M{M}_d768"] = {"argmax_us": a, "timestamp_gate_us": g, "gate_over_argmax": round(g["median"] / a["median"], 4)}
    out["lm_head"] = heads
    V, tb = 51865, 50364
    rules = {}
    for M in (B, 4 * B):
        for t in (1, 224, 448):
            prefix = torch.randint(0, V, (M, 449), dtype=torch.int32, device=dev)
            banned = torch.zeros(M, ops.constraint_words(V), dtype=torch.int32, device=dev)
            call = lambda: ops.timestamp_rules(prefix, 449, M, t, 0, V, tb, banned, no_timestamps_id=tb - 1, eos_id=2,  # noqa: E731
                                               max_initial=50, max_ts=1500)
            rules[f"M{M}_t{t}"] = _stats([graph_us(call) for _ in range(reps)])
    out["timestamp_rules_us"] = rules
    model = whisper.create_whisper_model("small", device=dev, precision="bf16")
    feats = torch.randn(B, 80, 3000, generator=torch.Generator().manual_seed(0)).to(dev)
    ts = dict(segment_timestamps=True)
    gen = {}
    for name, mode in (("greedy", {}), ("beam_K4", dict(num_beams=4)),
                       ("sample_k50_p0.9", dict(do_sample=True, top_k=50, top_p=0.9, temperature=0.8, seed=1))):
        runs = {"plain": [], "timestamps": []}
        for kw in ({}, ts):
            model.generate(feats, max_length=4, eos_token_id=-1, **mode, **kw)  # warm-up: workspace, kernels
        torch.cuda.synchronize()
        for _ in range(reps):
            for which, kw in (("plain", {}), ("timestamps", ts)):
                t0 = time.perf_counter()
                ids = model.generate(feats, max_length=args.steps, eos_token_id=-1, **mode, **kw)
                torch.cuda.synchronize()
                runs[which].append((time.perf_counter() - t0) * 1e3 / args.steps)
                ids = ids["sequences"] if isinstance(ids, dict) else ids
                assert ids.shape[1] == 1 + args.steps, ids.shape
        p, c = _stats(runs["plain"]), _stats(runs["timestamps"])
        gen[name] = {"plain_per_step_ms": p, "timestamps_per_step_ms": c,
                     "timestamps_over_plain": round(c["median"] / p["median"], 4),
                     "added_per_step_us": round((c["median"] - p["median"]) * 1e3, 1)}
    out["generate"] = gen
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({"wrote": args.out, "generate": {k: v["timestamps_over_plain"] for k, v in gen.items()},
                      "lm_head": {k: v["gate_over_argmax"] for k, v in heads.items()}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--constrained", action="store_true")
    ap.add_argument("--segment_timestamps", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=448)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--num_beams", type=int, default=1)
    ap.add_argument("--do_sample", action="store_true")
    ap.add_argument("--top_k", type=int, default=50)
    ap.add_argument("--top_p", type=float, default=0.9)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                "r22_generate_timestamps.json" if args.segment_timestamps else "r19_generate_constrained.json")
    if args.segment_timestamps:
        return timestamps_report(args)
    if args.constrained:
        return constrained_report(args)
    K = args.num_beams
    beam = dict(num_beams=K) if K > 1 else {}
    if args.do_sample:
        if K > 1:
            ap.error("--do_sample does not go with --num_beams > 1")
        beam = dict(do_sample=True, top_k=args.top_k, top_p=args.top_p, temperature=0.8, seed=1)
    dev = "cuda:0"
    model = whisper.create_whisper_model("small", device=dev, precision="bf16")
    B = args.batch
    feats = torch.randn(B, 80, 3000, generator=torch.Generator().manual_seed(0))
    feats_d = feats.to(dev)
    # encoder alone (the first part of every generate call), through the same inference path
    inf = model._infer_prepare(B, 3000, K)

    def encode():
        with model._inference(inf):
            model._cross_kv_infer(model._encode_infer(feats_d, inf))
    enc_ms = timed_us(encode, iters=10, warm=2) / 1e3
    model.generate(feats_d, max_length=4, eos_token_id=-1, **beam)  # warm-up: workspace, kernels
    torch.cuda.synchronize()
    best = None
    for _ in range(args.reps):
        t0 = time.perf_counter()
        ids = model.generate(feats_d, max_length=args.steps, eos_token_id=-1, **beam)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    assert tuple(ids.shape) == (B, 1 + args.steps), ids.shape
    decode_s = best - enc_ms / 1e3
    out = {"workload": "whisper_small_generate" + ("_beam" if K > 1 else "_sample" if args.do_sample else ""), "batch": B, "steps": args.steps,
           "precision": "bf16", "encoder_ms": round(enc_ms, 3), "generate_s": round(best, 4), "decode_s": round(decode_s, 4),
           "per_step_ms": round(decode_s * 1e3 / args.steps, 3), "tokens_per_s": round(B * args.steps / best, 1)}
    if args.do_sample:
        out["top_k"], out["top_p"] = args.top_k, args.top_p
        out["lm_head_M8_d768"] = {"argmax": argmax_alone(dev, 768), "topk_N16": argmax_alone(dev, 768, topk_n=16),
                                  "sample_k50_p0.9": argmax_alone(dev, 768, sample=(50, 0.9)),
                                  "sample_k64_p1": argmax_alone(dev, 768, sample=(64, 1.0)),
                                  "sample_k1": argmax_alone(dev, 768, sample=(1, 1.0)),
                                  "sample_k0_gumbel": argmax_alone(dev, 768, sample=(0, 1.0))}
    elif K > 1:
        out["num_beams"] = K
        out["decoder_rows"] = B * K
        head = {}
        for M in (8, 40):
            for d in (768, 1280):
                am, tk = argmax_alone(dev, d, M), argmax_alone(dev, d, M, topk_n=2 * K)
                head[f"M{M}_d{d}"] = {"argmax": am, f"topk_N{2 * K}": tk, "topk_over_argmax": round(tk["us"] / am["us"], 3)}
        out["lm_head_topk_vs_argmax"] = head
    else:
        out["lm_head_argmax_M8"] = {"d768": argmax_alone(dev, 768), "d1280": argmax_alone(dev, 1280)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
