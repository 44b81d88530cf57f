"""Wav2Vec2 evaluation, measured (Wav2Vec2-base, bf16, B = 8, clips of 2 s / 5 s / 30 s = 100 / 250 / 1500 frames), in one call:

1. ``model.evaluate`` per batch next to ``model.forward_infer`` on the same batch: the difference is the quantiser branch, the
   two projection heads, tmi_contrastive_score and tmi_vq_count (about ten launches) and the host reads of the sums.  Host
   clock around a call that ends in a device synchronise.
2. ``tmi_contrastive_score`` next to the route that existed before it on the same [B, T, 256] tensors and indices: the
   all-pairs ``tmi_gemm`` into S [B, T, T] fp32 plus ``tmi_contrastive_fwd_bwd`` (which also writes the gradient over S).
   Device events around ``--inner`` back-to-back launches, divided by that count; and the bytes each route allocates for its
   results and scratch.

The alternatives alternate inside every iteration after ``--warmup`` untimed ones, ``--iters`` (>= 50) iterations each, and the
whole run is repeated ``--runs`` times: the spread of a number is the range of its per-run medians, and a difference is
reported only when it is larger than the two spreads together ("beyond_spread").

Writes one JSON file (default profiles/r10_w2v_eval_bench.json) and prints it.
usage: python tools/w2v_eval_bench.py [--batch 8] [--iters 50] [--warmup 5] [--runs 3] [--inner 20] [--clips 32000,80000,480000]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import tethys_speech_amd  # noqa: E402,F401
from tethys_speech_amd import ops, wav2vec2  # noqa: E402


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def device_ms(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


def alternate(routes, timer, iters, warmup, runs):
    """-> {route: {"median_ms", "run_medians_ms", "spread_ms"}}: per run the median of ``iters`` timings, the routes taking
    turns inside every iteration; the spread is the range of the run medians."""
    for _ in range(warmup):
        for fn in routes.values():
            fn()
    meds = {k: [] for k in routes}
    for _ in range(runs):
        ts = {k: [] for k in routes}
        for _ in range(iters):
            for k, fn in routes.items():
                ts[k].append(timer(fn))
        for k in routes:
            meds[k].append(statistics.median(ts[k]))
    return {k: {"median_ms": round(statistics.median(v), 4), "run_medians_ms": [round(x, 4) for x in v],
                "spread_ms": round(max(v) - min(v), 4)} for k, v in meds.items()}


def compare(res, a, b):
    d = res[a]["median_ms"] - res[b]["median_ms"]
    return {"difference_ms": round(d, 4), "beyond_spread": abs(d) > res[a]["spread_ms"] + res[b]["spread_ms"]}


def model_point(model, B, clip, args, dev):
    cfg = model.config
    T = wav2vec2.frame_lengths(cfg, [clip])[0]
    rng = np.random.default_rng(clip)
    audio = torch.from_numpy(rng.standard_normal((B, clip)).astype(np.float32)).to(dev)
    neg = torch.from_numpy(wav2vec2.sample_negative_indices(rng, B, T, cfg.num_negatives)).to(dev)
    routes = {"forward_infer": lambda: model.forward_infer(audio), "evaluate": lambda: model.evaluate(audio, neg)}
    res = alternate(routes, host_ms, args.iters, args.warmup, args.runs)
    res["evaluate_minus_forward_infer"] = compare(res, "evaluate", "forward_infer")
    return {"clip_samples": clip, "frames": T, "batch": B, **res}


def kernel_point(B, T, args, dev, pd=256, Nn=100, temperature=0.1):
    rng = np.random.default_rng(T)
    h = torch.from_numpy(rng.standard_normal((B, T, pd))).to(torch.bfloat16).to(dev)
    q = (2.5 / np.sqrt(pd) * h.float() + torch.from_numpy(rng.standard_normal((B, T, pd))).float().to(dev)).to(torch.bfloat16)
    neg = torch.from_numpy(wav2vec2.sample_negative_indices(rng, B, T, Nn)).to(dev)
    R = B * T
    row_loss = torch.empty(R, dtype=torch.float32, device=dev)
    row_correct = torch.empty(R, dtype=torch.int32, device=dev)
    S = torch.empty(B, T, T, dtype=torch.float32, device=dev)
    row_loss2 = torch.empty(R, dtype=torch.float32, device=dev)

    def gathered():
        ops.contrastive_score(h, q, neg, row_loss, row_correct, B, T, pd, Nn, temperature, validate=False)

    def all_pairs():  # the step's route (wav2vec2.py _forward_backward): S = h . q^T per batch, then the loss over S
        ops.gemm(h, q, S, T, T, pd, pd, 1, 1, pd, T, nbatch=B, a_sb=T * pd, b_sb=T * pd, c_sb=T * T)
        ops.contrastive_fwd_bwd(S, neg, row_loss2, B, T, Nn, temperature, 1.0 / R)

    res = alternate({"contrastive_score": gathered, "gemm_plus_contrastive_fwd_bwd": all_pairs},
                    lambda fn: device_ms(fn, args.inner), args.iters, args.warmup, args.runs)
    res["score_minus_all_pairs"] = compare(res, "contrastive_score", "gemm_plus_contrastive_fwd_bwd")
    torch.cuda.synchronize()
    agree = float((row_loss.double() - row_loss2.double()).abs().max())
    return {"frames": T, "batch": B, "pd": pd, "negatives": Nn, **res,
            "bytes_allocated": {"contrastive_score": row_loss.numel() * 4 + row_correct.numel() * 4,
                                "gemm_plus_contrastive_fwd_bwd": S.numel() * 4 + row_loss2.numel() * 4},
            "flop": {"contrastive_score": 2 * R * (Nn + 1) * pd, "gemm_plus_contrastive_fwd_bwd": 2 * R * T * pd},
            "max_abs_row_loss_difference": agree}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--clips", default="32000,80000,480000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_w2v_eval_bench.json"))
    args = ap.parse_args()
    if args.iters < 50:
        ap.error("--iters must be at least 50")
    if not torch.cuda.is_available():
        raise SystemExit("w2v_eval_bench needs the GPU: there is nothing to measure without it")
    dev = "cuda:0"
    clips = [int(x) for x in args.clips.split(",")]
    model = wav2vec2.create_full_model("pretraining", "base", device=dev, precision="bf16")
    frames = [wav2vec2.frame_lengths(model.config, [c])[0] for c in clips]
    out = {"workload": "wav2vec2_base_evaluate", "device": torch.cuda.get_device_name(0), "precision": "bf16",
           "iters": args.iters, "warmup": args.warmup, "runs": args.runs, "inner_launches": args.inner,
           "model": [model_point(model, args.batch, c, args, dev) for c in clips]}
    del model
    torch.cuda.empty_cache()
    out["kernel"] = [kernel_point(args.batch, T, args, dev) for T in frames]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
