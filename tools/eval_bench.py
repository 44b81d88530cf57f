"""Teacher-forced evaluation, measured: ``model.evaluate`` (LM head in chunks folded by tmi_logprob_fold) against the route
that existed before it - ``model(features, labels=..., training=False)["logits"]`` materialised, then torch's log_softmax,
gather and argmax on those logits - at the headline shape (Whisper small-ref, B = 8, S = 448, features [8, 80, 3000], bf16)
and at one fp32 point (the same shape).  Both routes end in the same three host sums, so a timed call ends in a device
synchronise.  For every route: the median and the spread of ``--reps`` timed calls after ``--warmup`` untimed ones, the
routes alternating inside every repetition (one process, one box), and the peak device memory of one warm call above the
level before it (torch.cuda.max_memory_allocated).  The chunk widths of ``--chunk_cols`` are swept; per width one more
call runs under ops.PROFILE for the device time of the tmi_logprob_fold launches alone (``fold_kernel_ms``).

Writes one JSON file (default profiles/r09_eval_bench.json) and prints it.
usage: python tools/eval_bench.py [--batch 8] [--seq 448] [--reps 15] [--warmup 3] [--chunk_cols 2048,4096,8192,16384] [--out PATH]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import tethys_speech_amd  # noqa: E402,F401
from tethys_speech_amd import ops, whisper  # noqa: E402


def materialised(model, feats, labels):
    """The route before ``evaluate``: the whole [B, S, V] logits, then torch ops -> the same three sums."""
    logits = model(feats, labels=labels, training=False)["logits"]
    lp = torch.log_softmax(logits[:, :-1], dim=-1, dtype=torch.float32)
    tgt = labels[:, 1:].long()
    tok = lp.gather(-1, tgt[..., None])[..., 0]
    hit = logits[:, :-1].argmax(dim=-1) == tgt
    return float(-tok.double().sum().cpu()), float(hit.double().sum().cpu()), float(tgt.numel())


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def peak_mb(fn, dev):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated(dev) - base) / 2 ** 20, 1)


def point(precision, B, S, widths, reps, warmup, dev):
    model = whisper.create_whisper_model("small", device=dev, precision=precision)
    g = torch.Generator().manual_seed(0)
    feats = torch.randn(B, 80, 3000, generator=g).to(dev)
    labels = torch.randint(0, model.config.vocab_size, (B, S), generator=g, dtype=torch.int32).to(dev)
    routes = {f"evaluate_nc{nc}": (lambda nc=nc: model.evaluate(feats, labels, chunk_cols=nc)) for nc in widths}
    routes["materialised"] = lambda: materialised(model, feats, labels)
    for _ in range(warmup):
        for fn in routes.values():
            fn()
    times = {k: [] for k in routes}
    last = {}
    for _ in range(reps):
        for k, fn in routes.items():  # alternating: every route sees the same drift of the box
            ms, last[k] = timed(fn)
            times[k].append(ms)
    res = {"precision": precision, "batch": B, "seq": S, "reps": reps, "warmup": warmup, "routes": {}}
    for k, fn in routes.items():
        ts = sorted(times[k])
        res["routes"][k] = {"median_ms": round(statistics.median(ts), 3), "min_ms": round(ts[0], 3), "max_ms": round(ts[-1], 3),
                            "peak_MB": peak_mb(fn, dev)}
    # device time of the LM-head part alone, per width (one call under the probe)
    for nc in widths:
        ops.PROFILE = ops.OpProfile()
        try:
            model.evaluate(feats, labels, chunk_cols=nc)
            fold_ms, _, n = ops.PROFILE.totals("logprob_fold")
        finally:
            ops.PROFILE = None
        res["routes"][f"evaluate_nc{nc}"].update(fold_kernel_ms=round(fold_ms, 3), fold_launches=n)
    mat = res["routes"]["materialised"]["median_ms"]
    for nc in widths:
        r = res["routes"][f"evaluate_nc{nc}"]
        r["time_over_materialised"] = round(r["median_ms"] / mat, 3)
    ev = last[f"evaluate_nc{widths[0]}"]
    res["check"] = {"evaluate_loss": ev["loss"], "materialised_loss": last["materialised"][0] / last["materialised"][2],
                    "evaluate_n_correct": ev["n_correct"], "materialised_n_correct": last["materialised"][1]}
    del model
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--seq", type=int, default=448)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--chunk_cols", default="2048,4096,8192,16384")
    ap.add_argument("--fp32_reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_eval_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_bench needs the GPU: there is nothing to measure without it")
    dev = "cuda:0"
    widths = [int(x) for x in args.chunk_cols.split(",")]
    out = {"workload": "whisper_small_evaluate", "device": torch.cuda.get_device_name(0),
           "library_chunk_cols": ops.logprob_chunk_cols(),
           "points": [point("bf16", args.batch, args.seq, widths, args.reps, args.warmup, dev),
                      point("fp32", args.batch, args.seq, widths, args.fp32_reps, 2, dev)]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
