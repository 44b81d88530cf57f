"""LM fusion in the CTC beam kernel, measured: tmi_ctc_beam_lm next to tmi_ctc_beam (csrc/ctc_beam.hip) in the same run,
and ``Wav2Vec2ForCTC.decode(num_beams=K, lm=...)`` next to ``decode(num_beams=K)``.  Writes ONE JSON document (default
profiles/r20_ctc_lm.json) and prints it.

Kernel, the shapes of tools/ctc_beam_bench.py: B 8, V 32, K 4 and 16, T 250 and 1500, peaky log-probs (``peaky_lp`` of
tests/_ctc_beam_ref.py, boost 8), tables of order 2 and 3 (``lm_table`` of tests/_ctc_lm_ref.py: 4 KiB and 128 KiB, L2
resident), alpha 0.5, beta 0.25.  Each figure is the smallest of ``--repeats`` timings (HIP events around ``--iters``
back-to-back launches after a warm-up), the two kernels taken alternately; ``ratio`` is fused over unfused.  A frame costs
2 + (beams kept) barriers either way; the fusion adds one row load per wave, issued at the top of the frame, and a few
fp32 operations.

Model, base size, bf16, B 8, 5 s clips, the order-2 table: device time per ``decode`` call with and without ``lm``.

bench.py measures training and stays as it is; nothing in the tests depends on these numbers.

usage: python tools/ctc_lm_bench.py [--out profiles/r20_ctc_lm.json] [--iters 10] [--repeats 3]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import tethys_speech_amd  # noqa: E402,F401
from tethys_speech_amd import ops, wav2vec2  # noqa: E402

B, V = 8, 32
ALPHA, BETA = 0.5, 0.25


def timed_us(fn, iters, warm=3):
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


def best_of(fns, iters, repeats):
    """The smallest of ``repeats`` timings of each function, the functions taken alternately."""
    best = [float("inf")] * len(fns)
    for _ in range(repeats):
        for i, fn in enumerate(fns):
            best[i] = min(best[i], timed_us(fn, iters))
    return best


def kernel(dev, logp, K, tables, iters, repeats):
    N, T, _ = logp.shape
    i32 = dict(dtype=torch.int32, device=dev)
    fl = torch.full((N,), T, **i32)
    tok, ln, nb = torch.empty(N, K, T, **i32), torch.empty(N, K, **i32), torch.empty(N, **i32)
    sc, ctc, lms = (torch.empty(N, K, device=dev) for _ in range(3))
    ws = torch.empty(ops.ctc_beam_workspace_elems(N, K, T), **i32)
    fns = [lambda: ops.ctc_beam(logp, fl, 0, K, tok, ln, sc, nb, ws)]
    for order, table in tables:
        fns.append(lambda order=order, table=table: ops.ctc_beam_lm(logp, fl, 0, K, table, order, ALPHA, BETA, tok, ln, sc, ctc,
                                                                    lms, nb, ws))
    us = best_of(fns, iters, repeats)
    row = {"T": T, "K": K, "ctc_beam_us": round(us[0], 1), "ctc_beam_us_per_frame": round(us[0] / T, 3)}
    for (order, _), t in zip(tables, us[1:]):
        row[f"ctc_beam_lm_order{order}_us"] = round(t, 1)
        row[f"ratio_order{order}"] = round(t / us[0], 3)
    return row


def main():
    import _ctc_beam_ref as R
    import _ctc_lm_ref as L
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_ctc_lm.json"))
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "repeats": args.repeats,
           "shape": {"B": B, "V": V, "blank": 0, "log_probs": "peaky", "lm_alpha": ALPHA, "lm_beta": BETA},
           "timing": "the smallest of `repeats` timings, each HIP events around `iters` back-to-back launches after 3 warm-up "
                     "launches; the kernels (and the two decode calls) taken alternately in one process", "kernel": []}
    tables = [(order, torch.from_numpy(L.lm_table(V, order, 7 + order).astype(np.float32).reshape(-1)).to(dev)) for order in (2, 3)]
    for T in (250, 1500):
        peaky = torch.from_numpy(np.stack([R.peaky_lp(T, V, 100 + b) for b in range(B)]).astype(np.float32)).to(dev)
        for K in (4, 16):
            res["kernel"].append(kernel(dev, peaky, K, tables, args.iters, args.repeats))
    ratios = [v for row in res["kernel"] for k, v in row.items() if k.startswith("ratio_")]
    res["ratio_fused_over_unfused"] = {"min": min(ratios), "max": max(ratios), "expected_below": 1.5}
    m = wav2vec2.create_full_model("asr", "base", device=dev, precision="bf16")
    audio = (torch.randn(B, 5 * 16000, generator=torch.Generator().manual_seed(0)) * 0.1).to(dev)
    lm = L.lm_table(V, 2, 9).astype(np.float32).reshape(V, V)
    model = {"B": B, "seconds": 5.0, "frames": int(m.forward_infer(audio)["log_probs"].shape[1]), "lm_order": 2}
    for K in (4, 16):
        plain, fused = best_of([lambda: m.decode(audio, num_beams=K),
                                lambda: m.decode(audio, num_beams=K, lm=lm, lm_alpha=ALPHA, lm_beta=BETA)], args.iters, args.repeats)
        model[f"decode_num_beams_{K}_us"] = round(plain, 1)
        model[f"decode_num_beams_{K}_lm_us"] = round(fused, 1)
        model[f"decode_ratio_K{K}"] = round(fused / plain, 3)
    res["wav2vec2_base_bf16"] = model
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
