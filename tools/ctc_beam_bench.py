"""CTC prefix beam search, measured: tmi_ctc_beam (csrc/ctc_beam.hip) and ``Wav2Vec2ForCTC.decode(num_beams=K)``.
Writes ONE JSON document (default profiles/r17_ctc_beam.json) and prints it.

Kernel, B 8, V 32, K 4 and 16, at 5 s and 30 s clips (T 250 and 1500): the kernel time (HIP events around many launches
after a warm-up) and the time per frame, on peaky log-probs (``peaky_lp`` of tests/_ctc_beam_ref.py, boost 8) and on the
base model's own log-probs (a seeded initialisation: near-uniform rows, the long sequences of an untrained head; the
frames of the 5 s clips, repeated to fill the longer shape).  One
workgroup per item runs its frames one after the other, 2 + (beams kept) barriers each, so the time is the per-frame
latency times T, whatever B is below the number of compute units.

Model, base size, bf16, B 8, 5 s clips: ``decode(num_beams=K)`` next to ``decode()`` (device time per call), and the host
route on the same log-probs: a copy to the CPU, then the float64 reference of tests/_ctc_beam_ref.py (wall clock; K 16 on
one item only, scaled to the batch).

bench.py measures training and stays as it is; nothing in the tests depends on these numbers.

usage: python tools/ctc_beam_bench.py [--out profiles/r17_ctc_beam.json] [--iters 10]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import tethys_speech_amd  # noqa: E402,F401
from tethys_speech_amd import ops, wav2vec2  # noqa: E402

B, V = 8, 32


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


def kernel(dev, logp, K, iters, what):
    N, T, _ = logp.shape
    i32 = dict(dtype=torch.int32, device=dev)
    fl = torch.full((N,), T, **i32)
    tok, ln, sc, nb = torch.empty(N, K, T, **i32), torch.empty(N, K, **i32), torch.empty(N, K, device=dev), torch.empty(N, **i32)
    ws = torch.empty(ops.ctc_beam_workspace_elems(N, K, T), **i32)
    us = timed_us(lambda: ops.ctc_beam(logp, fl, 0, K, tok, ln, sc, nb, ws), iters)
    return {"log_probs": what, "T": T, "K": K, "kernel_us": round(us, 1), "us_per_frame": round(us / T, 3),
            "mean_best_length": float(ln[:, 0].float().mean()), "mean_n_beams": float(nb.float().mean())}


def main():
    import _ctc_beam_ref as R
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_ctc_beam.json"))
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "shape": {"B": B, "V": V, "blank": 0},
           "timing": "HIP events around `iters` back-to-back launches after 3 warm-up launches; the host route: one pass, "
                     "wall clock", "kernel": []}
    m = wav2vec2.create_full_model("asr", "base", device=dev, precision="bf16")
    audio = (torch.randn(B, 5 * 16000, generator=torch.Generator().manual_seed(0)) * 0.1).to(dev)
    logp = m.forward_infer(audio)["log_probs"].contiguous()
    for T in (250, 1500):
        peaky = torch.from_numpy(np.stack([R.peaky_lp(T, V, 100 + b) for b in range(B)]).astype(np.float32)).to(dev)
        own = logp.repeat(1, -(-T // logp.shape[1]), 1)[:, :T].contiguous()   # (the 5 s clips' frames, repeated for 30 s)
        for K in (4, 16):
            res["kernel"].append(kernel(dev, peaky, K, args.iters, "peaky"))
            res["kernel"].append(kernel(dev, own, K, args.iters, "model"))
    model = {"B": B, "seconds": 5.0, "frames": int(logp.shape[1]),
             "decode_greedy_us": round(timed_us(lambda: m.decode(audio), args.iters), 1)}
    for K in (4, 16):
        model[f"decode_num_beams_{K}_us"] = round(timed_us(lambda: m.decode(audio, num_beams=K), args.iters), 1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    lp64 = m.forward_infer(audio)["log_probs"].cpu().double().numpy()
    t1 = time.perf_counter()
    refs = [R.beam_ref(lp64[b], 4) for b in range(B)]
    t2 = time.perf_counter()
    R.beam_ref(lp64[0], 16)
    t3 = time.perf_counter()
    d = m.decode(audio, num_beams=4)
    same = [tuple(d["sequences"][b, :int(d["lengths"][b])].tolist()) == refs[b]["tokens"][0] for b in range(B)]
    model["host_route"] = {"forward_and_copy_s": round(t1 - t0, 4), "float64_reference_K4_s": round(t2 - t1, 3),
                           "float64_reference_K16_s_scaled_from_one_item": round((t3 - t2) * B, 3),
                           "best_sequences_equal_to_decode_K4": float(np.mean(same)),
                           "reference_decided_K4": float(np.mean([r["decided"] for r in refs]))}
    res["wav2vec2_base_bf16"] = model
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
