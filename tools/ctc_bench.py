"""CTC inference, measured: the four kernels of csrc/ctc.hip and ``Wav2Vec2ForCTC.decode`` / ``evaluate`` / ``align``.
Writes ONE JSON document (default profiles/r16_ctc.json) and prints it.

Kernels, B 8, V 32, at 5 s and 30 s clips (T 250 / L 40 and T 1500 / L 200): the kernel time of tmi_ctc_logsoftmax,
tmi_ctc_greedy, tmi_ctc_forward and tmi_ctc_viterbi (HIP events around many launches after a warm-up), and for the two
recursions the time per frame step (one barrier each) - next to it tmi_dtw's recorded 0.45 us per anti-diagonal
(profiles/r15_align.json), the kernel with the same one-barrier-per-step structure.

Model, base size, bf16, B 8, 5 s clips: ``decode`` / ``evaluate`` / ``align`` next to ``forward_infer`` alone (device time
per call), and the host route on the same log-probs: a copy to the CPU, then torch.nn.functional.ctc_loss and the numpy
references of tests/_ctc_ref.py (greedy collapse, Viterbi), one pass, wall clock.

bench.py measures training and stays as it is; nothing in the tests depends on these numbers.

usage: python tools/ctc_bench.py [--out profiles/r16_ctc.json] [--iters 30]"""
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


def timed_us(fn, iters, warm=5):
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


def kernels(dev, T, L, iters):
    import _ctc_ref as C
    g = torch.Generator(device=dev).manual_seed(T)
    i32 = dict(dtype=torch.int32, device=dev)
    logits = torch.randn(B * T, V, device=dev, generator=g) * 1.5
    logp, amax = torch.empty(B, T, V, device=dev), torch.empty(B * T, **i32)
    labels = torch.from_numpy(np.stack([C.labels_for("random", L, V, seed=b) for b in range(B)])).to(**i32)
    ll, fl = torch.full((B,), L, **i32), torch.full((B,), T, **i32)
    tok, st, en = (torch.empty(B, T, **i32) for _ in range(3))
    ol, best, nll, bad = torch.empty(B, **i32), torch.empty(B, device=dev), torch.empty(B, device=dev), torch.empty(B, **i32)
    ts, te = torch.empty(B, L, **i32), torch.empty(B, L, **i32)
    states = torch.empty(B, T, **i32)
    ws = torch.empty(ops.ctc_workspace_elems(B, L, T), **i32)
    t_ls = timed_us(lambda: ops.ctc_logsoftmax(logits, V, logp.view(B * T, V), amax), iters)
    t_gr = timed_us(lambda: ops.ctc_greedy(amax.view(B, T), logp, fl, 0, tok, ol, st, en, best), iters)
    n = max(5, iters // 3)
    t_fw = timed_us(lambda: ops.ctc_forward(logp, labels, ll, fl, 0, nll, bad), n)
    t_vi = timed_us(lambda: ops.ctc_viterbi(logp, labels, ll, fl, 0, ts, te, best, bad, ws, states), n)
    return {"T": T, "L": L, "states": 2 * L + 1, "logsoftmax_us": round(t_ls, 2), "greedy_us": round(t_gr, 2),
            "forward_us": round(t_fw, 1), "forward_us_per_frame": round(t_fw / T, 3), "viterbi_us": round(t_vi, 1),
            "viterbi_us_per_frame": round(t_vi / T, 3), "infeasible": int(bad.sum())}


def model(dev, iters, seconds=5.0, L=40):
    import _ctc_ref as C
    m = wav2vec2.create_full_model("asr", "base", device=dev, precision="bf16")
    T_in = int(seconds * 16000)
    audio = (torch.randn(B, T_in, generator=torch.Generator().manual_seed(0)) * 0.1).to(dev)
    labels = torch.from_numpy(np.stack([C.labels_for("random", L, V, seed=b) for b in range(B)]))
    T = wav2vec2.frame_lengths(m.config, [T_in])[0]
    res = {"B": B, "seconds": seconds, "frames": T, "labels": L,
           "forward_infer_us": round(timed_us(lambda: m.forward_infer(audio), iters, warm=3), 1),
           "decode_us": round(timed_us(lambda: m.decode(audio), iters, warm=3), 1),
           "evaluate_us": round(timed_us(lambda: m.evaluate(audio, labels), iters, warm=3), 1),
           "align_us": round(timed_us(lambda: m.align(audio, labels), iters, warm=3), 1)}
    # the host route: the same log-probs to the CPU, torch's ctc_loss and the numpy references on them
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = m.forward_infer(audio)
    lp, logits = out["log_probs"].cpu(), out["logits"].cpu()
    t1 = time.perf_counter()
    loss = torch.nn.functional.ctc_loss(lp.transpose(0, 1), labels, torch.full((B,), T), torch.full((B,), L), blank=0,
                                        reduction="none")
    t2 = time.perf_counter()
    lp64, amax = lp.double().numpy(), logits.numpy().argmax(axis=2)
    greedy = [C.greedy_ref(amax[b], lp64[b], T, 0) for b in range(B)]
    t3 = time.perf_counter()
    vit = [C.viterbi_ref(lp64[b], labels[b].numpy(), T, dtype=np.float32) for b in range(B)]
    t4 = time.perf_counter()
    ev = m.evaluate(audio, labels, return_items=True)
    al = m.align(audio, labels)
    d = m.decode(audio)
    res["host_route"] = {
        "forward_and_copy_s": round(t1 - t0, 4), "torch_ctc_loss_s": round(t2 - t1, 4), "numpy_greedy_s": round(t3 - t2, 4),
        "numpy_viterbi_s": round(t4 - t3, 4), "total_s": round(t4 - t0, 4),
        "nll_max_abs_diff_to_torch_fp32": float((ev["nll"].cpu() - loss).abs().max()),
        "token_starts_equal_to_align": float(np.mean(np.stack([v["start"] for v in vit]) == al["token_start_frames"].cpu().numpy())),
        "greedy_lengths_equal_to_decode": bool([len(g["tokens"]) for g in greedy] == d["lengths"].tolist())}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_ctc.json"))
    ap.add_argument("--iters", type=int, default=30)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "iters": args.iters,
           "timing": "HIP events around `iters` back-to-back launches after 5 warm-up launches (the recursions and the model "
                     "calls: iters / 3, at least 5); the host route: one pass, wall clock",
           "shape": {"B": B, "V": V, "blank": 0},
           "yardstick": {"tmi_dtw_us_per_anti_diagonal": 0.45, "from": "profiles/r15_align.json"},
           "kernels": [kernels(dev, T, L, args.iters) for T, L in ((250, 40), (1500, 200))]}
    res["wav2vec2_base_bf16"] = model(dev, max(5, args.iters // 3))
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
