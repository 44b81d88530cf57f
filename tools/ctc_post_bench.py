"""CTC forward-backward, measured: tmi_ctc_posteriors (csrc/ctc_post.hip) and ``Wav2Vec2ForCTC.posteriors``.
Writes ONE JSON document (default profiles/r18_ctc_posteriors.json) and prints it.

Kernels, B 8, V 32, at 5 s and 30 s clips (T 250 / L 40 and T 1500 / L 200, the shapes of tools/ctc_bench.py): the time
of one tmi_ctc_posteriors call (its two launches) with and without ``grad``, next to tmi_ctc_forward and tmi_ctc_viterbi
timed IN THE SAME PROCESS on the same buffers (HIP events around many calls after a warm-up).  What the time is measured
against is those two kernels of this run - the alpha pass alone and the best path - never an earlier run of itself: the
call is an alpha pass that also stores, a beta pass of the same one-barrier-per-frame structure that also loads and
stores, and the occupancy launch.  At both shapes also the largest |gamma - float64 gamma| and |grad - float64 grad| over
the batch, against the reference of tests/_ctc_post_ref.py on the host, and what the rows of occ sum to.

Model, base size, bf16, B 8, 5 s clips: ``posteriors`` (with and without ``return_logit_grad``) next to ``align`` and
``forward_infer`` (device time per call).

bench.py measures training and stays as it is; nothing in the tests depends on these numbers.

usage: python tools/ctc_post_bench.py [--out profiles/r18_ctc_posteriors.json] [--iters 30]"""
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
    import _ctc_post_ref as P
    import _ctc_ref as C
    g = torch.Generator(device=dev).manual_seed(T)
    i32 = dict(dtype=torch.int32, device=dev)
    logits = torch.randn(B * T, V, device=dev, generator=g) * 1.5
    logp, amax = torch.empty(B, T, V, device=dev), torch.empty(B * T, **i32)
    ops.ctc_logsoftmax(logits, V, logp.view(B * T, V), amax)
    labels_h = np.stack([C.labels_for("random", L, V, seed=b) for b in range(B)])
    labels = torch.from_numpy(labels_h).to(**i32)
    ll, fl = torch.full((B,), L, **i32), torch.full((B,), T, **i32)
    nll, bad, total = torch.empty(B, device=dev), torch.empty(B, **i32), torch.empty(B, device=dev)
    ts, te, states = torch.empty(B, L, **i32), torch.empty(B, L, **i32), torch.empty(B, T, **i32)
    ws = torch.empty(ops.ctc_workspace_elems(B, L, T), **i32)
    gamma, occ, grad = torch.empty(B, T, 2 * L + 1, device=dev), torch.empty(B, T, V, device=dev), torch.empty(B, T, V, device=dev)
    tf, tc = torch.empty(B, L, device=dev), torch.empty(B, L, device=dev)
    n = max(5, iters // 3)
    # alternating, so that a drift of the clocks reaches every figure alike
    t = {"forward": [], "viterbi": [], "post": [], "post_grad": []}
    for _ in range(3):
        t["forward"].append(timed_us(lambda: ops.ctc_forward(logp, labels, ll, fl, 0, nll, bad), n))
        t["viterbi"].append(timed_us(lambda: ops.ctc_viterbi(logp, labels, ll, fl, 0, ts, te, total, bad, ws, states), n))
        t["post"].append(timed_us(lambda: ops.ctc_posteriors(logp, labels, ll, fl, 0, nll, bad, gamma, occ, tf, tc), n))
        t["post_grad"].append(timed_us(lambda: ops.ctc_posteriors(logp, labels, ll, fl, 0, nll, bad, gamma, occ, tf, tc, grad), n))
    med = {k: float(np.median(v)) for k, v in t.items()}
    torch.cuda.synchronize()
    lp64, gh, grh, och = logp.double().cpu().numpy(), gamma.double().cpu().numpy(), grad.double().cpu().numpy(), occ.double().cpu().numpy()
    e_gamma = e_grad = b_gamma = 0.0
    for b in range(B):
        ref = P.post_ref(lp64[b], labels_h[b], T)
        e_gamma = max(e_gamma, float(np.abs(gh[b] - ref["gamma"]).max()))
        e_grad = max(e_grad, float(np.abs(grh[b] - ref["grad"]).max()))
        b_gamma = max(b_gamma, float(ref["b_gamma"].max()))
    return {"T": T, "L": L, "states": 2 * L + 1,
            "forward_us": round(med["forward"], 1), "viterbi_us": round(med["viterbi"], 1),
            "posteriors_us": round(med["post"], 1), "posteriors_with_grad_us": round(med["post_grad"], 1),
            "posteriors_over_forward": round(med["post"] / med["forward"], 2),
            "posteriors_over_viterbi": round(med["post"] / med["viterbi"], 2),
            "posteriors_us_per_frame": round(med["post"] / T, 3),
            "repeats_us": {k: [round(x, 1) for x in v] for k, v in t.items()},
            "max_abs_gamma_minus_float64": e_gamma, "max_abs_grad_minus_float64": e_grad, "derived_bound_gamma": b_gamma,
            "max_abs_occ_row_sum_minus_1": float(np.abs(och.sum(axis=2) - 1.0).max()), "infeasible": int(bad.sum())}


def model(dev, iters, seconds=5.0, L=40):
    import _ctc_ref as C
    m = wav2vec2.create_full_model("asr", "base", device=dev, precision="bf16")
    T_in = int(seconds * 16000)
    audio = (torch.randn(B, T_in, generator=torch.Generator().manual_seed(0)) * 0.1).to(dev)
    labels = torch.from_numpy(np.stack([C.labels_for("random", L, V, seed=b) for b in range(B)]))
    T = wav2vec2.frame_lengths(m.config, [T_in])[0]
    return {"B": B, "seconds": seconds, "frames": T, "labels": L,
            "forward_infer_us": round(timed_us(lambda: m.forward_infer(audio), iters, warm=3), 1),
            "align_us": round(timed_us(lambda: m.align(audio, labels), iters, warm=3), 1),
            "posteriors_us": round(timed_us(lambda: m.posteriors(audio, labels), iters, warm=3), 1),
            "posteriors_with_logit_grad_us": round(timed_us(lambda: m.posteriors(audio, labels, return_logit_grad=True), iters, warm=3), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_ctc_posteriors.json"))
    ap.add_argument("--iters", type=int, default=30)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "iters": args.iters,
           "timing": "HIP events around iters / 3 (at least 5) back-to-back calls after 5 warm-up calls, three rounds "
                     "alternating forward, viterbi, posteriors, posteriors with grad; the median of the three",
           "measured_against": "tmi_ctc_forward and tmi_ctc_viterbi timed in this same run on the same buffers, never an "
                               "earlier run of tmi_ctc_posteriors",
           "shape": {"B": B, "V": V, "blank": 0},
           "kernels": [kernels(dev, T, L, args.iters) for T, L in ((250, 40), (1500, 200))]}
    res["wav2vec2_base_bf16"] = model(dev, max(5, args.iters // 3))
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
