"""Error-rate evaluation, measured: tmi_edit_distance (csrc/edit.hip), ``evaluate_generate`` and
``Wav2Vec2ForCTC.evaluate(edit_ops=True)``.  Writes ONE JSON document (default profiles/r23_edit_distance.json) and prints it.

Kernel: the time per call (HIP events around many launches after a warm-up) at
  the Whisper shape   8 and 64 pairs of about 448 / 448 tokens (a 50000-id vocabulary, the hypothesis a corrupted reference),
  the CTC shape       8 pairs, hypotheses of about 300 tokens against 200 labels (31 symbols),
  words               64 pairs of about 40 / 40 (the reference fits one wave: no barrier between diagonals),
  the limit           one pair of 4096 / 4096,
each next to ``wav2vec2.edit_distance`` (numpy, one row per hypothesis token) looped over the same pairs on the host in the
same run (wall clock, the tokens already on the host: the copy is not counted), with the distances compared.
Model: ``evaluate_generate`` next to ``generate`` alone (Whisper small, bf16, B 8, 30 s of features, 24 tokens), and
``Wav2Vec2ForCTC.evaluate`` (base, bf16, B 8, 5 s clips, 60 labels each) with and without ``edit_ops``, greedy and K 4.

bench.py measures training and stays as it is; nothing in the tests depends on these numbers.

usage: python tools/edit_distance_bench.py [--out profiles/r23_edit_distance.json] [--iters 20]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import tethys_speech_amd  # noqa: E402,F401
from tethys_speech_amd import ops, wav2vec2, whisper  # noqa: E402


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


def corrupt(rng, ref, vocab, rate, target):
    """A hypothesis: the reference with a share ``rate`` of substitutions, deletions and insertions, cut or padded to about
    ``target`` tokens."""
    out = []
    for x in ref:
        u = rng.random()
        if u < rate / 3:
            continue
        out.append(int(rng.integers(0, vocab)) if u < 2 * rate / 3 else int(x))
        if u > 1 - rate / 3:
            out.append(int(rng.integers(0, vocab)))
    while len(out) < target:
        out.append(int(rng.integers(0, vocab)))
    return out[:target]


def kernel(dev, name, N, n, m, vocab, iters, rate=0.15, exact=False):
    rng = np.random.default_rng(N * 7 + n)
    cols_h, cols_r = n, m
    hyp, ref = np.full((N, cols_h), -1, np.int32), np.full((N, cols_r), -1, np.int32)
    hl, rl = np.zeros(N, np.int32), np.zeros(N, np.int32)
    for i in range(N):
        rl[i] = m if exact else int(rng.integers(max(1, m - m // 8), m + 1))
        hl[i] = n if exact else int(rng.integers(max(1, n - n // 8), n + 1))
        ref[i, :rl[i]] = rng.integers(0, vocab, rl[i])
        hyp[i, :hl[i]] = corrupt(rng, ref[i, :rl[i]], vocab, rate, hl[i])
    d = [torch.from_numpy(a).to(dev) for a in (hyp, ref, hl, rl)]
    out = torch.empty(N, 6, dtype=torch.int32, device=dev)
    us = timed_us(lambda: ops.edit_distance(d[0], d[1], d[2], d[3], out=out), iters)
    got = out.cpu().numpy()
    t0 = time.perf_counter()
    host = [wav2vec2.edit_distance(hyp[i, :hl[i]], ref[i, :rl[i]]) for i in range(N)]
    host_us = (time.perf_counter() - t0) * 1e6
    return {"shape": name, "pairs": N, "hyp_cols": n, "ref_cols": m, "mean_hyp_len": float(hl.mean()), "mean_ref_len": float(rl.mean()),
            "kernel_us": round(us, 1), "host_loop_us": round(host_us, 1), "host_over_kernel": round(host_us / us, 2),
            "diagonals": int((hl + rl).max()) + 1, "us_per_diagonal": round(us / (int((hl + rl).max()) + 1), 3),
            "mean_distance": float(got[:, 0].mean()), "distances_equal_to_host": bool((got[:, 0] == np.asarray(host)).all())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23_edit_distance.json"))
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "iters": args.iters,
           "timing": "kernel and model calls: HIP events around `iters` back-to-back calls after 3 warm-up calls (the model "
                     "calls include their host work and read-backs); host loop: one pass, wall clock, tokens already on the host",
           "kernel": [kernel(dev, "whisper", 8, 448, 448, 50000, args.iters),
                      kernel(dev, "whisper", 64, 448, 448, 50000, args.iters),
                      kernel(dev, "ctc", 8, 300, 200, 31, args.iters, rate=0.3),
                      kernel(dev, "words", 64, 40, 40, 5000, args.iters),
                      kernel(dev, "limit", 1, 4096, 4096, 50000, max(3, args.iters // 4), exact=True)]}

    B = 8
    m = whisper.create_whisper_model("small", device=dev, precision="bf16")
    feats = (torch.randn(B, m.config.n_mels, 3000, generator=torch.Generator().manual_seed(0)) * 0.5).to(dev)
    labels = torch.randint(3, 50000, (B, 24), generator=torch.Generator().manual_seed(1)).to(torch.int32).to(dev)
    it = max(2, args.iters // 5)
    w = {"B": B, "max_length": 24, "iters": it}
    for name, kw in (("greedy", {}), ("beam4_nbest4", dict(num_beams=4, num_return_sequences=4))):
        w[f"generate_{name}_us"] = round(timed_us(lambda: m.generate(feats, max_length=24, **kw), it, warm=1), 1)
        w[f"evaluate_generate_{name}_us"] = round(timed_us(lambda: m.evaluate_generate(feats, labels, max_length=24, **kw), it, warm=1), 1)
    res["whisper_small_bf16"] = w
    del m

    c = wav2vec2.create_full_model("asr", "base", device=dev, precision="bf16")
    audio = (torch.randn(B, 5 * 16000, generator=torch.Generator().manual_seed(0)) * 0.1).to(dev)
    V = c.config.vocab_size
    lab = torch.randint(1, V, (B, 60), generator=torch.Generator().manual_seed(2))
    lab[lab == c.config.ctc_blank_id] = (c.config.ctc_blank_id + 1) % V
    e = {"B": B, "seconds": 5.0, "labels": 60, "iters": args.iters}
    for name, kw in (("greedy", {}), ("num_beams_4", dict(num_beams=4))):
        e[f"evaluate_{name}_us"] = round(timed_us(lambda: c.evaluate(audio, lab, **kw), args.iters), 1)
        e[f"evaluate_{name}_edit_ops_us"] = round(timed_us(lambda: c.evaluate(audio, lab, edit_ops=True, **kw), args.iters), 1)
        a, b = c.evaluate(audio, lab, **kw), c.evaluate(audio, lab, edit_ops=True, **kw)
        e[f"{name}_same_n_edits"] = a["n_edits"] == b["n_edits"]
        e[f"{name}_mean_hyp_tokens"] = b["n_hyp_tokens"] / B
    res["wav2vec2_base_bf16"] = e
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
