"""Token timestamps, measured: tmi_align_cost, tmi_dtw and ``model.align``.  Writes ONE JSON document (default
profiles/r15_align.json) and prints it.

Kernels, at Whisper small's shapes - B 8, H 12, T 1500, S 100 and S 448, bf16 and fp32 weights, all heads selected,
medfilt_width 7, normalised:

  * ``tmi_align_cost``: the kernel time (HIP events around many launches after a warm-up) and the weight bytes it has to
    read (N H S T elements, once) per microsecond; next to it ``tmi_memset_async`` over the same number of bytes in the
    same process on the same device, and the share of that rate the kernel reaches.  The kernel reads the weights three
    times (sum, squares, filter): the figure counts them once.
  * ``tmi_dtw`` over the cost that call left, without and with the path output.

Model, Whisper small bf16, B 8, 3000 frames, 100 tokens per row: ``align`` next to ``forward_infer(output_attentions=
("cross",))`` alone (device time per call), and the host route a user has without ``align``: the fp32 weights of the upper
half of the layers copied to the CPU, then tests/_align_ref.py's float64 cost and DTW on them (one pass, wall clock).

bench.py measures training and stays as it is; nothing in the tests depends on these numbers.

usage: python tools/align_bench.py [--out profiles/r15_align.json] [--iters 30]"""
import argparse
import json
import os
import socket
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import tethys_speech_amd  # noqa: E402,F401
from tethys_speech_amd import ops, whisper  # noqa: E402

B, H, T, WIDTH = 8, 12, 1500, 7


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


def kernels(dev, S, dtype, iters):
    g = torch.Generator(device=dev).manual_seed(S)
    probs = torch.softmax(torch.randn(B, H, S, T, device=dev, generator=g) * 2.0, dim=-1).to(dtype)
    rows = torch.full((B,), S, dtype=torch.int32, device=dev)
    cols = torch.full((B,), T, dtype=torch.int32, device=dev)
    hw = torch.full((H,), 1.0 / H, device=dev)
    cost = torch.zeros(B, S, T, device=dev)
    nbytes = probs.numel() * probs.element_size()
    t_c = timed_us(lambda: ops.align_cost(probs, rows, cols, hw, cost, WIDTH, True), iters)
    t_m = timed_us(lambda: ops.fill_zero(probs), iters)
    st, en = torch.empty(B, S, dtype=torch.int32, device=dev), torch.empty(B, S, dtype=torch.int32, device=dev)
    tot = torch.empty(B, device=dev)
    ws = torch.empty(ops.dtw_workspace_elems(B, S, T), dtype=torch.int32, device=dev)
    path = torch.empty(B, S + T - 1, 2, dtype=torch.int32, device=dev)
    plen = torch.empty(B, dtype=torch.int32, device=dev)
    n = max(5, iters // 3)
    return {"S": S, "weights": "bf16" if dtype == torch.bfloat16 else "fp32", "weight_bytes": nbytes,
            "align_cost_us": round(t_c, 2), "align_cost_weight_bytes_per_us": round(nbytes / t_c, 1),
            "memset_us": round(t_m, 2), "memset_bytes_per_us": round(nbytes / t_m, 1),
            "share_of_memset_rate": round(t_m / t_c, 3),
            "dtw_us": round(timed_us(lambda: ops.dtw(cost, rows, cols, st, en, tot, ws), n), 1),
            "dtw_with_path_us": round(timed_us(lambda: ops.dtw(cost, rows, cols, st, en, tot, ws, path, plen), n), 1),
            "dtw_diagonals": S + T - 1}


def model(dev, iters):
    import _align_ref as A
    S = 100
    m = whisper.create_whisper_model("small", device=dev, precision="bf16")
    feats = torch.randn(B, 80, 3000, generator=torch.Generator().manual_seed(0)).to(dev)
    seq = torch.randint(3, 50000, (B, 1 + S), generator=torch.Generator().manual_seed(1)).to(torch.int32)
    seq[:, 0] = m.config.decoder_start_token_id
    seq = seq.to(dev)
    res = {"B": B, "frames": 3000, "tokens": S,
           "forward_infer_cross_us": round(timed_us(lambda: m.forward_infer(feats, decoder_input_ids=seq, output_attentions=("cross",)),
                                                    iters, warm=3), 1),
           "forward_infer_plain_us": round(timed_us(lambda: m.forward_infer(feats, decoder_input_ids=seq), iters, warm=3), 1),
           "align_us": round(timed_us(lambda: m.align(feats, seq), iters, warm=3), 1),
           "align_with_path_us": round(timed_us(lambda: m.align(feats, seq, return_path=True), iters, warm=3), 1)}
    # the host route: the same weights (fp32, the layers align selects) to the CPU, float64 numpy on them
    Ld, Hd = m.config.decoder_layers, m.config.decoder_attention_heads
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = m.forward_infer(feats, decoder_input_ids=seq, output_attentions=("cross",), attentions_dtype=torch.float32)
    host = [out["cross_attentions"][l][:, :, 1:, :].cpu().numpy() for l in range(Ld // 2, Ld)]
    t1 = time.perf_counter()
    hw = np.full(Hd, 1.0 / (Hd * len(host)), dtype=np.float32)
    cost = None
    for p in host:
        cost, _ = A.cost_ref(p, [S] * B, [T] * B, hw, WIDTH, True, base=cost, with_bound=False)
    t2 = time.perf_counter()
    starts = [A.dtw_ref(cost[b])["start"] for b in range(B)]
    t3 = time.perf_counter()
    al = m.align(feats, seq)
    same = float(np.mean(np.stack(starts) == al["token_start_frames"].cpu().numpy()))
    res["host_route"] = {"forward_and_copy_s": round(t1 - t0, 3), "copied_bytes": int(sum(p.nbytes for p in host)),
                         "numpy_cost_s": round(t2 - t1, 3), "numpy_dtw_s": round(t3 - t2, 3), "total_s": round(t3 - t0, 3),
                         "token_starts_equal_to_align": round(same, 4)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_align.json"))
    ap.add_argument("--iters", type=int, default=30)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "host": socket.gethostname(), "iters": args.iters,
           "timing": "HIP events around `iters` back-to-back launches after 5 warm-up launches (tmi_dtw and the model calls: "
                     "iters / 3, at least 5); the host route: one pass, wall clock",
           "shape": {"B": B, "H": H, "T": T, "medfilt_width": WIDTH, "normalize": True},
           "kernels": [kernels(dev, S, dt, args.iters) for S in (100, 448) for dt in (torch.bfloat16, torch.float32)]}
    res["whisper_small_bf16"] = model(dev, max(5, args.iters // 3))
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
