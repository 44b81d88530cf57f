"""The Wav2Vec2 inference path, measured: Wav2Vec2-base, B = 8, 2 s clips (32000 samples -> 100 frames), bf16.  Every second
clip is cut to 60 % and padded back, so the frame mask has holes at the end of four rows.  Writes ONE JSON document
(default profiles/r08_w2v_infer.json) and prints it:

  * the time per call of ``model(..., attention_mask=mask, pool="mean", training=False)`` and of the same call without a
    mask (host wall clock around synchronised calls, and device time from HIP events);
  * the fused attention launch alone on that layer's shape (B 8, H 12, T 100): mask_mode 2 (key bias: every tile on the
    edge path) next to mask_mode 0 (the branch-free tiles), and both again at T = 1000 where the tile loop dominates;
  * tmi_masked_mean_pool alone on [8, 100, 768] bf16.

bench.py measures training and stays as it is; nothing in the tests depends on these numbers.

usage: python tools/w2v_infer_bench.py [--out profiles/r08_w2v_infer.json] [--iters 50]"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import tethys_speech_amd  # noqa: E402,F401
from tethys_speech_amd import ops, wav2vec2, whisper  # noqa: E402


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


def wall_us(fn, iters, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / iters


def attn_pair(dev, B, H, T, iters):
    d = H * 64
    g = torch.Generator(device=dev).manual_seed(T)
    qkv = torch.randn(B * T, 3 * d, device=dev, generator=g).to(torch.bfloat16)
    o = torch.empty(B * T, d, dtype=torch.bfloat16, device=dev)
    stats = torch.empty(B, H, T, 2, dtype=torch.float32, device=dev)
    kb = torch.zeros(B, T, dtype=torch.float32, device=dev)
    kb[1::2, (3 * T) // 5:] = -10000.0
    m = lambda off: (qkv, off, T * 3 * d, 3 * d)  # noqa: E731
    sc = 1.0 / math.sqrt(64)
    plain = timed_us(lambda: ops.attn_fwd(m(0), m(d), m(2 * d), (o, 0, T * d, d), stats, B, H, T, T, 0, score_scale=sc), iters)
    bias = timed_us(lambda: ops.attn_fwd(m(0), m(d), m(2 * d), (o, 0, T * d, d), stats, B, H, T, T, 2, score_scale=sc,
                                         key_bias=kb), iters)
    return {"B": B, "H": H, "T": T, "mask_mode_0_us": round(plain, 2), "mask_mode_2_us": round(bias, 2),
            "ratio": round(bias / plain, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_w2v_infer.json"))
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, T_in = 8, 32000
    model = wav2vec2.create_full_model("pretraining", "base", device=dev, precision="bf16")
    wave = torch.from_numpy(whisper.dummy_waveform()[:T_in].copy())
    lengths = [T_in if i % 2 == 0 else (3 * T_in) // 5 for i in range(B)]
    audio = torch.stack([torch.cat([wave[:n], torch.zeros(T_in - n)]) for n in lengths]).to(dev)
    mask = wav2vec2.frame_attention_mask(model.config, lengths, T_in)
    masked = lambda: model(audio, attention_mask=mask, pool="mean", training=False)  # noqa: E731
    plain = lambda: model(audio, pool="mean", training=False)  # noqa: E731
    res = {"model": "wav2vec2-base", "precision": "bf16", "batch": B, "samples": T_in, "frames": int(mask.shape[1]),
           "frames_per_clip": [int(x) for x in mask.sum(1).tolist()],
           "masked_forward": {"device_us": round(timed_us(masked, args.iters), 1), "wall_us": round(wall_us(masked, args.iters), 1)},
           "unmasked_forward": {"device_us": round(timed_us(plain, args.iters), 1), "wall_us": round(wall_us(plain, args.iters), 1)},
           "attention_launch": [attn_pair(dev, B, 12, 100, 4 * args.iters), attn_pair(dev, B, 12, 1000, args.iters)]}
    x = torch.randn(B, 100, 768, device=dev).to(torch.bfloat16)
    out = torch.empty(B, 768, device=dev)
    md = mask.to(dev)
    res["masked_mean_pool_us"] = round(timed_us(lambda: ops.masked_mean_pool(x, md, out, B, 100, 768), 4 * args.iters), 2)
    res["device"] = torch.cuda.get_device_name(0)
    text = json.dumps(res, indent=1)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
