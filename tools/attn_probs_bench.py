"""tmi_attn_probs, measured.  Writes ONE JSON document (default profiles/r11_attn_probs.json) and prints it.

For the shapes  encoder 8x12x1500x1500,  cross 8x12x100x1500,  decoder self 8x12x100x100 (mask_mode 1)  and  Wav2Vec2
8x12x250x250 (score_scale 1/8), and both output dtypes:

  * the kernel time (HIP events around many launches after a warm-up) and the bytes it writes per microsecond;
  * next to it ``tmi_memset_async`` over the same number of bytes in the same process on the same device - the write
    ceiling the kernel is compared with - and the share of that rate the kernel reaches;
  * for the fp32 output, what produces P on the fp32 path: the batched q.k^T GEMM plus ``tmi_softmax_fwd``;
  * the fused forward (``tmi_attn_fwd``) of the same shape, for scale.

Then ``forward_infer`` with and without the outputs for Whisper small (B 8, 3000 frames, S 100) and Wav2Vec2-base (B 8,
5 s clips), bf16, device time per call.

bench.py measures training and stays as it is; nothing in the tests depends on these numbers.

usage: python tools/attn_probs_bench.py [--out profiles/r11_attn_probs.json] [--iters 30]"""
import argparse
import json
import os
import socket
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import tethys_speech_amd  # noqa: E402,F401
from tethys_speech_amd import ops, wav2vec2, whisper  # noqa: E402

SHAPES = [("encoder", 8, 12, 1500, 1500, 0, 1.0), ("cross", 8, 12, 100, 1500, 0, 1.0),
          ("decoder_self", 8, 12, 100, 100, 1, 1.0), ("wav2vec2", 8, 12, 250, 250, 0, 0.125)]


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


def one_shape(dev, name, B, H, Tq, Tk, mode, scale, iters):
    d = H * 64
    g = torch.Generator(device=dev).manual_seed(Tq + Tk)
    q = (torch.randn(B * Tq, d, device=dev, generator=g) * (0.125 if scale == 1.0 else 1.0)).to(torch.bfloat16)
    kv = torch.randn(B * Tk, 2 * d, device=dev, generator=g).to(torch.bfloat16)
    o = torch.empty(B * Tq, d, dtype=torch.bfloat16, device=dev)
    stats = torch.empty(B, H, Tq, 2, dtype=torch.float32, device=dev)
    qm, km, vm, om = (q, 0, Tq * d, d), (kv, 0, Tk * 2 * d, 2 * d), (kv, d, Tk * 2 * d, 2 * d), (o, 0, Tq * d, d)
    fwd = lambda: ops.attn_fwd(qm, km, vm, om, stats, B, H, Tq, Tk, mode, score_scale=scale)  # noqa: E731
    n = 4 * iters if Tq * Tk < 10 ** 6 else iters
    rec = {"shape": name, "B": B, "H": H, "Tq": Tq, "Tk": Tk, "mask_mode": mode, "score_scale": scale,
           "attn_fwd_us": round(timed_us(fwd, n), 2)}
    for dtype, tag in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
        out = torch.empty(B, H, Tq, Tk, dtype=dtype, device=dev)
        nbytes = out.numel() * out.element_size()
        t_k = timed_us(lambda: ops.attn_probs(qm, km, stats, out, B, H, Tq, Tk, mode, score_scale=scale), n)
        t_m = timed_us(lambda: ops.fill_zero(out), n)
        rec[tag] = {"bytes": nbytes, "kernel_us": round(t_k, 2), "kernel_bytes_per_us": round(nbytes / t_k, 1),
                    "memset_us": round(t_m, 2), "memset_bytes_per_us": round(nbytes / t_m, 1),
                    "share_of_memset_rate": round(t_m / t_k, 3)}
        del out
    # the fp32 path's way to P: one batched GEMM over all (sample, head) pairs, then the materialised softmax
    q32, k32 = q.float(), kv[:, :d].float().contiguous()
    P = torch.empty(B, H, Tq, Tk, dtype=torch.float32, device=dev)

    def fp32_path():
        ops.gemm(q32, k32, P, Tq, Tk, 64, d, 1, 1, d, Tk, nbatch=H, a_sb=64, b_sb=64, c_sb=Tq * Tk,
                 scale_cols=Tk if scale != 1.0 else 0, scale=scale, nbatch2=B, a_sb2=Tq * d, b_sb2=Tk * d, c_sb2=H * Tq * Tk)
        ops.softmax_fwd(P, B * H * Tq, Tq, Tk, mode)

    rec["fp32_path_gemm_plus_softmax_us"] = round(timed_us(fp32_path, n), 2)
    return rec


def models(dev, iters):
    res = {}
    B = 8
    m = whisper.create_whisper_model("small", device=dev, precision="bf16")
    feats = torch.randn(B, 80, 3000, generator=torch.Generator().manual_seed(0)).to(dev)
    dec = torch.randint(3, 50000, (B, 100), generator=torch.Generator().manual_seed(1)).to(torch.int32)
    dec[:, 0] = m.config.decoder_start_token_id
    dec = dec.to(dev)
    w = {}
    for tag, kw in (("plain", {}), ("cross", dict(output_attentions=("cross",))),
                    ("cross_decoder_hidden", dict(output_attentions=("cross", "decoder"), output_hidden_states=True)),
                    ("all", dict(output_attentions=True, output_hidden_states=True))):
        w[tag + "_us"] = round(timed_us(lambda: m.forward_infer(feats, decoder_input_ids=dec, **kw), iters, warm=3), 1)
    res["whisper_small_B8_T1500_S100_bf16"] = w
    del m
    torch.cuda.empty_cache()
    v = wav2vec2.create_full_model("pretraining", "base", device=dev, precision="bf16")
    audio = torch.randn(B, 80000, generator=torch.Generator().manual_seed(2)).to(dev)
    r = {"frames": int(wav2vec2.frame_lengths(v.config, [80000])[0])}
    for tag, kw in (("plain", {}), ("attentions", dict(output_attentions=True)),
                    ("attentions_fp32", dict(output_attentions=True, attentions_dtype=torch.float32))):
        r[tag + "_us"] = round(timed_us(lambda: v.forward_infer(audio, **kw), iters, warm=3), 1)
    res["wav2vec2_base_B8_5s_bf16"] = r
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_attn_probs.json"))
    ap.add_argument("--iters", type=int, default=30)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "host": socket.gethostname(), "iters": args.iters,
           "timing": "HIP events around `iters` back-to-back launches (4 x iters for the small shapes) after 5 warm-up launches",
           "kernels": [one_shape(dev, *s, args.iters) for s in SHAPES]}
    res["forward_infer"] = models(dev, max(5, args.iters // 3))
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
