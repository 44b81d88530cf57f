"""Does the alignment of the row stride limit tmi_attn_probs?  The encoder shape 8x12x1500x1500, the same kernel writing rows
at a stride of 1500 (the natural one: 6000 / 3000 bytes, no multiple of a 128-byte line), 1504 and 1536 elements, fp32 and
bf16, from a 128-byte aligned base.  Prints one JSON list and writes it to --out (default
profiles/r11_attn_probs_row_stride.json).

usage: python tools/attn_probs_stride_probe.py [--out PATH]"""
import argparse
import json
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch
import tethys_speech_amd  # noqa
from tethys_speech_amd import ops
from attn_probs_bench import timed_us

dev = torch.device("cuda:0")
B, H, T = 8, 12, 1500
d = H * 64
g = torch.Generator(device=dev).manual_seed(1)
q = (torch.randn(B * T, d, device=dev, generator=g) * 0.125).to(torch.bfloat16)
kv = torch.randn(B * T, 2 * d, device=dev, generator=g).to(torch.bfloat16)
o = torch.empty(B * T, d, dtype=torch.bfloat16, device=dev)
stats = torch.empty(B, H, T, 2, dtype=torch.float32, device=dev)
qm, km, vm, om = (q, 0, T * d, d), (kv, 0, T * 2 * d, 2 * d), (kv, d, T * 2 * d, 2 * d), (o, 0, T * d, d)
ops.attn_fwd(qm, km, vm, om, stats, B, H, T, T, 0)
res = []
for dtype in (torch.float32, torch.bfloat16):
    for sq in (1500, 1504, 1536):
        flat = torch.empty(B * H * T * sq + 64, dtype=dtype, device=dev)
        off = (-flat.data_ptr() // flat.element_size()) % 64  # a 128-byte aligned base (256 for fp32)
        out = torch.as_strided(flat, (B, H, T, T), (H * T * sq, T * sq, sq, 1), off)
        t = timed_us(lambda: ops.attn_probs(qm, km, stats, out, B, H, T, T, 0), 30)
        res.append({"dtype": str(dtype), "p_sq": sq, "kernel_us": round(t, 1)})
        del out, flat
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_attn_probs_row_stride.json"))
args = ap.parse_args()
print(json.dumps(res))
with open(args.out, "w") as f:
    f.write(json.dumps(res, indent=1) + "\n")
