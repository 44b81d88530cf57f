"""SpecAugment on the CTC probe, measured: tmi_spec_masks (csrc/spec_augment.hip) alone, the plain and the mixed head step with
and without the masks fused into the head kernels, and the unfused alternative.  Writes ONE JSON document (default
profiles/r28_spec_augment.json) and prints it.

The shapes of profiles/r26_ctc_head.json and profiles/r27_layer_mix.json - H 768, V 32, K 13, bf16 features, dropout 0.1,
"mean", at (N 8, T 249, L 40), (N 8, T 1499, L 200) and (N 32, T 249, L 40) - with a time mask 0.05 / 10 and a feature mask
0.05 / 10.  Per shape, all in the same rounds:
  - tmi_spec_masks alone (both masks and the counts, one launch);
  - the plain head step of tools/ctc_head_bench.py and the same step with the masks: one tmi_spec_masks launch, then
    tmi_ctc_head_fwd_m / tmi_ctc_head_bwd_m;
  - the mixed head step of tools/layer_mix_bench.py and the same with the masks (tmi_layer_mix_bwd_m as well);
  - the unfused alternative: tmi_spec_masks, tmi_span_mask_apply of the bf16 features into a copy, then the plain step on the
    copy; behind a mix the copy is of the fp32 ``mixed`` buffer (the K layers are never copied), and tmi_layer_mix_bwd - which
    reads the layers, not ``mixed`` - then still needs its masked form, so the unfused mixed step saves nothing there;
  - tmi_span_mask_apply alone on the bf16 features.

HIP events around back-to-back calls after a warm-up of every shape, five rounds alternating the candidates; the median of
the five, and the rounds are kept so that the spread can be read next to every difference.  No threshold: nothing in the
tests depends on these numbers, and bench.py stays as it is.

usage: python tools/spec_augment_bench.py [--out profiles/r28_spec_augment.json] [--iters 40]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402
import tethys_speech_amd  # noqa: E402,F401
from tethys_speech_amd import ops  # noqa: E402
import ctc_head_bench as HB  # noqa: E402
import layer_mix_bench as MB  # noqa: E402

H, V, K = MB.H, MB.V, MB.K
TIME, FEAT = (0.05, 10), (0.05, 10)
ROUNDS = 5


class MaskedHead(MB.MixedHead):
    def __init__(self, dev, N, T, L):
        super().__init__(dev, N, T, L)
        i32 = dict(dtype=torch.int32, device=dev)
        self.tb, self.fb = torch.zeros(N, ops.spec_masks_words(T), **i32), torch.zeros(N, ops.spec_masks_words(H), **i32)
        self.counts = torch.zeros(N, 2, **i32)
        self.x_copy, self.mixed_copy = torch.zeros_like(self.x), torch.zeros_like(self.mixed)

    def masks(self):
        ops.spec_masks(self.N, self.T, H, self.tb, self.fb, self.counts, TIME[0], TIME[1], FEAT[0], FEAT[1], seed=self.step + 77)

    def apply(self):
        ops.span_mask_apply(self.x, self.x_copy, self.tb, self.fb)

    def _head(self, x, tb, fb):
        ops.ctc_head_fwd(x, self.W, self.b, self.fl, self.logp, p=self.drop, seed=self.step, time_bits=tb, feat_bits=fb)
        self.post()
        ops.ctc_head_bwd(x, self.fl, self.ll, self.grad, self.nll, self.bad, self.gW, self.gb, self.loss, self.nbad, self.ws, self.L,
                         p=self.drop, seed=self.step, reduction="mean", time_bits=tb, feat_bits=fb)

    def _adam(self, mix):
        ops.adam_step(self.p, self.g, self.m, self.v, self.n, 1e-3, 0.9, 0.999, 1e-7, self.step)
        if mix:
            ops.adam_step(self.mp, self.mg, self.mm, self.mv, 16, 1e-3, 0.9, 0.999, 1e-7, self.step)

    def _mix_bwd(self, tb, fb):
        ops.layer_mix_bwd(self.layers, self.mp, self.fl, self.ll, self.grad, self.bad, self.W, self.mg, self.mix_ws, self.L,
                          p=self.drop, seed=self.step, reduction="mean", time_bits=tb, feat_bits=fb)

    def masked_step(self):          # fused: the plain step + one launch
        self.step += 1
        self.masks()
        self._head(self.x, self.tb, self.fb)
        self._adam(False)

    def unfused_step(self):         # a masked bf16 copy, then the plain step on it
        self.step += 1
        self.masks()
        self.apply()
        self._head(self.x_copy, None, None)
        self._adam(False)

    def masked_mixed_step(self):
        self.step += 1
        self.masks()
        self.mix_fwd()
        self._head(self.mixed, self.tb, self.fb)
        self._mix_bwd(self.tb, self.fb)
        self._adam(True)

    def unfused_mixed_step(self):   # a masked fp32 copy of `mixed`; the mix backward keeps its masked form
        self.step += 1
        self.masks()
        self.mix_fwd()
        ops.span_mask_apply(self.mixed, self.mixed_copy, self.tb, self.fb)
        self._head(self.mixed_copy, None, None)
        self._mix_bwd(self.tb, self.fb)
        self._adam(True)


def spread(rep):
    return {k: {"min": min(v), "max": max(v)} for k, v in rep.items()}


def shape(dev, N, T, L, iters):
    hd = MaskedHead(dev, N, T, L)
    for fn in (hd.train_step, hd.mixed_step, hd.masked_step, hd.unfused_step, hd.masked_mixed_step, hd.unfused_mixed_step):
        fn()
    torch.cuda.synchronize()
    frac = hd.counts.double().sum(0).cpu() / torch.tensor([N * T, N * H], dtype=torch.float64)
    med, rep = HB.rounds({"spec_masks": hd.masks, "span_mask_apply": hd.apply, "plain_step": hd.train_step, "masked_step": hd.masked_step,
                          "unfused_step": hd.unfused_step, "mixed_step": hd.mixed_step, "masked_mixed_step": hd.masked_mixed_step,
                          "unfused_mixed_step": hd.unfused_mixed_step}, iters, ROUNDS)
    return {"N": N, "T": T, "L": L, "H": H, "V": V, "K": K, "masked_frame_fraction": round(float(frac[0]), 4),
            "masked_column_fraction": round(float(frac[1]), 4), "spec_masks_us": med["spec_masks"],
            "span_mask_apply_bf16_us": med["span_mask_apply"], "plain_head_step_us": med["plain_step"],
            "masked_head_step_us": med["masked_step"], "unfused_head_step_us": med["unfused_step"],
            "masked_minus_plain_us": round(med["masked_step"] - med["plain_step"], 1),
            "unfused_minus_masked_us": round(med["unfused_step"] - med["masked_step"], 1),
            "mixed_head_step_us": med["mixed_step"], "masked_mixed_head_step_us": med["masked_mixed_step"],
            "unfused_mixed_head_step_us": med["unfused_mixed_step"],
            "masked_mixed_minus_mixed_us": round(med["masked_mixed_step"] - med["mixed_step"], 1),
            "unfused_mixed_minus_masked_mixed_us": round(med["unfused_mixed_step"] - med["masked_mixed_step"], 1),
            "spread_us": spread(rep), "rounds_us": rep}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r28_spec_augment.json"))
    ap.add_argument("--iters", type=int, default=40)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "rounds": ROUNDS,
           "masks": {"time": {"prob": TIME[0], "length": TIME[1]}, "feature": {"prob": FEAT[0], "length": FEAT[1]}},
           "timing": "HIP events around `iters` back-to-back calls after 5 warm-up calls of the same shape, five rounds alternating "
                     "the candidates; the median of the five, every round kept, min and max of the rounds under spread_us",
           "measured_against": "the plain and the mixed head step without masks, and the unfused alternative (tmi_span_mask_apply "
                               "into a copy, then the plain kernels on the copy), all timed in this same run",
           "shapes": [shape(dev, N, T, L, args.iters) for N, T, L in ((8, 249, 40), (8, 1499, 200), (32, 249, 40))]}
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
