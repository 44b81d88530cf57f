"""The learned weighted sum over layers in front of the CTC head, measured: tmi_layer_mix_fwd / tmi_layer_mix_bwd
(csrc/layer_mix.hip) alone, and the mixed head step.  Writes ONE JSON document (default profiles/r27_layer_mix.json) and
prints it.

The shapes of profiles/r26_ctc_head.json - H 768, V 32, bf16 layers, dropout 0.1, "mean", at (N 8, T 249, L 40), (N 8,
T 1499, L 200) and (N 32, T 249, L 40) - with K 13 layers stacked [K, N, T, H].  Per shape:
  - each kernel alone with the bytes it moves (the live rows' K layers read, ``mixed`` written; the backward reads the layers,
    ``grad`` and W per tile), the GB/s that makes, and a plain device copy (tmi_memcpy_async) of the same byte count - half
    read, half written - timed in the same rounds;
  - the mixed head step (mix, head forward, posteriors, head backward, mix backward, Adam over the head, Adam over the mix)
    next to the plain head step of tools/ctc_head_bench.py on the last layer, in the same rounds;
  - the mixed head step next to the torch composite in the same rounds: softmax weights, ``einsum`` over the stacked layers,
    then ctc_head_bench's composite (dropout, linear, log_softmax, ctc_loss, autograd, torch.optim.Adam over W, b and a);
  - the cost of the fp32 ``mixed`` round trip the unfused design pays: its bytes (one write, two reads: head forward and head
    backward) and what they take at the copy's measured rate.

HIP events around back-to-back calls after a warm-up of every shape, three rounds alternating the candidates, the median of
the three; the rounds are kept (the method of tools/ctc_head_bench.py).  No threshold: nothing in the tests depends on these
numbers, and bench.py stays as it is.

usage: python tools/layer_mix_bench.py [--out profiles/r27_layer_mix.json] [--iters 40]"""
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

H, V, K = HB.H, HB.V, 13
F = torch.nn.functional


class MixedHead(HB.Head):
    """ctc_head_bench's head on the LAST of K stacked layers, and the same head behind a layer mix over all of them."""

    def __init__(self, dev, N, T, L):
        super().__init__(dev, N, T, L)
        g = torch.Generator(device=dev).manual_seed(7 + N + T)
        f32 = dict(dtype=torch.float32, device=dev)
        self.layers = (torch.randn(K, N, T, H, generator=g, **f32) * 0.5).to(torch.bfloat16)
        self.layers[-1].copy_(self.x)
        self.mp, self.mg, self.mm, self.mv = (torch.zeros(16, **f32) for _ in range(4))
        self.mixed = torch.zeros(N, T, H, **f32)
        self.mix_ws = torch.empty(ops.layer_mix_workspace_elems(N, T, H, V, K), **f32)
        self.mstep = 0
        self.rows = int(self.fl.sum())
        # the composite: the head's parameters and the logits
        self.ta = torch.zeros(K, **f32).requires_grad_(True)
        self.mopt = torch.optim.Adam(self.tw + [self.ta], lr=1e-3, eps=1e-7)
        self.tlayers = self.layers.float()

    def mix_fwd(self):
        ops.layer_mix_fwd(self.layers, self.mp, self.fl, self.mixed)

    def mix_bwd(self):
        ops.layer_mix_bwd(self.layers, self.mp, self.fl, self.ll, self.grad, self.bad, self.W, self.mg, self.mix_ws, self.L,
                          p=self.drop, seed=self.mstep, reduction="mean")

    def mixed_step(self):
        self.mstep += 1
        self.mix_fwd()
        ops.ctc_head_fwd(self.mixed, self.W, self.b, self.fl, self.logp, p=self.drop, seed=self.mstep)
        self.post()
        ops.ctc_head_bwd(self.mixed, self.fl, self.ll, self.grad, self.nll, self.bad, self.gW, self.gb, self.loss, self.nbad, self.ws,
                         self.L, p=self.drop, seed=self.mstep, reduction="mean")
        self.mix_bwd()
        ops.adam_step(self.p, self.g, self.m, self.v, self.n, 1e-3, 0.9, 0.999, 1e-7, self.mstep)
        ops.adam_step(self.mp, self.mg, self.mm, self.mv, 16, 1e-3, 0.9, 0.999, 1e-7, self.mstep)

    def torch_mixed_step(self):
        self.mopt.zero_grad(set_to_none=True)
        Wt, bt = self.tw
        mixed = torch.einsum("k,knth->nth", torch.softmax(self.ta, 0), self.tlayers)
        lp = torch.log_softmax(F.linear(F.dropout(mixed, self.drop, training=True), Wt.t(), bt), dim=2)
        F.ctc_loss(lp.transpose(0, 1), self.tlab, self.tfl, self.tll, blank=0, reduction="mean", zero_infinity=True).backward()
        self.mopt.step()

    def copier(self, nbytes):
        n = max(8, nbytes // 2 // 4)
        src, dst = torch.zeros(n, dtype=torch.float32, device=self.x.device), torch.zeros(n, dtype=torch.float32, device=self.x.device)
        return lambda: ops.copy(dst, src)


def shape(dev, N, T, L, iters):
    hd = MixedHead(dev, N, T, L)
    hd.train_step()
    hd.mixed_step()
    rows = hd.rows
    fwd_bytes = K * rows * H * 2 + rows * H * 4
    tiles = ops.layer_mix_workspace_elems(N, T, H, V, K) // K
    bwd_bytes = K * rows * H * 2 + rows * V * 4 + tiles * H * V * 4
    trip_bytes = 3 * rows * H * 4
    med, rep = HB.rounds({"mix_fwd": hd.mix_fwd, "copy_fwd_bytes": hd.copier(fwd_bytes), "mix_bwd": hd.mix_bwd,
                          "copy_bwd_bytes": hd.copier(bwd_bytes), "copy_round_trip_bytes": hd.copier(trip_bytes),
                          "mixed_step": hd.mixed_step, "plain_step": hd.train_step, "torch_mixed_step": hd.torch_mixed_step}, iters)
    gbs = lambda nbytes, us: round(nbytes / us * 1e-3, 1)
    return {"N": N, "T": T, "L": L, "H": H, "V": V, "K": K, "live_rows": rows, "bwd_tiles": tiles,
            "layer_mix_fwd": {"us": med["mix_fwd"], "bytes": fwd_bytes, "GBps": gbs(fwd_bytes, med["mix_fwd"]),
                              "copy_same_bytes_us": med["copy_fwd_bytes"], "copy_GBps": gbs(fwd_bytes, med["copy_fwd_bytes"])},
            "layer_mix_bwd": {"us": med["mix_bwd"], "bytes": bwd_bytes, "GBps": gbs(bwd_bytes, med["mix_bwd"]),
                              "copy_same_bytes_us": med["copy_bwd_bytes"], "copy_GBps": gbs(bwd_bytes, med["copy_bwd_bytes"])},
            "mixed_round_trip": {"bytes": trip_bytes, "copy_same_bytes_us": med["copy_round_trip_bytes"],
                                 "share_of_mixed_step": round(med["copy_round_trip_bytes"] / med["mixed_step"], 3)},
            "mixed_head_step_us": med["mixed_step"], "plain_head_step_us": med["plain_step"],
            "torch_composite_mixed_step_us": med["torch_mixed_step"],
            "mixed_over_plain": round(med["mixed_step"] / med["plain_step"], 2),
            "mixed_over_torch": round(med["mixed_step"] / med["torch_mixed_step"], 2), "rounds_us": rep}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r27_layer_mix.json"))
    ap.add_argument("--iters", type=int, default=40)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "iters": args.iters,
           "timing": "HIP events around `iters` back-to-back calls after 5 warm-up calls of the same shape, three rounds "
                     "alternating the candidates; the median of the three, the rounds kept",
           "measured_against": "a device copy (tmi_memcpy_async) of the same byte count, the plain head step on the last layer, and "
                               "the torch composite (softmax, einsum over the stacked layers, F.dropout, F.linear, log_softmax, "
                               "F.ctc_loss(mean, zero_infinity), autograd, torch.optim.Adam) on fp32 copies of the same layers, all "
                               "timed in this same run",
           "shapes": [shape(dev, N, T, L, args.iters) for N, T, L in ((8, 249, 40), (8, 1499, 200), (32, 249, 40))]}
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
