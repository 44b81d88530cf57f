"""The CTC head on cached features, measured: tmi_ctc_head_fwd / tmi_ctc_head_bwd (csrc/ctc_head.hip), tmi_ctc_posteriors
between them, and the whole head step.  Writes ONE JSON document (default profiles/r26_ctc_head.json) and prints it.

H 768, V 32, bf16 features, dropout 0.1, "mean", at (N 8, T 249, L 40), (N 8, T 1499, L 200) and (N 32, T 249, L 40): each new
kernel, tmi_ctc_posteriors, and one whole head step (forward + posteriors + backward + tmi_adam_step over the head) next to
the torch composite timed IN THE SAME PROCESS on the same numbers: ``F.dropout``, ``F.linear``, ``log_softmax``,
``F.ctc_loss(reduction="mean", zero_infinity=True)``, autograd, ``torch.optim.Adam``.  Also the largest difference between
the two weight gradients without dropout (the composite draws another mask), relative to the largest gradient entry.

HIP events around back-to-back calls after a warm-up of every shape, three rounds alternating the candidates, the median of
the three; the rounds are kept.  No threshold: nothing in the tests depends on these numbers, and bench.py stays as it is.

usage: python tools/ctc_head_bench.py [--out profiles/r26_ctc_head.json] [--iters 40]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import tethys_speech_amd  # noqa: E402,F401
from tethys_speech_amd import ops  # noqa: E402

H, V = 768, 32
F = torch.nn.functional


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


def rounds(cands, iters, n=3):
    """{name: fn} -> ({name: median us}, {name: [us per round]}), the candidates alternating inside every round."""
    t = {k: [] for k in cands}
    for _ in range(n):
        for k, fn in cands.items():
            t[k].append(timed_us(fn, iters))
    return {k: round(float(np.median(v)), 1) for k, v in t.items()}, {k: [round(x, 1) for x in v] for k, v in t.items()}


class Head:
    """The head's parameters as one flat arena (p, g, m, v), the kernels' buffers, and the torch composite on copies."""

    def __init__(self, dev, N, T, L, seed=0):
        g = torch.Generator(device=dev).manual_seed(seed + N + T)
        f32, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
        self.N, self.T, self.L = N, T, L
        self.n = H * V + V
        self.p, self.g, self.m, self.v = (torch.zeros(self.n, **f32) for _ in range(4))
        self.W, self.b = self.p[:H * V].view(H, V), self.p[H * V:]
        self.gW, self.gb = self.g[:H * V].view(H, V), self.g[H * V:]
        self.W.copy_((torch.rand(H, V, generator=g, **f32) * 2 - 1) * (6.0 / (H + V)) ** 0.5)
        self.x = (torch.randn(N, T, H, generator=g, **f32) * 0.5).to(torch.bfloat16)
        self.fl = torch.randint(max(2 * L + 1, (3 * T) // 4), T + 1, (N,), generator=g, device=dev).to(torch.int32)
        self.fl[0] = T
        self.ll = torch.randint(L // 2, L + 1, (N,), generator=g, device=dev).to(torch.int32)
        self.lab = torch.randint(1, V, (N, L), generator=g, device=dev).to(torch.int32)
        self.logp, self.grad, self.occ = (torch.zeros(N, T, V, **f32) for _ in range(3))
        self.gamma = torch.zeros(N, T, 2 * L + 1, **f32)
        self.tf, self.tc = torch.zeros(N, L, **f32), torch.zeros(N, L, **f32)
        self.nll, self.bad = torch.zeros(N, **f32), torch.zeros(N, **i32)
        self.loss, self.nbad = torch.zeros(1, **f32), torch.zeros(1, **i32)
        self.ws = torch.empty(ops.ctc_head_workspace_elems(N, T, H, V), **f32)
        self.step, self.drop = 0, 0.1
        # the composite
        self.tw = [self.W.clone().requires_grad_(True), self.b.clone().requires_grad_(True)]
        self.opt = torch.optim.Adam(self.tw, lr=1e-3, eps=1e-7)
        self.tx = self.x.float()
        self.tlab, self.tfl, self.tll = self.lab.long(), self.fl.long(), self.ll.long()

    def fwd(self):
        ops.ctc_head_fwd(self.x, self.W, self.b, self.fl, self.logp, p=self.drop, seed=self.step)

    def post(self):
        ops.ctc_posteriors(self.logp, self.lab, self.ll, self.fl, 0, self.nll, self.bad, self.gamma, self.occ, self.tf, self.tc,
                           self.grad, True)

    def bwd(self):
        ops.ctc_head_bwd(self.x, self.fl, self.ll, self.grad, self.nll, self.bad, self.gW, self.gb, self.loss, self.nbad, self.ws,
                         self.L, p=self.drop, seed=self.step, reduction="mean")

    def train_step(self):
        self.step += 1
        self.fwd()
        self.post()
        self.bwd()
        ops.adam_step(self.p, self.g, self.m, self.v, self.n, 1e-3, 0.9, 0.999, 1e-7, self.step)

    def torch_loss(self):
        Wt, bt = self.tw
        lp = torch.log_softmax(F.linear(F.dropout(self.tx, self.drop, training=self.drop > 0), Wt.t(), bt), dim=2)
        return F.ctc_loss(lp.transpose(0, 1), self.tlab, self.tfl, self.tll, blank=0, reduction="mean", zero_infinity=True)

    def torch_step(self):
        self.opt.zero_grad(set_to_none=True)
        self.torch_loss().backward()
        self.opt.step()

    def gradient_difference(self):
        """max |gW - autograd's| / max |autograd's| at dropout 0, from the same parameters."""
        drop, self.drop = self.drop, 0.0
        try:
            self.tw[0].data.copy_(self.W)
            self.tw[1].data.copy_(self.b)
            self.fwd()
            self.post()
            self.bwd()
            self.opt.zero_grad(set_to_none=True)
            loss = self.torch_loss()
            loss.backward()
            ref = self.tw[0].grad
            return {"max_abs_gW_difference": float((self.gW - ref).abs().max()), "max_abs_gW": float(ref.abs().max()),
                    "max_abs_gb_difference": float((self.gb - self.tw[1].grad).abs().max()),
                    "loss": float(self.loss), "torch_loss": float(loss.detach())}
        finally:
            self.drop = drop


def shape(dev, N, T, L, iters):
    hd = Head(dev, N, T, L)
    diff = hd.gradient_difference()
    hd.train_step()
    med, rep = rounds({"fwd": hd.fwd, "posteriors": hd.post, "bwd": hd.bwd, "step": hd.train_step, "torch_step": hd.torch_step}, iters)
    return {"N": N, "T": T, "L": L, "H": H, "V": V, "ctc_head_fwd_us": med["fwd"], "ctc_posteriors_us": med["posteriors"],
            "ctc_head_bwd_us": med["bwd"], "head_step_us": med["step"], "torch_composite_step_us": med["torch_step"],
            "step_over_torch": round(med["step"] / med["torch_step"], 2), "gradients": diff, "rounds_us": rep}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r26_ctc_head.json"))
    ap.add_argument("--iters", type=int, default=40)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "iters": args.iters,
           "timing": "HIP events around `iters` back-to-back calls after 5 warm-up calls of the same shape, three rounds "
                     "alternating the candidates; the median of the three, the rounds kept",
           "measured_against": "the torch composite (F.dropout, F.linear, log_softmax, F.ctc_loss(mean, zero_infinity), autograd, "
                               "torch.optim.Adam) on fp32 copies of the same features, timed in this same run",
           "shapes": [shape(dev, N, T, L, args.iters) for N, T, L in ((8, 249, 40), (8, 1499, 200), (32, 249, 40))]}
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
