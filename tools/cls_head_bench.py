"""The classification head, measured: tmi_cls_head_fwd / tmi_cls_head_bwd (csrc/cls_head.hip) and
``Wav2Vec2ForSequenceClassification.evaluate``.  Writes ONE JSON document (default profiles/r25_cls_head.json) and prints it.

Kernels, H 768, P 256, C 2 and 64, N 8 / 256 / 4096 rows: the forward call (dropout 0.1, labels, every output) and one whole
head step (forward + backward + tmi_adam_step over the head's parameters) next to the torch composite timed IN THE SAME
PROCESS on the same numbers: ``torch.tanh(x @ Wp + bp)``, dropout, ``@ Wc``, ``log_softmax``, ``nll_loss``, autograd,
``torch.optim.Adam``.  "gwp": the weight gradient of the projection both ways at N 8 and 4096 - inside tmi_cls_head_bwd
(the call timed with H 768 minus the call timed with H 4, where that product is a single tile) and as one exact-fp32
tmi_gemm with transposed strides on the same operands.

Model, base size, bf16, B 8, clips of 2 / 5 / 30 s: ``evaluate`` next to ``forward_infer(pool="mean")`` of the same model.

HIP events around back-to-back calls after a warm-up of every shape, three rounds alternating the candidates, the median of
the three; the rounds are kept.  No threshold: nothing in the tests depends on these numbers, and bench.py stays as it is.

usage: python tools/cls_head_bench.py [--out profiles/r25_cls_head.json] [--iters 60]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import tethys_speech_amd  # noqa: E402,F401
from tethys_speech_amd import ops, wav2vec2  # noqa: E402

H, P = 768, 256


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

    def __init__(self, dev, N, C, h=H, seed=0):
        g = torch.Generator(device=dev).manual_seed(seed + N + C)
        f32 = dict(dtype=torch.float32, device=dev)
        self.N, self.C, self.h = N, C, h
        sizes = [h * P, P, P * C, C]
        offs = np.concatenate([[0], np.cumsum([(s + 7) // 8 * 8 for s in sizes])])
        self.n = int(offs[-1])
        self.p, self.g, self.m, self.v = (torch.zeros(self.n, **f32) for _ in range(4))
        view = lambda buf, i, shape: buf[int(offs[i]):int(offs[i]) + sizes[i]].view(*shape)
        shapes = [(h, P), (P,), (P, C), (C,)]
        self.W = [view(self.p, i, s) for i, s in enumerate(shapes)]
        self.G = [view(self.g, i, s) for i, s in enumerate(shapes)]
        self.W[0].copy_((torch.rand(h, P, generator=g, **f32) * 2 - 1) * (6.0 / (h + P)) ** 0.5)
        self.W[2].copy_((torch.rand(P, C, generator=g, **f32) * 2 - 1) * (6.0 / (P + C)) ** 0.5)
        self.x = torch.randn(N, h, generator=g, **f32) * 0.5
        self.labels = torch.randint(0, C, (N,), generator=g, device=dev).to(torch.int32)
        self.logits, self.logp, self.z = torch.empty(N, C, **f32), torch.empty(N, C, **f32), torch.empty(N, P, **f32)
        self.pred, self.rank = torch.empty(N, dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.int32, device=dev)
        self.nll, self.loss = torch.empty(N, **f32), torch.empty(1, **f32)
        self.ws = torch.empty(ops.cls_head_workspace_elems(N, h, P, C), **f32)
        self.step = 0
        # the composite
        self.tw = [w.clone().requires_grad_(True) for w in self.W]
        self.opt = torch.optim.Adam(self.tw, lr=1e-3, eps=1e-7)
        self.tlab = self.labels.long()

    def fwd(self):
        ops.cls_head_fwd(self.x, *self.W, self.logits, self.pred, labels=self.labels, p=0.1, seed=self.step, z=self.z,
                         log_probs=self.logp, nll=self.nll, label_rank=self.rank)

    def bwd(self):
        ops.cls_head_bwd(self.x, self.W[2], self.labels, self.z, self.logp, *self.G, self.loss, self.ws, p=0.1, seed=self.step)

    def train_step(self):
        self.step += 1
        self.fwd()
        self.bwd()
        ops.adam_step(self.p, self.g, self.m, self.v, self.n, 1e-3, 0.9, 0.999, 1e-7, self.step)

    def torch_forward(self):
        Wp, bp, Wc, bc = self.tw
        y = torch.nn.functional.dropout(torch.tanh(self.x @ Wp + bp), 0.1, training=True)
        lp = torch.log_softmax(y @ Wc + bc, dim=1)
        return lp, torch.nn.functional.nll_loss(lp, self.tlab)

    def torch_fwd(self):
        with torch.no_grad():
            lp, _ = self.torch_forward()
            nll = -lp.gather(1, self.tlab[:, None])
            return lp.argmax(dim=1), nll

    def torch_step(self):
        self.opt.zero_grad(set_to_none=True)
        _, loss = self.torch_forward()
        loss.backward()
        self.opt.step()


def kernels(dev, N, C, iters):
    hd = Head(dev, N, C)
    med, rep = rounds({"fwd": hd.fwd, "torch_fwd": hd.torch_fwd, "step": hd.train_step, "torch_step": hd.torch_step}, iters)
    return {"N": N, "H": H, "P": P, "C": C, "cls_head_fwd_us": med["fwd"], "torch_composite_fwd_us": med["torch_fwd"],
            "head_step_us": med["step"], "torch_composite_step_us": med["torch_step"],
            "fwd_over_torch": round(med["fwd"] / med["torch_fwd"], 2), "step_over_torch": round(med["step"] / med["torch_step"], 2),
            "rounds_us": rep}


def gwp(dev, N, iters, C=2):
    """gWp inside tmi_cls_head_bwd (the call at H 768 minus the call at H 4) and as one fp32 tmi_gemm: gWp[h][c] = sum_r
    x[r][h] dpre[r][c], A = x read with a_sm = 1, a_sk = H."""
    big, small = Head(dev, N, C), Head(dev, N, C, h=4)
    for hd in (big, small):
        hd.fwd()
    big.bwd()
    dpre = big.ws[64:64 + N * P].view(N, P)
    out = torch.empty(H, P, dtype=torch.float32, device=dev)
    gemm = lambda: ops.gemm(big.x, dpre, out, H, P, N, 1, H, P, 1, P)
    gemm()
    torch.cuda.synchronize()
    err = float((out - big.G[0]).abs().max())
    med, rep = rounds({"bwd_h768": big.bwd, "bwd_h4": small.bwd, "gemm": gemm}, iters)
    return {"N": N, "H": H, "P": P, "C": C, "cls_head_bwd_us": med["bwd_h768"], "cls_head_bwd_h4_us": med["bwd_h4"],
            "gwp_in_kernel_us": round(med["bwd_h768"] - med["bwd_h4"], 1), "gwp_tmi_gemm_us": med["gemm"],
            "max_abs_gemm_minus_kernel": err, "rounds_us": rep}


def model(dev, iters):
    m = wav2vec2.create_classification_model("base", num_labels=8, device=dev, precision="bf16")
    B, res = 8, []
    labels = torch.arange(B) % 8
    for seconds in (2, 5, 30):
        audio = (torch.randn(B, seconds * 16000, generator=torch.Generator().manual_seed(seconds)) * 0.1).to(dev)
        base = lambda: wav2vec2.Wav2Vec2ForPreTraining.forward_infer(m, audio, pool="mean")
        n = max(3, iters // (4 if seconds < 30 else 12))
        med, rep = rounds({"forward_infer_pool": base, "evaluate": lambda: m.evaluate(audio, labels, top_k=(1, 3))}, n)
        res.append({"B": B, "seconds": seconds, "frames": wav2vec2.frame_lengths(m.config, [seconds * 16000])[0],
                    "forward_infer_pool_mean_us": med["forward_infer_pool"], "evaluate_us": med["evaluate"],
                    "evaluate_minus_forward_infer_us": round(med["evaluate"] - med["forward_infer_pool"], 1), "rounds_us": rep})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r25_cls_head.json"))
    ap.add_argument("--iters", type=int, default=60)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "iters": args.iters,
           "timing": "HIP events around `iters` back-to-back calls after 5 warm-up calls of the same shape, three rounds "
                     "alternating the candidates; the median of the three, the rounds kept (evaluate includes its one "
                     "read-back of the sums)",
           "measured_against": "the torch composite (tanh(x @ Wp + bp), dropout, @ Wc, log_softmax, nll_loss, autograd, "
                               "torch.optim.Adam) and forward_infer(pool='mean'), timed in this same run",
           "kernels": [kernels(dev, N, C, args.iters) for C in (2, 64) for N in (8, 256, 4096)],
           "gwp": [gwp(dev, N, args.iters) for N in (8, 4096)]}
    res["wav2vec2_base_bf16"] = model(dev, args.iters)
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
