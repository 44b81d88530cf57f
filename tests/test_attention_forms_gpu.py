"""tmi_attn_fwd / tmi_attn_bwd (csrc/attention.hip) the way the step calls them, at the lengths inference uses, on inputs
that are hard for a streaming softmax, and with their argument checks.

Ground truth: ``test_kernels_gpu._attn_ref`` - bf16-rounded inputs, evaluated in float64 on the CPU - with ``score_scale``
applied to q.k^T before the mask, one batch item at a time.

No tolerance is written down here.  Beside the reference stands ``restate``: the same operation in float64 with the bf16
roundings the kernels perform (P before P.V and P^T.dO, dS before the dQ and dK products, o / dq / dk / dv on store, the keep
bits and keep_scale where the kernels apply them).  The bound of a case and metric is TWICE the restatement's own error
against float64 on that case and metric, computed at test time - the factor of tests/_margins.py; it covers the kernels'
summation order and their fp32 exp2.  tests/test_attention_restatement_cpu.py keeps the restatement itself honest.

Metrics: o and dv per row (row's max error / row's max |ref|, worst row) and over the whole tensor; dq and dk per
(batch, head) and over the whole tensor (their rows can have a near-zero gradient, where a per-row ratio means nothing even
for the restatement).  Where the reference is exactly zero the kernel's output must be exactly zero.
Every comparison is reported through ``_margins.within`` (profiles/r07_attention_margins.json)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from _margins import within  # noqa: E402
from test_kernels_gpu import _attn_ref, _decode_dropmask, rnd  # noqa: E402

HD = 64
BF = torch.bfloat16
TMI_ERR_INVALID = -1  # include/tethys_mi.h


def _mods():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import _lib, ops
    return ops, _lib


def bf(t):
    """Round to bf16, keep computing in float64."""
    return t.to(BF).double()


# ----------------------------------------------------------------------------- reference and restatement (CPU, float64)
def _scores(q, k, mask_mode, scale):
    """scale * q.k^T with the reference's decoder mask: -1e9 added in fp32 to keys j <= i, which absorbs the score."""
    s = (q @ k.transpose(-1, -2)) * scale
    if mask_mode:
        i = torch.arange(q.shape[-2])
        masked = i[None, :] <= i[:, None]
        s = torch.where(masked, (s.float() + torch.tensor(-1e9, dtype=torch.float32)).double(), s)
    return s


def reference(q, k, v, do, mask_mode, scale, dq_scale, keep, ks, backward=True):
    """float64 ground truth on [H, T, 64] inputs (one batch item): o, and dq * dq_scale / dk / dv for the cotangent ``do``."""
    with torch.enable_grad():
        qr, kr, vr = (t.clone()[None].requires_grad_(backward) for t in (q, k, v))
        o = _attn_ref(qr * scale, kr, vr, mask_mode, None if keep is None else keep[None].double(), ks)
        if not backward:
            return {"o": o[0].detach()}
        o.backward(do[None])
    return {"o": o[0].detach(), "dq": dq_scale * qr.grad[0], "dk": kr.grad[0], "dv": vr.grad[0]}


# The forward kernel does not subtract the row's final maximum before it rounds P: its running maximum is only raised when
# some row of the wave grew by more than 2^8 (LAZY), every key range of the key split has a maximum of its own, and the
# accumulators are rescaled in fp32 afterwards.  So P is rounded at 2^lag times the value a textbook softmax would round,
# lag anywhere in [0, 8]: the row's largest probability is rounded too (with lag 0 it is exactly 1), and a near-uniform row
# straddles a power of two, above which a bf16 step is twice as wide.  Only the fractional part of lag changes a rounding,
# so the restatement is evaluated at these three and its error on a case and metric is the largest of them.  (Added after
# the first GPU run: with lag 0 alone the kernels measured 2.1 - 2.4 x the restatement on 5 of 107 cases, among them the
# near-uniform quiet head and Tq = 1.)
LAGS = (0.0, 1.0 / 3.0, 2.0 / 3.0)


def restate(q, k, v, do, mask_mode, scale, dq_scale, keep, ks, backward=True, lag=0.0):
    """The same operation with the kernels' bf16 rounding points (csrc/attention.hip), everything else in float64.
    forward:  e = 2^lag * exp(s - max); l = sum of the UNROUNDED e, dropped keys included; o = bf16((bf16(e) * keep) . v * ks / l)
    dQ pass:  delta = sum_d dO * o (the stored bf16 o); P = e / l; dS = bf16(P * (dP * keep * ks - delta));
              dq = bf16(dS . k * dq_scale * scale)
    dK/dV:    dv = bf16(bf16(P * keep)^T . dO * ks); dS' = bf16(P * keep * dP - P * delta / ks);
              dk = bf16(dS'^T . q * scale * ks)      (keep_scale goes to the dK store, so dS' is rounded without it)"""
    s = _scores(q, k, mask_mode, scale)
    e = torch.exp(s - s.amax(-1, keepdim=True) + lag * 0.6931471805599453)
    l = e.sum(-1, keepdim=True)
    kp = 1.0 if keep is None else keep.double()
    o = bf(((bf(e) * kp) @ v) * (ks / l))
    if not backward:
        return {"o": o}
    delta = (do * o).sum(-1, keepdim=True)
    p = e / l
    dp = do @ v.transpose(-1, -2)
    dq = bf((bf(p * (dp * kp * ks - delta)) @ k) * (dq_scale * scale))
    pk = p * kp
    dv = bf((bf(pk).transpose(-1, -2) @ do) * ks)
    dk = bf((bf(pk * dp - p * (delta / ks)).transpose(-1, -2) @ q) * (scale * ks))
    return {"o": o, "dq": dq, "dk": dk, "dv": dv}


class Errors:
    """Error of one implementation against the reference, folded over batch items: whole tensor, worst row, worst head."""

    def __init__(self):
        self.rec = {}

    def add(self, name, got, ref):  # [H, T, 64]
        r = self.rec.setdefault(name, {"err": 0.0, "mag": 0.0, "row": 0.0, "head": 0.0, "nonzero_where_ref_is_zero": 0})
        if not bool(ref.count_nonzero()):  # an exactly zero reference tensor (dk when q = 0) admits no error at all
            r["nonzero_where_ref_is_zero"] += int(got.count_nonzero())
            return
        err = (got - ref).abs()
        r["err"], r["mag"] = max(r["err"], float(err.max())), max(r["mag"], float(ref.abs().max()))
        for key, dims in (("row", (-1,)), ("head", (-2, -1))):
            e, m = err.amax(dims), ref.abs().amax(dims)
            nz = m > 0
            if bool(nz.any()):
                r[key] = max(r[key], float((e[nz] / m[nz]).max()))

    def metric(self, name, which):
        r = self.rec[name]
        if which == "whole":
            return r["err"] / r["mag"] if r["mag"] > 0 else None
        return r[which]


METRICS = {"o": ("row", "whole"), "dv": ("row", "whole"), "dq": ("head", "whole"), "dk": ("head", "whole")}


def heads(t, H):  # [T, H*64] -> [H, T, 64] float64
    return t.double().reshape(t.shape[0], H, HD).permute(1, 0, 2)


def compare(tag, got, inp, H, mask_mode, scale, dq_scale, keep, ks, backward=True):
    """``got`` / ``inp``: name -> CPU [B, T, H*64]; keep: [B, H, Tq, Tk] bool or None.  Returns both error records."""
    kern, rests = Errors(), [Errors() for _ in LAGS]
    B = inp["q"].shape[0]
    for b in range(B):
        q, k, v = heads(inp["q"][b], H), heads(inp["k"][b], H), heads(inp["v"][b], H)
        do = heads(inp["do"][b], H) if backward else None
        kp = None if keep is None else torch.from_numpy(keep[b])
        ref = reference(q, k, v, do, mask_mode, scale, dq_scale, kp, ks, backward)
        for name in ref:
            kern.add(name, heads(got[name][b], H), ref[name])
        for lag, rest in zip(LAGS, rests):
            rst = restate(q, k, v, do, mask_mode, scale, dq_scale, kp, ks, backward, lag)
            for name in ref:
                rest.add(name, rst[name], ref[name])
    for name in kern.rec:
        assert kern.rec[name]["nonzero_where_ref_is_zero"] == 0, (tag, name, "the reference is exactly zero there")
        for which in METRICS[name]:
            m = kern.metric(name, which)
            if m is not None:
                within(f"attn-forms {tag} {name} {which}", m, 2.0 * max(rest.metric(name, which) for rest in rests))
    return kern, rests


# ----------------------------------------------------------------------------- canaried buffers
GUARD = 256  # elements in front of and behind every buffer (a multiple of 16 bytes for every dtype used)
PATTERN = {BF: (torch.int16, 0x5AA5), torch.float32: (torch.int32, 0x5AA55AA5), torch.uint8: (torch.uint8, 0xA5)}


class Canaried:
    """``n`` elements inside a larger allocation filled with a fixed bit pattern.  ``own(shape)`` is a bool view of the
    body in which the caller marks what the kernels may write; ``untouched()``: everything else still holds the pattern."""

    def __init__(self, dev, n, dtype):
        self.it, self.pat = PATTERN[dtype]
        self.n = int(n)
        self.flat = torch.full((self.n + 2 * GUARD,), self.pat, dtype=self.it, device=dev).view(dtype)
        self.owned = torch.zeros(self.n + 2 * GUARD, dtype=torch.bool)

    @property
    def body(self):
        return self.flat[GUARD:GUARD + self.n]

    def own(self, *shape):
        return self.owned[GUARD:GUARD + self.n].view(*shape)

    def untouched(self):
        bits = self.flat.view(self.it).cpu()
        return bool((bits[~self.owned] == self.pat).all())


PAD = 3   # rows past Tq / Tk that belong to nobody
CROSS_L, CROSS_I = 3, 1  # cross-attention: k / v of the middle one of three decoder layers in kvc_all [B*T, 2*L*D]


class Case:
    """One attention call in the step's form.
    self  (Tq == Tk): q, k, v = columns 0, D, 2D of a fused [B, T, 3D] buffer; dq, dk, dv the same columns of dqkv.
    cross: q in [B, S, D]; k, v = columns 2iD, (2i+1)D of kvc_all [B*T, 2*L*D]; dq in [B, S, D]; dk, dv the same columns of dkv.
    o and dO are [B, Tq, D] buffers of their own.  Every batch item has PAD rows past its last token (kvc_all: past B*T)."""

    def __init__(self, dev, B, H, Tq, Tk, mask_mode, drop, inp, score_scale=1.0, dq_scale=1.0, seed=0x5EED0001, form=None,
                 layers=CROSS_L, layer=CROSS_I):
        ops, _lib = _mods()
        self.ops, self.lib, self.check = ops, _lib.lib(), _lib.check
        self.dev, self.B, self.H, self.Tq, self.Tk, self.mask, self.drop = dev, B, H, Tq, Tk, mask_mode, drop
        self.scale, self.dq_scale, self.seed, self.inp = score_scale, dq_scale, seed, inp
        self.form = form or ("self" if Tq == Tk else "cross")
        D = self.D = H * HD
        Tqp = Tq + PAD
        self.bufs = {}

        def new(name, n, dtype=BF):
            c = self.bufs[name] = Canaried(dev, n, dtype)
            return c

        if self.form == "self":
            assert Tq == Tk
            qkv, dqkv = new("qkv", B * Tqp * 3 * D), new("dqkv", B * Tqp * 3 * D)
            view = qkv.body.view(B, Tqp, 3 * D)
            for i, name in enumerate("qkv"):
                view[:, :Tq, i * D:(i + 1) * D] = inp[name].to(dev)
            dqkv.own(B, Tqp, 3 * D)[:, :Tq, :] = True
            sb, st = Tqp * 3 * D, 3 * D
            self.Q, self.K, self.V = ((qkv.flat, GUARD + i * D, sb, st) for i in range(3))
            self.DQ, self.DK, self.DV = ((dqkv.flat, GUARD + i * D, sb, st) for i in range(3))
            self.grads = {n: (dqkv, (B, Tqp, 3 * D), i * D, Tq) for i, n in enumerate(("dq", "dk", "dv"))}
        else:
            W = 2 * layers * D
            qb, dqb = new("q", B * Tqp * D), new("dq", B * Tqp * D)
            kvc, dkv = new("kvc_all", (B * Tk + PAD) * W), new("dkv", (B * Tk + PAD) * W)
            qb.body.view(B, Tqp, D)[:, :Tq] = inp["q"].to(dev)
            view = kvc.body.view(B * Tk + PAD, W)
            c0 = 2 * layer * D
            view[:B * Tk, c0:c0 + D] = inp["k"].reshape(B * Tk, D).to(dev)
            view[:B * Tk, c0 + D:c0 + 2 * D] = inp["v"].reshape(B * Tk, D).to(dev)
            dqb.own(B, Tqp, D)[:, :Tq] = True
            dkv.own(B * Tk + PAD, W)[:B * Tk, c0:c0 + 2 * D] = True
            self.Q, self.DQ = (qb.flat, GUARD, Tqp * D, D), (dqb.flat, GUARD, Tqp * D, D)
            self.K, self.V = (kvc.flat, GUARD + c0, Tk * W, W), (kvc.flat, GUARD + c0 + D, Tk * W, W)
            self.DK, self.DV = (dkv.flat, GUARD + c0, Tk * W, W), (dkv.flat, GUARD + c0 + D, Tk * W, W)
            self.grads = {"dq": (dqb, (B, Tqp, D), 0, Tq), "dk": (dkv, (B, Tk, W), c0, Tk), "dv": (dkv, (B, Tk, W), c0 + D, Tk)}
        o = new("o", B * Tqp * D)
        o.own(B, Tqp, D)[:, :Tq] = True
        self.O = (o.flat, GUARD, Tqp * D, D)
        if "do" in inp:
            do = new("do", B * Tqp * D)
            do.body.view(B, Tqp, D)[:, :Tq] = inp["do"].to(dev)
            self.DO = (do.flat, GUARD, Tqp * D, D)
        new("stats", B * H * Tq * 2, torch.float32).owned[GUARD:-GUARD] = True   # the kernels own B*H*Tq*2 floats, no more
        new("delta", B * H * Tq, torch.float32).owned[GUARD:-GUARD] = True
        if drop > 0:
            new("drop_mask", self.lib.tmi_attn_dropmask_bytes(B, H, Tq, Tk), torch.uint8).owned[GUARD:-GUARD] = True
        # the key-split workspace under ops._attn_desc's own gate, sized exactly tmi_attn_workspace_bytes
        if mask_mode == 0 and Tq <= 128 and Tk >= 512:
            new("workspace", self.lib.tmi_attn_workspace_bytes(B, H, Tq), torch.uint8).owned[GUARD:-GUARD] = True
        self.inputs_before = {n: self.bufs[n].flat.clone() for n in ("qkv", "q", "kvc_all", "do") if n in self.bufs}

    def desc(self, score_scale=None):
        d = self.ops._attn_desc(self.Q, self.K, self.V, self.O, self.bufs["stats"].body, self.B, self.H, self.Tq, self.Tk, self.mask,
                                self.scale if score_scale is None else score_scale)
        d.workspace, d.workspace_bytes = None, 0
        if "workspace" in self.bufs:
            d.workspace, d.workspace_bytes = self.bufs["workspace"].body.data_ptr(), self.bufs["workspace"].n
        self.ops._set_dropout(d, self.drop, self.seed, self.bufs["drop_mask"].body if self.drop > 0 else None)
        return d

    def fwd(self, score_scale=None):
        d = self.desc(score_scale)
        self.check(self.lib.tmi_attn_fwd(C.byref(d), self.ops.stream()), "tmi_attn_fwd")
        torch.cuda.synchronize()

    def bwd_desc(self, passes=0, score_scale=None):
        d = self.desc(score_scale)
        for name, field, (t, off, sb, st) in (("d_o", "do", self.DO), ("dq", "dq", self.DQ), ("dk", "dk", self.DK), ("dv", "dv", self.DV)):
            setattr(d, name, t.data_ptr() + off * t.element_size())
            setattr(d, f"{field}_sb", sb)
            setattr(d, f"{field}_st", st)
        d.delta, d.dq_scale, d.bwd_passes = self.bufs["delta"].body.data_ptr(), self.dq_scale, passes
        return d

    def bwd(self, passes=0, score_scale=None):
        d = self.bwd_desc(passes, score_scale)
        self.check(self.lib.tmi_attn_bwd(C.byref(d), self.ops.stream()), "tmi_attn_bwd")
        torch.cuda.synchronize()

    # ---- results
    def out_o(self):
        return self.bufs["o"].body.view(self.B, self.Tq + PAD, self.D)[:, :self.Tq].cpu()

    def out_grad(self, name):
        c, shape, col, T = self.grads[name]
        rows = c.body[:shape[0] * shape[1] * shape[2]].view(*shape)
        return rows[:, :T, col:col + self.D].cpu()

    def keep(self):
        if self.drop <= 0:
            return None, 1.0
        from oracle import dropout as DO
        return _decode_dropmask(self.bufs["drop_mask"].body, self.B, self.H, self.Tq, self.Tk), DO.keep_scale(self.drop)

    def assert_canaries(self):
        for name, c in self.bufs.items():
            if name not in self.inputs_before:
                assert c.untouched(), f"{name}: a kernel wrote outside what it owns"
        for name, before in self.inputs_before.items():
            assert torch.equal(self.bufs[name].flat.view(torch.int16), before.view(torch.int16)), f"{name}: an input changed"

    def run_and_compare(self, tag, backward=True):
        self.fwd()
        keep, ks = self.keep()
        got = {"o": self.out_o()}
        if backward:
            self.bwd()
            got.update({n: self.out_grad(n) for n in ("dq", "dk", "dv")})
        self.assert_canaries()
        return compare(tag, got, self.inp, self.H, self.mask, self.scale if self.scale != 0 else 1.0, self.dq_scale, keep, ks,
                       backward)


def gaussian(B, H, Tq, Tk, seed, q_std=0.35, do_std=1.0):
    D = H * HD
    return {"q": rnd((B, Tq, D), BF, "cpu", seed, q_std), "k": rnd((B, Tk, D), BF, "cpu", seed + 1),
            "v": rnd((B, Tk, D), BF, "cpu", seed + 2), "do": rnd((B, Tq, D), BF, "cpu", seed + 3, do_std)}


# ----------------------------------------------------------------------------- A. the models' call forms, with canaries
# Paths (csrc/attention.hip): pick_ksplit splits the keys when mask 0, Tq <= 128, >= 8 key tiles and a workspace is given;
# pick_grid uses the XCD-aware 1-D grid when B*H % 8 == 0 and there is more than one block per (batch, head); the backward
# is one launch (attn_bwd_small_kernel, plain 3-D grid) when Tq <= 256 and Tk <= 256 and no key split, two passes otherwise.
FORMS = [
    # B*H = 8, 12 query tiles, Tq > 128 so no key split: forward, dQ (12 blocks) and dK/dV (12 blocks) all on the XCD grid
    (2, 4, 1500, 1500, 0, 0.1),
    # B*H = 8, Tq = 200 > 128 so no split: forward / dQ with 2 blocks, dK/dV with 3 (Tk = 333 > 256: two passes), XCD grid
    (8, 1, 200, 333, 0, 0.1),
    # B*H = 8, causal (never split), 3 blocks per pair on the XCD grid, T = 300 > 256: two passes
    (2, 4, 300, 300, 1, 0.0),
    # B*H = 96 but one block per pair: plain 3-D forward grid; T <= 256: the one-launch backward, 1 + 1 blocks
    (8, 12, 99, 99, 0, 0.1),
    # two query blocks: the forward on the XCD grid (gx = 2); the one-launch backward with 2 + 2 blocks on its 3-D grid
    (8, 12, 249, 249, 0, 0.1),
    # cross-attention of the benchmark: Tq <= 128, 24 key tiles, workspace: 4 key ranges (gx = 4, XCD grid) + combine in
    # the forward and the dQ pass; dK/dV 12 blocks on the XCD grid
    (8, 12, 100, 1500, 0, 0.1),
    # Tq = 130 > 128: tmi_attn_workspace_bytes is 0, no split; 2 query blocks (XCD grid), two passes
    (2, 4, 130, 1500, 0, 0.0),
]


@pytest.mark.parametrize("B,H,Tq,Tk,mask,drop", FORMS)
def test_model_call_forms_with_canaries(dev, B, H, Tq, Tk, mask, drop):
    c = Case(dev, B, H, Tq, Tk, mask, drop, gaussian(B, H, Tq, Tk, 700 + Tq), dq_scale=0.5)
    c.run_and_compare(f"A {c.form}({B},{H},{Tq}x{Tk}) mask{mask} drop{drop}")
    if drop > 0:  # the stored bits are the generator's, also through these strides
        from oracle import dropout as DO
        assert (c.keep()[0] == DO.keep_attention(c.seed, B, H, Tq, Tk, drop)).all()


# ----------------------------------------------------------------------------- B. score_scale
# Wav2Vec2's form: q unscaled (std 1), score_scale = 1/sqrt(64), dq_scale = 1.
SCALED = [(8, 12, 99, 99), (8, 12, 249, 249),   # the one-launch backward
          (2, 4, 400, 400),                     # two passes (T > 256), XCD grid
          (2, 2, 100, 1000)]                    # key split (16 key tiles, workspace): c2 in the partials, dq_scale * sscale in the combine


@pytest.mark.parametrize("drop", [0.0, 0.1])
@pytest.mark.parametrize("B,H,Tq,Tk", SCALED)
def test_score_scale(dev, B, H, Tq, Tk, drop):
    c = Case(dev, B, H, Tq, Tk, 0, drop, gaussian(B, H, Tq, Tk, 800 + Tq, q_std=1.0), score_scale=0.125, dq_scale=1.0)
    c.run_and_compare(f"B scale0.125 ({B},{H},{Tq}x{Tk}) drop{drop}")


def _all_outputs(c):
    return [c.out_o(), c.bufs["stats"].body.clone().cpu()] + [c.out_grad(n) for n in ("dq", "dk", "dv")] + \
           [c.bufs["delta"].body.clone().cpu()]


@pytest.mark.parametrize("B,H,Tq,Tk,drop", [(2, 3, 130, 200, 0.1), (2, 2, 100, 1000, 0.0)])
def test_score_scale_zero_means_one(dev, B, H, Tq, Tk, drop):
    inp = gaussian(B, H, Tq, Tk, 820)
    res = []
    for scale in (0.0, 1.0):
        c = Case(dev, B, H, Tq, Tk, 0, drop, inp, score_scale=scale)
        c.fwd()
        c.bwd()
        c.assert_canaries()
        res.append(_all_outputs(c))
    for a, b in zip(*res):
        assert torch.equal(a, b)


@pytest.mark.parametrize("drop", [0.0, 0.1])
def test_scaled_one_launch_backward_equals_the_two_passes(dev, drop):
    B, H, Tq, Tk = 2, 3, 130, 200
    inp = gaussian(B, H, Tq, Tk, 830, q_std=1.0)
    res = []
    for passes in ((0,), (1, 2)):
        c = Case(dev, B, H, Tq, Tk, 0, drop, inp, score_scale=0.125)
        c.fwd()
        for ps in passes:
            c.bwd(ps)
        c.assert_canaries()
        res.append(_all_outputs(c))
    for a, b in zip(*res):
        assert torch.equal(a, b)


# ----------------------------------------------------------------------------- C. decode lengths (forward only)
def _fwd_plain(dev, B, H, Tq, Tk, mask, seed):
    """Forward through ops.attn_fwd (workspace as ops._attn_desc provides it) on the step's buffers without guard zones:
    fused [B, S, 3D] for self-attention, q [B, S, D] against k | v side by side in [B*T, 2D] for cross-attention."""
    ops, _ = _mods()
    D = H * HD
    inp = gaussian(B, H, Tq, Tk, seed)
    if Tq == Tk and mask:
        qkv = torch.cat([inp["q"], inp["k"], inp["v"]], -1).to(dev)
        Q, K, V = ((qkv, i * D, Tq * 3 * D, 3 * D) for i in range(3))
    else:
        q = inp["q"].to(dev)
        kv = torch.cat([inp["k"], inp["v"]], -1).reshape(B * Tk, 2 * D).to(dev)
        Q, K, V = (q, 0, Tq * D, D), (kv, 0, Tk * 2 * D, 2 * D), (kv, D, Tk * 2 * D, 2 * D)
    o = torch.full((B, Tq, D), float("nan"), dtype=BF, device=dev)
    stats = torch.empty((B, H, Tq, 2), dtype=torch.float32, device=dev)
    ops.attn_fwd(Q, K, V, (o, 0, Tq * D, D), stats, B, H, Tq, Tk, mask)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(o).all()) and bool(torch.isfinite(stats[..., 1]).all())
    return inp, o.cpu()


BH = [(1, 12), (8, 12)]  # B*H = 12: plain grid; 96: the XCD grid wherever there is more than one block per pair


@pytest.mark.parametrize("B,H", BH)
@pytest.mark.parametrize("S", [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 448])
def test_decode_self_attention_lengths(dev, B, H, S):
    """generate() re-decodes the prefix: mask_mode 1 at every Tq = Tk = S.  The last row is fully masked: every score is
    absorbed by -1e9, so its probabilities are all equal and o is the average of v with the kernel's rounding points."""
    inp, o = _fwd_plain(dev, B, H, S, S, 1, 900 + S)
    tag = f"C self BH{B * H} S{S}"
    compare(tag, {"o": o}, inp, H, 1, 1.0, 1.0, None, 1.0, backward=False)
    last = {n: t[:, S - 1:] for n, t in inp.items()}
    last["k"], last["v"] = inp["k"], inp["v"]
    # the last row alone, unmasked against q = 0: the same uniform softmax, so the same reference and restatement
    last["q"] = torch.zeros_like(last["q"])
    compare(tag + " masked-row", {"o": o[:, S - 1:]}, last, H, 0, 1.0, 1.0, None, 1.0, backward=False)


@pytest.mark.parametrize("B,H", BH)
@pytest.mark.parametrize("S", [1, 127, 128, 129, 257, 448])
def test_decode_cross_attention_lengths(dev, B, H, S):
    """Tq = S against the encoder's 1500 keys: the key split is on up to S = 128 and off above."""
    inp, o = _fwd_plain(dev, B, H, S, 1500, 0, 950 + S)
    compare(f"C cross BH{B * H} S{S}x1500", {"o": o}, inp, H, 0, 1.0, 1.0, None, 1.0, backward=False)


@pytest.mark.parametrize("B,H", BH)
@pytest.mark.parametrize("Tk", [511, 512, 513, 640, 832, 1088])
def test_key_split_boundaries(dev, B, H, Tk):
    """Both sides of ops' Tk >= 512 gate and of the kernel's ntiles >= 8 rule; 8, 9, 10, 13 and 17 key tiles: pick_ksplit's
    loop leaves at 4 ranges (8, 10, 13, 17 tiles) and at 3 (9 tiles: 4 ranges of 3 would leave the last one empty)."""
    inp, o = _fwd_plain(dev, B, H, 100, Tk, 0, 1000 + Tk)
    compare(f"C split BH{B * H} 100x{Tk}", {"o": o}, inp, H, 0, 1.0, 1.0, None, 1.0, backward=False)


# ----------------------------------------------------------------------------- D. hard inputs
def hard_inputs(kind, B, H, Tq, Tk, seed):
    inp = gaussian(B, H, Tq, Tk, seed)
    D = H * HD
    if kind in ("max_in_last_ragged_tile", "max_in_first_tile"):
        # every query leans 2 units along one direction u of its head, and ONE key is 8 u: its score is about 16 while the
        # others stay around +-3.4, so it holds the row maximum of every row
        j = Tk - 1 if kind == "max_in_last_ragged_tile" else 3
        u = torch.nn.functional.normalize(rnd((H, HD), torch.float64, "cpu", seed + 9), dim=-1).reshape(D)
        inp["q"] = (inp["q"].double() + 2.0 * u).to(BF)
        inp["k"][:, j] = (8.0 * u).to(BF)
    elif kind == "sharp":     # scores with a std of about 12: near one-hot rows
        inp["q"] = rnd((B, Tq, D), BF, "cpu", seed, 1.5)
    elif kind == "uniform":   # every probability 1 / Tk: o is the mean of v, dk is exactly zero
        inp["q"] = torch.zeros_like(inp["q"])
    elif kind == "quiet_head":  # one (batch, head) at 2^-6 of the others, inputs and cotangent
        for t in inp.values():
            t.view(B, -1, H, HD)[B - 1, :, 0] *= 2.0 ** -6
    elif kind == "large_do":
        inp["do"] = rnd((B, Tq, D), BF, "cpu", seed + 3, 64.0)
    else:
        raise KeyError(kind)
    return inp


@pytest.mark.parametrize("drop", [0.0, 0.1])
@pytest.mark.parametrize("kind", ["max_in_last_ragged_tile", "max_in_first_tile", "sharp", "uniform", "quiet_head", "large_do"])
@pytest.mark.parametrize("B,H,Tq,Tk", [(2, 3, 100, 333),    # ragged last key tile (13 keys), two passes
                                       (2, 2, 200, 1500),   # 24 key tiles, ragged last one (28 keys), two query blocks
                                       (2, 3, 130, 200)])   # the one-launch backward, 2 + 2 blocks, 8 keys in the last tile
def test_hard_inputs(dev, B, H, Tq, Tk, kind, drop):
    c = Case(dev, B, H, Tq, Tk, 0, drop, hard_inputs(kind, B, H, Tq, Tk, 1100 + Tk))
    kern, _ = c.run_and_compare(f"D {kind} ({B},{H},{Tq}x{Tk}) drop{drop}")
    if kind == "uniform":
        assert kern.rec["dk"]["mag"] == 0.0 and not bool(c.out_grad("dk").count_nonzero())


# ----------------------------------------------------------------------------- E. argument checks
def _bad_arguments(c):
    """(label, forward too?, mutation of a valid descriptor)"""
    def f(**kw):
        def apply(d):
            for k_, v_ in kw.items():
                setattr(d, k_, v_(getattr(d, k_)) if callable(v_) else v_)
        return apply
    return [
        ("token stride not a multiple of 8", True, f(k_st=lambda s: s + 4)),
        ("batch stride not a multiple of 8", True, f(v_sb=lambda s: s + 4)),
        ("o token stride not a multiple of 8", True, f(o_st=lambda s: s + 2)),
        ("q pointer off 16-byte alignment", True, f(q=lambda p: p + 8)),
        ("mask_mode 2", True, f(mask_mode=2)),
        ("score_scale < 0", True, f(score_scale=-0.125)),
        ("dropout without a drop_mask", True, f(drop_mask=None)),
        ("drop_mask 16 bytes short", True, f(drop_mask_bytes=lambda n: n - 16)),
        ("drop_mask off 16-byte alignment", True, f(drop_mask=lambda p: p + 4)),
        ("bwd_passes 4", False, f(bwd_passes=4)),
        ("bwd_passes -1", False, f(bwd_passes=-1)),
        ("delta NULL", False, f(delta=None)),
        ("dq token stride not a multiple of 8", False, f(dq_st=lambda s: s + 4)),
        ("dO pointer off 16-byte alignment", False, f(d_o=lambda p: p + 2)),
    ]


def _refused(c, entry, d, label):
    rc = getattr(c.lib, entry)(C.byref(d), c.ops.stream())
    assert rc == TMI_ERR_INVALID, (entry, label, rc)
    msg = c.lib.tmi_last_error()
    assert msg and msg.decode().startswith(entry + ":"), (entry, label, msg)  # (fwd and bwd alternate, so each call set it)
    torch.cuda.synchronize()
    c.assert_canaries()  # with nothing owned: no output byte changed, so nothing was launched


def test_attention_rejects_bad_arguments(dev):
    ops, _lib = _mods()
    B, H, Tq, Tk = 2, 2, 100, 200
    c = Case(dev, B, H, Tq, Tk, 0, 0.1, gaussian(B, H, Tq, Tk, 1200), form="cross")
    for buf in c.bufs.values():
        buf.owned[:] = False
    for label, fwd_too, mutate in _bad_arguments(c):
        if fwd_too:
            d = c.desc()
            mutate(d)
            _refused(c, "tmi_attn_fwd", d, label)
        d = c.bwd_desc()
        mutate(d)
        _refused(c, "tmi_attn_bwd", d, label)
    # through ops: the error is raised
    with pytest.raises(_lib.TmiError):
        ops.attn_fwd(c.Q, c.K, c.V, c.O, c.bufs["stats"].body, B, H, Tq, Tk, 2)
    with pytest.raises(_lib.TmiError):
        ops.attn_bwd(c.Q, c.K, c.V, c.O, c.bufs["stats"].body, c.DO, c.DQ, c.DK, c.DV, c.bufs["delta"].body, B, H, Tq, Tk, 0, passes=4)
    with pytest.raises(_lib.TmiError):
        ops.attn_fwd(c.Q, c.K, c.V, c.O, c.bufs["stats"].body, B, H, Tq, Tk, 0, score_scale=-1.0)
    torch.cuda.synchronize()
    c.assert_canaries()
    # the untouched descriptor is accepted, so each refusal above was the mutated field's
    assert c.lib.tmi_attn_fwd(C.byref(c.desc()), ops.stream()) == 0
    assert c.lib.tmi_attn_bwd(C.byref(c.bwd_desc()), ops.stream()) == 0
    torch.cuda.synchronize()
    assert not c.bufs["o"].untouched() and not c.bufs["dq"].untouched() and not c.bufs["dkv"].untouched()


def test_attention_dropout_rejects_more_than_2_17_keys(dev):
    """dropout_p > 0 with Tk = 2^17 + 1 (the generator's column limit, TMI_DROP_MAX_COLS): B = H = 1 and Tq = 8 keep the
    buffers small (kvc_all and dkv 32 MiB each with one layer, the mask 2 MiB).  The same call without dropout is accepted."""
    B, H, Tq, Tk = 1, 1, 8, (1 << 17) + 1
    D = HD
    inp = {"q": rnd((B, Tq, D), BF, "cpu", 1300, 0.35), "k": torch.zeros((B, Tk, D), dtype=BF),
           "v": torch.ones((B, Tk, D), dtype=BF), "do": rnd((B, Tq, D), BF, "cpu", 1303)}
    c = Case(dev, B, H, Tq, Tk, 0, 0.1, inp, form="cross", layers=1, layer=0)
    for buf in c.bufs.values():
        buf.owned[:] = False
    _refused(c, "tmi_attn_fwd", c.desc(), "Tk = 2^17 + 1 with dropout")
    _refused(c, "tmi_attn_bwd", c.bwd_desc(), "Tk = 2^17 + 1 with dropout")
    d = c.desc()
    d.dropout_p = 0.0
    assert c.lib.tmi_attn_fwd(C.byref(d), c.ops.stream()) == 0
    torch.cuda.synchronize()
    assert not c.bufs["o"].untouched()
