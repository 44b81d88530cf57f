"""Float64 references, seeded inputs and bounds for the Wav2Vec2 pre-training kernels (csrc/wav2vec2.hip).  CPU only: nothing
here imports the GPU package or the oracle, so tests/test_w2v_kernel_ref_cpu.py can check these restatements (against the
oracle and autograd) and every property of the inputs the GPU tests lean on before any kernel is compared with them.

Each reference is the operation's formula in torch.float64, written from the formula and not from the kernel:
``gn_ref``            GroupNorm + erf-GELU, its gradients, the saved (mean, rstd) and (mean dxhat, mean dxhat*xhat)
``fir_ref``           Conv1D(k = 10, stride 5, "same", no bias) on one channel and its weight gradient
``pack_ref`` / ``unpack_ref`` / ``weight_pack_ref``   the positional-conv layout packs as index maps
``vq_dist`` / ``vq_argmin`` / ``perplexity_ref`` / ``vq_scatter_ref``   the quantiser
``contrastive_ref``   row loss and d loss / d S
``segment_sumsq_ref`` / ``clip_scale_f32``            gradient clipping
"""
import math

import numpy as np
import torch

U = 2.0 ** -24   # unit roundoff of fp32
F64 = torch.float64
NAN = float("nan")


def tol_fwd(dtype):   # the project's tolerances against float64, relative to max|ref| (tests/test_wav2vec2_gpu.py)
    return 1.5e-2 if dtype == torch.bfloat16 else 2e-5


def tol_grad(dtype):
    return 3e-2 if dtype == torch.bfloat16 else 1e-4


def randn(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=F64) * scale


def bf16_rne(x32):
    """fp32 -> bf16 by round-to-nearest-even on the bit pattern (no NaN inputs), independent of torch's conversion."""
    bits = x32.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    r = ((bits + 0x7FFF + ((bits >> 16) & 1)) >> 16) & 0xFFFF
    r = torch.where(r >= 0x8000, r - 0x10000, r).to(torch.int16)
    return r.view(torch.bfloat16)


# ------------------------------------------------------------------------------------------------- GELU
def gelu(z):
    return 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))


def gelu_grad(z):
    return 0.5 * (1.0 + torch.erf(z / math.sqrt(2.0))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


# ------------------------------------------------------------------------------------------------- GroupNorm + GELU
# (B, T, C, G, dtypes): the path each shape reaches.  chunks = min(32, ceil(T / 64)), rows per chunk = ceil(T / chunks);
# a thread owns one 16-byte vector of a row (VEC = 4 fp32 / 8 bf16 channels), cpr = C / VEC threads cover a row,
# rstep = 256 / cpr rows run side by side; per = (C / G) / VEC vectors per group; the fold uses nsub = 256 / G slices.
GN_SHAPES = [
    # T = 1: one chunk of one row, rstep = 32 (fp32: cpr 8) / 64 (bf16: cpr 4) row lanes of which one has work
    ("one-row", (2, 1, 32, 4), "both"),
    # T = 65: 2 chunks of 33 rows, last chunk 32 rows (r1 = min(T, ...) cuts it)
    ("two-chunks-ragged", (2, 65, 64, 4), "both"),
    # T = 67: 2 chunks of 34, last 33; G = 1: one group spans the row, nsub = 256 fold slices for 2 chunks
    ("one-group", (3, 67, 64, 1), "both"),
    # T = 2113: ceil(2113 / 64) = 34 -> capped to 32 chunks of ceil(2113 / 32) = 67 rows, last chunk 2113 - 31 * 67 = 36 rows
    ("32-chunks-of-67-last-36", (1, 2113, 64, 8), "both"),
    # C = 2048 bf16: cpr = 256, rstep = 1; C / G = 8 = VEC: per = 1; G = 256: nsub = 1, all 256 threads fold
    ("rstep1-per1-nsub1-bf16", (2, 70, 2048, 256), "bf16"),
    # C = 1024 fp32: cpr = 256, rstep = 1; C / G = 4 = VEC: per = 1; G = 256: nsub = 1.  T = 70: 2 chunks of 35
    ("rstep1-per1-nsub1-fp32", (2, 70, 1024, 256), "fp32"),
    # C / G = 8 in bf16 (per = 1) with rstep = 4 and 5 chunks of 60 rows
    ("cg8-bf16", (1, 300, 512, 64), "bf16"),
]
GN_CLASS_SHAPE = (2, 65, 64, 4)
GN_CONST_GROUP = 1       # the group held at GN_CONST_VALUE in the "const" class
GN_CONST_VALUE = 0.5
GN_OFFSET_RATIO = 16.0   # mean / std of every group in the "offset" class


def gn_cases():
    out = []
    for name, shape, which in GN_SHAPES:
        for dt_ in (torch.float32, torch.bfloat16):
            if which == "both" or (which == "bf16") == (dt_ == torch.bfloat16):
                out.append((name, shape, dt_))
    return out


def gn_inputs(shape, dtype, kind="plain"):
    """-> x, dy (in ``dtype``: the reference sees the rounded values), gamma, beta (fp32), all on the CPU."""
    B, T, C, G = shape
    x = randn((B, T, C), 101, 1.5) + 0.3
    if kind == "const":
        x.reshape(B, T, G, C // G)[:, :, GN_CONST_GROUP, :] = GN_CONST_VALUE
    elif kind == "offset":
        x = randn((B, T, C), 102, 0.5) + 0.5 * GN_OFFSET_RATIO
    dy = randn((B, T, C), 103)
    gamma = (randn((C,), 104, 0.2) + 1.0).float()
    beta = randn((C,), 105, 0.2).float()
    return x.to(dtype), dy.to(dtype), gamma, beta


def gn_ref(x, dy, gamma, beta, G, eps):
    """Everything the forward and the backward produce, float64.  x, dy [B, T, C]; statistics per (batch row, group) over
    (time, C / G) with the biased variance."""
    x, dy, gamma, beta = (t.to(F64) for t in (x, dy, gamma, beta))
    B, T, C = x.shape
    xg = x.reshape(B, T, G, C // G)
    mean = xg.mean(dim=(1, 3))
    var = ((xg - mean[:, None, :, None]) ** 2).mean(dim=(1, 3))
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = ((xg - mean[:, None, :, None]) * rstd[:, None, :, None]).reshape(B, T, C)
    z = gamma * xhat + beta
    y = gelu(z)
    dz = dy * gelu_grad(z)
    dxhat = dz * gamma
    m1 = dxhat.reshape(B, T, G, -1).mean(dim=(1, 3))
    m2 = (dxhat * xhat).reshape(B, T, G, -1).mean(dim=(1, 3))
    rep = C // G
    dx = rstd.repeat_interleave(rep, 1)[:, None, :] * (dxhat - m1.repeat_interleave(rep, 1)[:, None, :]
                                                        - xhat * m2.repeat_interleave(rep, 1)[:, None, :])
    return dict(y=y, dx=dx, dgamma=(dz * xhat).sum(dim=(0, 1)), dbeta=dz.sum(dim=(0, 1)),
                stats=torch.stack([mean, rstd], -1), sums=torch.stack([m1, m2], -1), z=z, var=var)


def gn_chunks(T):
    """tmi_groupnorm_chunks restated (the GPU test asserts the library agrees)."""
    return max(1, min(32, (T + 63) // 64))


def gn_two_pass_fp32(x, dy, gamma, beta, G, eps):
    """The textbook two-pass algorithm in float32: the mean first, then the centred sum of squares, each as numpy float32
    sums over the kernel's row chunks whose partials are then added in chunk order; the apply formulas in float32 too.
    Its float64 error is what the "offset" class's bound is made of (gn_offset_bounds)."""
    B, T, C = x.shape
    nch = gn_chunks(T)
    rpc = -(-T // nch)
    f = np.float32
    xn = x.float().numpy().reshape(B, T, G, C // G)
    cnt = f(T * (C // G))
    mean = np.zeros((B, G), f)
    ssq = np.zeros((B, G), f)
    for c in range(nch):
        mean += xn[:, c * rpc:(c + 1) * rpc].sum(axis=(1, 3), dtype=f)
    mean = mean / cnt
    d = xn - mean[:, None, :, None]
    for c in range(nch):
        ssq += (d[:, c * rpc:(c + 1) * rpc] ** 2).sum(axis=(1, 3), dtype=f)
    rstd = f(1.0) / np.sqrt(ssq / cnt + f(eps))
    xhat = torch.from_numpy((d * rstd[:, None, :, None]).reshape(B, T, C))
    g32, b32 = gamma.float(), beta.float()
    z = g32 * xhat + b32
    y = 0.5 * z * (1.0 + torch.erf(z * np.float32(math.sqrt(0.5))))
    dz = dy.float() * (0.5 * (1.0 + torch.erf(z * np.float32(math.sqrt(0.5)))) + z * torch.exp(-0.5 * z * z) * np.float32(1.0 / math.sqrt(2.0 * math.pi)))
    dxhat = dz * g32
    m1 = dxhat.reshape(B, T, G, -1).numpy().sum(axis=(1, 3), dtype=f) / cnt
    m2 = (dxhat * xhat).reshape(B, T, G, -1).numpy().sum(axis=(1, 3), dtype=f) / cnt
    rep = C // G
    r_, m1_, m2_ = (torch.from_numpy(np.repeat(a, rep, 1))[:, None, :] for a in (rstd, m1, m2))
    dx = r_ * (dxhat - m1_ - xhat * m2_)
    return dict(y=y, dx=dx, stats=torch.from_numpy(np.stack([mean, rstd], -1)), sums=torch.from_numpy(np.stack([m1, m2], -1)))


def gn_one_pass_fp32(x, G, eps):
    """E[x^2] - mean^2 from float32 chunk sums folded in float64 (the form the kernel had before its statistics were centred
    on a pivot): -> (mean, rstd).  Kept so that the CPU test shows why that form had to go."""
    B, T, C = x.shape
    nch = gn_chunks(T)
    rpc = -(-T // nch)
    xn = x.float().numpy().reshape(B, T, G, C // G)
    a = np.zeros((B, G), np.float64)
    s = np.zeros((B, G), np.float64)
    for c in range(nch):
        blk = xn[:, c * rpc:(c + 1) * rpc]
        a += blk.sum(axis=(1, 3), dtype=np.float32)
        s += (blk * blk).sum(axis=(1, 3), dtype=np.float32)
    cnt = T * (C // G)
    mean = a / cnt
    var = np.maximum(s / cnt - mean * mean, 0.0)
    return torch.from_numpy(np.stack([mean.astype(np.float32), (1.0 / np.sqrt(var + eps)).astype(np.float32)], -1))


def rel_max(got, ref):
    got, ref = got.detach().to(F64).cpu(), ref.detach().to(F64).cpu()
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-300))


def gn_offset_bounds(dtype=torch.float32, eps=1e-5):
    """The "offset" class (mean / std = 16 per group) has no bound known in advance: it is FOUR times the float64 error of
    gn_two_pass_fp32 on the same inputs (the factor: the kernel's summation order is not the emulation's).  Every entry is
    max|err| / max|ref|; "rstd" is relative per entry.  -> (bounds, measured two-pass errors)."""
    x, dy, gamma, beta = gn_inputs(GN_CLASS_SHAPE, dtype, "offset")
    G = GN_CLASS_SHAPE[3]
    ref = gn_ref(x, dy, gamma, beta, G, eps)
    emu = gn_two_pass_fp32(x, dy, gamma, beta, G, eps)
    meas = {k: rel_max(emu[k], ref[k]) for k in ("y", "dx")}
    meas["mean"] = rel_max(emu["stats"][..., 0], ref["stats"][..., 0])
    meas["rstd"] = float(((emu["stats"][..., 1].double() - ref["stats"][..., 1]) / ref["stats"][..., 1]).abs().max())
    return {k: 4.0 * v for k, v in meas.items()}, meas


# ------------------------------------------------------------------------------------------------- FIR stem
# (B, Tin, C, G): T = ceil(Tin / 5).  A thread owns 8 channels: cpr = C / 8, rstep = 256 / cpr.  Forward and the backward
# sums pass use fir chunks = min(64, ceil(T / 100)); the backward apply pass uses the GroupNorm chunking min(32, ceil(T / 64))
# and leaves B * chunks partial rows which the reduce kernel folds in 8 y-slices when there are >= 64 of them.
FIR_SHAPES = [
    # Tin = 5: T = 1, pad 5 (left 2): every window overhangs both ends.  C = 8: cpr = 1, rstep = 256; C / G = 8
    ("T1-cpr1-rstep256", (2, 5, 8, 1)),
    # Tin = 7: T = 2, pad 8 (left 4).  C = 16, G = 2: C / G = 8, cpr = 2, rstep = 128
    ("T2-cg8", (2, 7, 16, 2)),
    # C = 2048: cpr = 256, rstep = 1.  Tin = 333: T = 67: 1 fir chunk of 67, 2 GroupNorm chunks of 34 + 33
    ("rstep1", (1, 333, 2048, 64)),
    # Tin = 10565: T = 2113: fir chunks ceil(2113 / 100) = 22 of 97 rows, last 2113 - 21 * 97 = 76; GroupNorm chunks 32 of 67,
    # last 36; 3 * 32 = 96 partial rows >= 64 -> 8 reduce slices of 12 rows: one unrolled round of 8 and 4 single steps
    ("T2113-ragged-both-96-parts", (3, 10565, 64, 2)),
    # Tin = 4500: T = 900: 9 fir chunks of 100; GroupNorm chunks ceil(900 / 64) = 15 of 60; 5 * 15 = 75 partial rows into 8
    # slices: slices 0-2 take 10 rows (one round of 8 + 2), slices 3-7 take 9 (one round of 8 + 1)
    ("T900-75-parts", (5, 4500, 32, 4)),
]
FIR_K, FIR_S = 10, 5


def same_pad(Tin, k, s):
    out = -(-Tin // s)
    total = max((out - 1) * s + k - Tin, 0)
    return out, total // 2, total - total // 2


def fir_inputs(shape, dtype, kind="plain"):
    """-> audio [B, Tin] fp32, w [10, 1, C] fp32, gamma, beta fp32, dy [B, T, C] in ``dtype``."""
    B, Tin, C, G = shape
    T = same_pad(Tin, FIR_K, FIR_S)[0]
    audio = randn((B, Tin), 201) if kind == "plain" else 0.25 + randn((B, Tin), 202, 0.01)   # "dc": offset 0.25, amplitude 0.01
    w = randn((FIR_K, 1, C), 203, 0.3)
    gamma = randn((C,), 204, 0.2) + 1.0
    beta = randn((C,), 205, 0.2)
    dy = randn((B, T, C), 206)
    return audio.float(), w.float(), gamma.float(), beta.float(), dy.to(dtype)


def fir_windows(audio, k=FIR_K, s=FIR_S):
    """[B, T, k]: window t holds audio[5 t + j - pad_left], zero outside the clip."""
    B, Tin = audio.shape
    T, pl, _ = same_pad(Tin, k, s)
    idx = torch.arange(T)[:, None] * s + torch.arange(k)[None, :] - pl
    ok = (idx >= 0) & (idx < Tin)
    return torch.where(ok[None], audio.to(F64)[:, idx.clamp(0, Tin - 1)], torch.zeros((), dtype=F64))


def fir_conv(audio, w):
    """u[b, t, c] = sum_j audio[b, 5 t + j - pad_left] w[j, 0, c], float64."""
    return torch.einsum("btj,jc->btc", fir_windows(audio), w.to(F64)[:, 0, :])


def fir_ref(audio, w, gamma, beta, dy, G, eps):
    u = fir_conv(audio, w)
    r = gn_ref(u, dy, gamma, beta, G, eps)
    r["dW"] = torch.einsum("btj,btc->jc", fir_windows(audio), r["dx"])[:, None, :]   # du = the GroupNorm input gradient
    r["u"] = u
    return r


# ------------------------------------------------------------------------------------------------- packs (index maps)
def pack_ref(x, B, T, C, G, Tp, pl):
    """x [B*T, C] -> xg [G, B*Tp, C/G]: row b*Tp + r holds source row b*T + r - pl for 0 <= r - pl < T, zero elsewhere."""
    Cg = C // G
    out = torch.zeros((G, B, Tp, Cg), dtype=x.dtype)
    out[:, :, pl:pl + T, :] = x.reshape(B, T, G, Cg).permute(2, 0, 1, 3)
    return out.reshape(G, B * Tp, Cg)


def unpack_ref(yg, B, T, C, G, Tp, row_off):
    """yg [G, B*Tp, C/G] -> [B*T, C]: out[b*T + t][g*Cg + j] = yg[g][b*Tp + t + row_off][j]."""
    Cg = C // G
    return yg.reshape(G, B, Tp, Cg)[:, :, row_off:row_off + T, :].permute(1, 2, 0, 3).reshape(B * T, C).contiguous()


def weight_pack_ref(w, k, Cg, G):
    """w [k, Cg, C] -> wf[g][kk*Cg + i][o] = w[kk][i][g*Cg + o], wb[g][kk'*Cg + o][i] = w[k-1-kk'][i][g*Cg + o]."""
    w5 = w.reshape(k, Cg, G, Cg)                          # [kk, i, g, o]
    wf = w5.permute(2, 0, 1, 3).reshape(G, k * Cg, Cg)
    wb = w5.flip(0).permute(2, 0, 3, 1).reshape(G, k * Cg, Cg)
    return wf.contiguous(), wb.contiguous()


# (B, T, C, G, k)
PACK_SHAPES = [
    ("T-lt-k-cg8", (1, 5, 24, 3, 8)),         # T = 5 < k = 8, C / G = 8
    ("odd-k-one-group", (3, 20, 64, 1, 7)),   # k = 7, G = 1
    # Tp = 1100 + 7: 2 * 1107 * 512 = 1 133 568 elements = 4428 blocks of 256 > the 4096-block cap: the pack's grid wraps;
    # the unpack has 2 * 1100 * 512 = 1 126 400 elements = 4400 blocks and wraps too
    ("grid-wraps", (2, 1100, 512, 16, 8)),
]


# ------------------------------------------------------------------------------------------------- quantiser
# (rows, G, Nc, gd).  One wave per (row, group), 4 waves per workgroup; lane l takes codes l, l + 64, ...
VQ_SHAPES = [
    ("rowsG-201-Nc17-gd24", (201, 1, 17, 24)),     # 201 items: 201 % 4 = 1 (a workgroup with 3 idle waves); Nc = 17 < 64: 47 lanes keep bi = 0x7fffffff; gd = 24 < 64
    ("Nc70-gd100", (50, 3, 70, 100)),              # 150 items: 150 % 4 = 2; Nc = 70 and gd = 100: not multiples of 64 (6 lanes take two codes)
    ("base-320-128", (64, 2, 320, 128)),           # the model's code book: 5 codes per lane
]
VQ_TIE_CODE = 3   # code c of the planted ties: rows (c, c+1) [neighbouring lanes] and, where Nc > c + 64, (c, c+64) [one lane]
VQ_BWD_SHAPE = (1100, 2, 16, 256)   # 1100 * 2 * 256 = 563 200 elements = 2200 blocks > the 2048-block cap; 2200 / 32 ~ 69 rows a code


def vq_inputs(shape, dtype, ties=False):
    """-> h [rows, G*gd] in ``dtype``, codebook [G, Nc, gd] fp32, tie_rows (h rows planted next to the duplicated code)."""
    rows, G, Nc, gd = shape
    h = randn((rows, G * gd), 301)
    cb = randn((G, Nc, gd), 302).float()
    tie_rows = []
    if ties:
        c = VQ_TIE_CODE
        cb[:, c + 1] = cb[:, c]
        if Nc > c + 64:
            cb[:, c + 64] = cb[:, c]
        tie_rows = [0, 5, rows - 1]
        for r in tie_rows:   # the row sits next to code c in every group: c and its copies are the nearest codes
            h[r] = (cb[:, c].double() + randn((G, gd), 303 + r, 0.01)).reshape(-1)
    return h.to(dtype), cb, tie_rows


def vq_dist(h, cb):
    """[rows, G, Nc] float64 squared distances."""
    G, Nc, gd = cb.shape
    hh = h.to(F64).reshape(-1, G, gd)
    return ((hh[:, :, None, :] - cb.to(F64)[None]) ** 2).sum(-1)


def vq_argmin(dist):
    """First index of the minimum (torch.argmin does not promise the first: done by hand)."""
    mn = dist.min(-1, keepdim=True).values
    Nc = dist.shape[-1]
    return torch.where(dist == mn, torch.arange(Nc).expand_as(dist), torch.full_like(dist, Nc, dtype=torch.int64)).min(-1).values


def vq_dist_bound(d, gd):
    """fp32 error of the kernel's distance sum s = sum_d (h_d - c_d)^2: every term carries the subtraction's and the
    square's rounding (2 u, or 1 with a fused multiply-add), the gd terms are added one after the other (gd - 1 additions):
    |s - d| <= (gd + 1) u d (1 + O(u)) since every term is >= 0.  (gd + 2) u d covers the second order."""
    return (gd + 2) * U * d


def vq_judge(idx, dist, gd):
    """The rule of the quantiser tests -> (ok [rows, G] bool, decisive [rows, G] bool).  A row is decisive when the float64
    gap between its two best codes exceeds the two distances' fp32 bounds: there the index must be the float64 argmin.
    Elsewhere the chosen code's float64 distance must be within the bounds of the minimum."""
    srt = dist.sort(-1).values
    d1, d2 = srt[..., 0], srt[..., 1] if dist.shape[-1] > 1 else srt[..., 0] + 1.0
    decisive = (d2 - d1) > vq_dist_bound(d1, gd) + vq_dist_bound(d2, gd)
    ref = vq_argmin(dist)
    idx = idx.long()
    inrange = (idx >= 0) & (idx < dist.shape[-1])
    dk = torch.gather(dist, -1, idx.clamp(0, dist.shape[-1] - 1).unsqueeze(-1)).squeeze(-1)
    near = dk - d1 <= vq_dist_bound(d1, gd) + vq_dist_bound(dk, gd)
    return inrange & torch.where(decisive, idx == ref, near), decisive


def vq_tie_rows(dist, gd):
    """[rows, G] bool, for the tie inputs: the float64 argmin is VQ_TIE_CODE and, its copies aside, no code is within the fp32
    bounds of it.  The copies are bit-identical rows of the code book, so their fp32 sums are equal too: the first index,
    VQ_TIE_CODE, is the only right answer."""
    c, Nc = VQ_TIE_CODE, dist.shape[-1]
    other = torch.ones(Nc, dtype=torch.bool)
    other[[k for k in (c, c + 1, c + 64) if k < Nc]] = False
    o = dist[..., other].min(-1).values
    dc = dist[..., c]
    return (vq_argmin(dist) == c) & (o - dc > vq_dist_bound(o, gd) + vq_dist_bound(dc, gd))


def perplexity_ref(idx, Nc):
    """mean_g exp(-sum_c p log(p + 1e-10)), p = clip(count / rows, 1e-10, 1); idx [rows, G] int."""
    rows, G = idx.shape
    out = 0.0
    for g in range(G):
        p = (torch.bincount(idx[:, g].long(), minlength=Nc).to(F64) / rows).clamp(1e-10, 1.0)
        out += math.exp(-float((p * torch.log(p + 1e-10)).sum()))
    return out / G


def vq_scatter_ref(idx, dq, Nc):
    """dcodebook[g][idx[r][g]][:] += dq[r][g][:] -> (sum [G, Nc, gd], sum of |terms|, rows per code [G, Nc])."""
    rows, G = idx.shape
    gd = dq.shape[1] // G
    d = dq.to(F64).reshape(rows, G, gd)
    s = torch.zeros((G, Nc, gd), dtype=F64)
    a = torch.zeros_like(s)
    n = torch.zeros((G, Nc), dtype=F64)
    for g in range(G):
        s[g].index_add_(0, idx[:, g].long(), d[:, g])
        a[g].index_add_(0, idx[:, g].long(), d[:, g].abs())
        n[g] = torch.bincount(idx[:, g].long(), minlength=Nc).to(F64)
    return s, a, n


def perplexity_patterns(rows, G, Nc):
    """Two of the three index patterns of the perplexity check (the third is the argmin's own choice)."""
    one = torch.full((rows, G), Nc - 1, dtype=torch.int32)                              # every row on one code: perplexity 1
    spread = ((torch.arange(rows)[:, None] * 7 + torch.arange(G)[None, :]) % Nc).int()  # 7 and Nc coprime or not: near uniform
    return {"one-code": one, "spread": spread}


# ------------------------------------------------------------------------------------------------- contrastive loss
# (B, T, Nn, per_time).  One workgroup of 128 threads per (b, t) row: three loops of stride 128 over the Nn + 1 logits, two
# over the T columns.
CONTRASTIVE_SHAPES = [
    ("T1-all-negatives-are-t", (2, 1, 3, False)),       # T = 1: every negative is 0 = t: four atomics on one LDS word
    ("no-negatives", (2, 130, 0, False)),               # Nn = 0: loss 0, dS row all zeros; T = 130 > 128: the column loops run twice
    ("T300-Nn200", (2, 300, 200, False)),               # 201 logits: the logit loops run twice; 300 columns: three times
    ("T150-Nn129-per-time", (2, 150, 129, True)),       # 130 logits: thread 0 and 1 take two, the others one
]
CONTRASTIVE_TEMP = 0.1
CONTRASTIVE_GRAD_SCALE = 0.37


def contrastive_inputs(shape, kind="plain"):
    """-> S [B, T, T] fp32, neg int32 [B, Nn] or [T, Nn] drawn WITH replacement (repeats and hits on t occur)."""
    B, T, Nn, per_time = shape
    S = randn((B, T, T), 401, 0.3)
    if kind == "large":        # |S| / temperature up to ~2000: without the max subtraction exp() overflows
        g = torch.Generator().manual_seed(402)
        S = (torch.rand((B, T, T), generator=g, dtype=F64) * 2.0 - 1.0) * 200.0
    elif kind == "dominant":   # the positive logit 50 / 0.1 = 500 above the rest: loss ~ 0, every p_neg underflows
        S = S + 50.0 * torch.eye(T, dtype=F64)
    rng = np.random.default_rng(403)
    neg = rng.integers(0, T, size=((T if per_time else B), Nn)).astype(np.int32)
    return S.float(), torch.from_numpy(neg)


def contrastive_ref(S, neg, temperature, grad_scale, per_time):
    """-> row_loss [B*T], dS [B, T, T] (= d(sum of row losses) / dS * grad_scale), sampled [B, T, T] bool, and the sum of
    |terms| behind every dS entry (a column sampled more than once, or t among its own negatives, adds several).  The temperature
    and grad_scale cross the C ABI as fp32 and the kernel multiplies by fl32(1 / temperature): the reference takes those."""
    B, T, _ = S.shape
    inv_t = float(np.float32(1.0) / np.float32(temperature))
    gs = float(np.float32(grad_scale))
    S = S.to(F64)
    loss = torch.zeros(B * T, dtype=F64)
    dS = torch.zeros_like(S)
    dS_abs = torch.zeros_like(S)
    sampled = torch.zeros(S.shape, dtype=torch.bool)
    for b in range(B):
        for t in range(T):
            nb = (neg[t] if per_time else neg[b]).long()
            cols = torch.cat([torch.tensor([t]), nb])
            lg = S[b, t, cols] * inv_t
            lse = torch.logsumexp(lg, 0)
            loss[b * T + t] = lse - lg[0]
            p = torch.exp(lg - lse)
            p[0] -= 1.0
            dS[b, t].index_add_(0, cols, p * inv_t * gs)
            dS_abs[b, t].index_add_(0, cols, p.abs() * inv_t * gs)
            sampled[b, t, cols] = True
    return loss, dS, sampled, dS_abs


# ------------------------------------------------------------------------------------------------- segments
SEG_OFFSETS = [0, 101, 101, 103, 4001, 60000]   # starts 101, 103, 4001 are not multiples of 4 (scalar path); [101, 101) is empty;
SEG_CLIP = 1.0                                  # [101, 103) has 2 elements (shorter than the 16-way split: 15 slices get nothing)
SEG_BIG_N = 1_700_000   # one segment, 512 slices of 3324 elements = 831 float4: threads 0-62 run the four-in-flight round


def seg_inputs(n=SEG_OFFSETS[-1], seed=501):
    return randn((n,), seed, 0.05).float()


def segment_sumsq_ref(g, offs):
    return torch.stack([(g[a:b].to(F64) ** 2).sum() for a, b in zip(offs[:-1], offs[1:])])


def segment_sum_bound(n, split, exact, natomics=None):
    """fp32 error of a segment's sum of squares.  Every square is rounded once (1).  A thread adds its elements one after
    the other: a slice holds per = ceil(n / split) rounded up to 4 elements and 256 threads share it, so at most
    ceil(per / 256) + 3 of them (the + 3: a thread takes whole float4s) - that many sequential additions.  The workgroup
    fold is 6 butterfly levels plus 3 additions of the wave sums (9), and the slices meet in ``natomics`` atomic additions on
    one word, in any order (a chain as long as their number).  All terms are >= 0, so the sum of |terms| is the sum itself:
    |err| <= (1 + ceil(per / 256) + 3 + 9 + natomics) u * exact."""
    per = (-(-n // split) + 3) // 4 * 4 if n else 0
    k = 1 + (-(-per // 256) + 3) + 9 + (split if natomics is None else natomics)
    return k * U * float(exact)


def clip_scale_f32(ss32, clip):
    """fl32(clip / max(sqrt(ss), clip)) with every operation in fp32 (sqrt and division are correctly rounded)."""
    ss32 = np.asarray(ss32, dtype=np.float32)
    c = np.float32(clip)
    return (c / np.maximum(np.sqrt(ss32), c)).astype(np.float32)
