"""Float64 references, seeded inputs and per-element bounds for the row kernels of the Whisper step: LayerNorm
(csrc/layernorm.hip), cross-entropy, softmax, the decoder embedding and tmi_sum_scale (csrc/softmax_xent.hip).  CPU only:
nothing here imports the GPU package, so tests/test_row_kernel_ref_cpu.py checks the references (against the oracle and
autograd), the inputs and the bounds (reachable by an honest fp32 implementation, exceeded by every listed mutation) before
tests/test_row_kernels_gpu.py compares a kernel with them.

Every bound is per element (per row or column for sums) and analytic: a count of fp32 roundings times U = 2^-24 times
magnitudes of the REFERENCE's intermediates, plus UB = 2^-8 |ref| for a bf16 output.  gam(n) = n U / (1 - n U) is the
usual bound on a chain of n roundings.  The counts are written next to each bound; none is fitted, none is relative to a
tensor-wide maximum.  ``check_*(out, ref)`` returns the largest measured / bound of its ``ratios_*``.

UB is exact, not generous: round-to-nearest-even to bf16 errs by up to half an ulp, 2^-8 of a value at the lower edge of its
binade, so over a few thousand elements a correct bf16 output measures about 0.99 of its bound - and one more bf16 ulp (or
64 fp32 ulps on an fp32 output) exceeds it, which the CPU test shows.  fp32 outputs that are one rounding of a larger sum
(dx added onto an old dx much larger than it) come as close for the same reason.
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
UB = 2.0 ** -8
F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
NAN = float("nan")
TINY = 2.0 ** -100   # no reference output that a relative bound covers may lie below this: no underflow floor is needed


def gam(n):
    return n * U / (1.0 - n * U)


def dname(dtype):
    return "bf16" if dtype == BF16 else "fp32"


def randn(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=F64) * scale


def bf16_rne(x32):
    """fp32 -> bf16 by round-to-nearest-even on the bit pattern (no NaN inputs), independent of torch's conversion."""
    b = x32.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) & 0xFFFF
    r = torch.where(r >= 0x8000, r - 0x10000, r).to(torch.int16)
    return r.view(BF16)


def to_dtype(x32, dtype):
    return bf16_rne(x32.float()) if dtype == BF16 else x32.float()


def guard_pattern(n, dtype):
    """7.0 / NaN alternating (integers: 7 / a large negative): a stray store of any finite value, or of NaN, shows."""
    t = torch.full((n,), 7, dtype=dtype)
    t[1::2] = NAN if dtype.is_floating_point else -(2 ** 30)
    return t


def ratio(got, ref, bound):
    """max over elements of |got - ref| / bound; an exact element counts 0 whatever its bound, a NaN or an error against a
    zero bound counts inf."""
    got, ref = got.detach().to(F64).reshape(-1), ref.detach().to(F64).reshape(-1)
    bound = torch.as_tensor(bound, dtype=F64)
    bound = bound.expand(ref.shape) if bound.dim() == 0 else bound.reshape(-1)
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    if got.numel() == 0:
        return 0.0
    err = (got - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    r = torch.where(torch.isnan(r), torch.full_like(r, math.inf), r)
    return float(r.max())


# ================================================================================================= LayerNorm
LN_EPS = float(np.float32(1e-5))   # eps crosses the C ABI as fp32
LN_ROWS = [1, 3, 9, 17]            # < the 4 forward waves; 8 + 1 backward waves; 17: the first to enter the backward prefetch
# every NCH instantiation (1, 2, 3, 4, 8) with a last 16-byte chunk of one lane and with a full last chunk
LN_C = {F32: [4, 256, 260, 516, 772, 1028, 2048], BF16: [8, 512, 520, 1032, 1544, 2048]}
LN_EMIT_MAX_C = 1704               # 8 waves * 3 sums * C * 4 bytes <= 160 KiB
LN_BIG = (4097, 520)               # a forward wave walks two rows, a backward wave three
LN_KINDS = ["plain", "offset", "outlier", "const", "scales"]
LN_CLASS_SHAPE = {F32: (17, 516), BF16: (17, 520)}
LN_CONST_VALUE = 0.3
LN_DROP_P, LN_DROP_SEED = 0.25, 0xABCDEF12345


def ln_vec(dtype):
    return 8 if dtype == BF16 else 4


def ln_nch(C, dtype):
    need = -(-C // (64 * ln_vec(dtype)))
    return need if need <= 4 else 8


def ln_E(C, dtype):
    """A lane's serial additions per row: NCH chunks of VEC elements."""
    return ln_nch(C, dtype) * ln_vec(dtype)


def ln_bwd_blocks(rows):
    """ln_bwd_blocks of csrc/layernorm.hip restated -> (workgroups, rows a wave walks at most)."""
    rpw = max(2, -(-rows // (8 * 256)))
    return -(-rows // (8 * rpw)), rpw


def ln_fwd_rows_per_wave(rows):
    rpw = -(-rows // (4 * 1024))
    blocks = -(-rows // (4 * rpw))
    return -(-rows // (4 * blocks))


def ln_col_depth(rows):
    """Additions between one row's term and a column sum: a wave's serial walk (<= rpw), the 8-wave fold (8), then either one
    atomic per workgroup onto the destination (<= blocks) or the fold kernel's ceil(blocks / 16) + 16 + 1 (<= blocks + 16)."""
    blocks, rpw = ln_bwd_blocks(rows)
    return rpw + 8 + blocks + 16


def ln_inputs(rows, C, dtype, kind="plain"):
    """-> x, dy, old (the dx to accumulate onto) in ``dtype``; gamma, beta, and the bases of dgamma / dbeta / colsum in fp32."""
    x = randn((rows, C), 11, 2.0) + 0.5
    dy = randn((rows, C), 12)
    if kind == "offset":
        x = randn((rows, C), 13) + (8.0 if dtype == BF16 else 40.0)
    elif kind == "outlier":
        x = randn((rows, C), 14)
        x[:, sorted({0, C // 2, C - 1})] = 200.0
    elif kind == "const":
        x[rows // 2] = LN_CONST_VALUE
    elif kind == "scales":
        sc = 10.0 ** torch.linspace(-3.0, 3.0, rows, dtype=F64)[:, None] if rows > 1 else torch.ones((1, 1), dtype=F64)
        x, dy = x * sc, dy * sc.flip(0)
    old = randn((rows, C), 15)
    gamma = (randn((C,), 16, 0.3) + 1.0).float()
    beta = randn((C,), 17, 0.3).float()
    bases = [randn((C,), 18 + i).float() for i in range(3)]
    return dict(x=to_dtype(x, dtype), dy=to_dtype(dy, dtype), old=to_dtype(old, dtype), gamma=gamma, beta=beta, bases=bases,
                rows=rows, C=C, dtype=dtype, kind=kind)


def ln_fwd_ref(inp, keep=None, scale=1.0):
    """LayerNorm forward in float64 with the bounds of its three outputs.  ``keep`` [rows, C] bool, ``scale``: the fused
    Dropout (y kept * scale, dropped = +0).

    depth = E + 7: a lane adds its E elements (E - 1 roundings), 6 butterfly levels, fl(1 / C) and the multiply by it.
      dmu   <= gam(depth) mean|x|
      dvar  <= gam(E + 10) (var + dmu^2) + dmu^2 + 2 sigma dmu   (x - mu': 2 on the square, the square 1, E - 1 + 6 additions,
               1 / C twice; sum (x - mu')^2 / C = var + dmu^2; the 2 sigma dmu term is the skeleton's allowance)
      drstd / rstd <= dvar / (2 (var + eps - dvar)) + 3 U         (the eps addition 1/2, sqrt 1, the reciprocal 1: 2.5, stated as 3)
      dy    <= |gamma| (rstd dmu + |xhat| (drstd / rstd + 3 U)) + 2 U |y|   (x - mu, * rstd, * gamma: 3; + beta, and second order)
    and U |y| for the dropout scale, UB |y| for a bf16 output."""
    x, gamma, beta, dtype = inp["x"].to(F64), inp["gamma"].to(F64), inp["beta"].to(F64), inp["dtype"]
    C = x.shape[1]
    E = ln_E(C, dtype)
    mean = x.mean(-1)
    var = ((x - mean[:, None]) ** 2).mean(-1)
    rstd = 1.0 / torch.sqrt(var + LN_EPS)
    xhat = (x - mean[:, None]) * rstd[:, None]
    y = xhat * gamma + beta
    dmu = gam(E + 7) * x.abs().mean(-1)
    dvar = gam(E + 10) * (var + dmu ** 2) + dmu ** 2 + 2.0 * torch.sqrt(var) * dmu
    drs = dvar / (2.0 * (var + LN_EPS - dvar)) + 3.0 * U
    yb = gamma.abs() * (rstd * dmu)[:, None] + (gamma * xhat).abs() * (drs[:, None] + 3.0 * U) + 2.0 * U * y.abs()
    if keep is not None:
        y = torch.where(keep, y * scale, torch.zeros_like(y))
        yb = torch.where(keep, yb * scale + U * y.abs(), torch.zeros_like(y))
    if dtype == BF16:
        yb = yb + UB * y.abs()
    return dict(y=y, mean=mean, rstd=rstd, var=var, xhat=xhat, y_b=yb, mean_b=dmu, rstd_b=drs * rstd)


def ratios_ln_fwd(out, ref):
    return {k: ratio(out[k], ref[k], ref[k + "_b"]) for k in ("y", "mean", "rstd")}


def check_ln_fwd(out, ref):
    return max(ratios_ln_fwd(out, ref).values())


def ln_bwd_ref(inp, mean, rstd, accumulate, keep_dy=None, scale_dy=1.0, emit=False, keep=None, scale=1.0):
    """LayerNorm backward in float64 of (dy, x, gamma, mean, rstd) - the statistics are INPUTS of the backward, so the
    reference takes the values the kernel is given.  ``keep_dy``: the LayerNorm's output went through Dropout (dy is masked
    and rescaled on load, one more rounding ex = 1 on everything linear in dy).  ``emit``: colsum (+ ``keep``: masked).

    gg = dy gamma, s1 = sum gg / C, s2 = sum gg xhat / C, dx = rstd (gg - s1 - xhat s2) [+ old].  With A1 = sum |gg| / C and
    A2 = sum |gg xhat| / C of the element's own row:
      ds1 <= gam(E + 8 + ex) A1        (the product 1, E - 1 + 6 additions, 1 / C twice)
      ds2 <= gam(E + 11 + ex) A2       (xhat 2, gg 1, the product 1, then as above)
      ddx <= rstd ((4 + ex) U |gg| + 3 U |s1| + 7 U |xhat s2| + ds1 + |xhat| ds2)
             (|gg|: product, two subtractions, * rstd; |s1|: three; |xhat s2|: xhat 2, the product 1, subtraction, * rstd, + 2)
             + U |dx + old| when the old dx is added; UB |dx| for a bf16 output.
    Column sums: gam(roundings per term + ln_col_depth(rows)) (sum_r |term| + |base|); colsum also carries the sum of its
    terms' own fp32 bounds - its terms are the dx (or masked) values BEFORE they are rounded to the dtype."""
    x, dy, gamma, dtype = inp["x"].to(F64), inp["dy"].to(F64), inp["gamma"].to(F64), inp["dtype"]
    rows, C = x.shape
    E, ex = ln_E(C, dtype), (0 if keep_dy is None else 1)
    if keep_dy is not None:
        dy = torch.where(keep_dy, dy * scale_dy, torch.zeros_like(dy))
    mean, rstd = mean.to(F64), rstd.to(F64)
    xhat = (x - mean[:, None]) * rstd[:, None]
    gg = dy * gamma
    s1, s2 = gg.mean(-1, keepdim=True), (gg * xhat).mean(-1, keepdim=True)
    A1, A2 = gg.abs().mean(-1, keepdim=True), (gg * xhat).abs().mean(-1, keepdim=True)
    dx = rstd[:, None] * (gg - s1 - xhat * s2)
    b32 = rstd[:, None] * ((4 + ex) * U * gg.abs() + 3 * U * s1.abs() + 7 * U * (xhat * s2).abs() + gam(E + 8 + ex) * A1
                           + xhat.abs() * gam(E + 11 + ex) * A2)
    if accumulate:
        dx = dx + inp["old"].to(F64)
        b32 = b32 + U * dx.abs()
    depth = ln_col_depth(rows)
    bg, bb, bc = (b.to(F64) for b in inp["bases"])
    r = dict(dx=dx, dx_b32=b32, dx_b=b32 + (UB * dx.abs() if dtype == BF16 else 0.0),
             dgamma=bg + (dy * xhat).sum(0), dgamma_b=gam(3 + ex + depth) * ((dy * xhat).abs().sum(0) + bg.abs()),
             dbeta=bb + dy.sum(0), dbeta_b=gam(ex + depth) * (dy.abs().sum(0) + bb.abs()), xhat=xhat, dyeff=dy, depth=depth)
    if emit:
        term, tb = dx, b32
        if keep is not None:
            term = torch.where(keep, dx * scale, torch.zeros_like(dx))
            tb = torch.where(keep, b32 * scale + U * term.abs(), torch.zeros_like(dx))
            r["masked"], r["masked_b"] = term, tb + (UB * term.abs() if dtype == BF16 else 0.0)
        r["colsum"] = bc + term.sum(0)
        r["colsum_b"] = tb.sum(0) + gam(depth) * (term.abs().sum(0) + bc.abs())
    return r


def ratios_ln_bwd(out, ref):
    return {k: ratio(out[k], ref[k], ref[k + "_b"]) for k in ("dx", "dgamma", "dbeta", "colsum", "masked") if k in ref}


def check_ln_bwd(out, ref):
    return max(ratios_ln_bwd(out, ref).values())


def ln_fp32(inp, accumulate, keep_dy=None, scale_dy=1.0, emit=False, keep=None, scale=1.0, keep_y=None, scale_y=1.0):
    """An honest fp32 LayerNorm, forward and backward, in torch.float32 and torch's summation order -> (fwd outputs,
    bwd outputs given the fp32-rounded reference statistics): what the bounds must admit."""
    x, dy, g, b, dtype = inp["x"].float(), inp["dy"].float(), inp["gamma"], inp["beta"], inp["dtype"]
    mean = x.mean(-1)
    d = x - mean[:, None]
    rstd = 1.0 / torch.sqrt((d * d).mean(-1) + np.float32(LN_EPS))
    y = d * rstd[:, None] * g + b
    if keep_y is not None:
        y = torch.where(keep_y, y * np.float32(scale_y), torch.zeros_like(y))
    fwd = dict(y=to_dtype(y, dtype), mean=mean, rstd=rstd)
    ref = ln_fwd_ref(inp)
    m32, r32 = ref["mean"].float(), ref["rstd"].float()
    if keep_dy is not None:
        dy = torch.where(keep_dy, dy * np.float32(scale_dy), torch.zeros_like(dy))
    xh = (x - m32[:, None]) * r32[:, None]
    gg = dy * g
    dx = r32[:, None] * (gg - gg.mean(-1, keepdim=True) - xh * (gg * xh).mean(-1, keepdim=True))
    if accumulate:
        dx = dx + inp["old"].float()
    bwd = dict(dx=to_dtype(dx, dtype), dgamma=inp["bases"][0] + (dy * xh).sum(0), dbeta=inp["bases"][1] + dy.sum(0))
    if emit:
        term = dx
        if keep is not None:
            term = torch.where(keep, dx * np.float32(scale), torch.zeros_like(dx))
            bwd["masked"] = to_dtype(term, dtype)
        bwd["colsum"] = inp["bases"][2] + term.sum(0)
    return fwd, bwd, (m32, r32)


# ================================================================================================= cross-entropy
XENT_B, XENT_S = 2, 5   # 8 scored rows, 2 last-position rows
XREG_SLOTS, XLDS_SLOTS = 17, 9
XENT_ONCHIP_MAX_LD = 256 * 8 * (XREG_SLOTS + XLDS_SLOTS)   # 53248
# (V, ld).  On-chip bf16 kernel: one chunk; 2047 / 2048 / 2049 around slot 0's last column; 34815 / 34817 around the
# register / LDS seam (17 slots * 2048); the step's own; a ragged and a full last LDS slot.  Then the generic bf16 kernel.
XENT_BF16 = [(5, 8), (2047, 2048), (2048, 2048), (2049, 2056), (34815, 34816), (34817, 34824), (51865, 51904), (53241, 53248),
             (53248, 53248), (53250, 53256)]
XENT_F32 = [(5, 8), (1021, 1024), (53250, 53252)]
XENT_TARGETS = [0, 7, 8, -1, 2047, 2048, 34815, 34816]   # -1: V - 1; chunk edges, slot edge, the register / LDS seam
XENT_KINDS = ["normal", "equal", "dom-target", "dom-other", "spread"]
XENT_EQUAL_VALUE = 1.5
XENT_LM_D = 64


def xent_kernel_kind(V, ld, dtype):
    if dtype == F32:
        return "fp32"
    return "onchip" if ld <= XENT_ONCHIP_MAX_LD else "generic"


def xent_grad_scale(kind):
    """1 / (B (S - 1)), the reference's reduce_mean; the "spread" class under a loss scale of 2^16, so that its smallest
    gradient, exp(-77) / 8 unscaled, stays above TINY."""
    return (65536.0 if kind == "spread" else 1.0) / (XENT_B * (XENT_S - 1))


def xent_targets(V):
    """Target column of each of the 8 scored rows: the listed columns that fit under V, in turn."""
    cols = []
    for c in XENT_TARGETS:
        c = V - 1 if c < 0 else c
        if c < V and c not in cols:
            cols.append(c)
    n = XENT_B * (XENT_S - 1)
    return [cols[i % len(cols)] for i in range(n)]


def xent_inputs(V, ld, dtype, kind="normal"):
    """-> logits [B*S, ld] in ``dtype`` (pad columns and last-position rows NaN), labels [B, S] int32, the scored rows'
    indices and targets."""
    B, S = XENT_B, XENT_S
    rows = [b * S + t for b in range(B) for t in range(S - 1)]
    tg = xent_targets(V)
    labels = torch.zeros((B, S), dtype=torch.int32)
    for r, c in zip(rows, tg):
        labels[r // S, r % S + 1] = c
    n = len(rows)
    if kind == "normal":
        z = randn((n, V), 31, 2.0)
    elif kind == "equal":
        z = torch.full((n, V), XENT_EQUAL_VALUE, dtype=F64)
    elif kind in ("dom-target", "dom-other"):
        z = randn((n, V), 32, 0.01)
        for i, c in enumerate(tg):
            z[i, c if kind == "dom-target" else (c + 9) % V] += 20.0
    else:
        g = torch.Generator().manual_seed(33)
        z = torch.rand((n, V), generator=g, dtype=F64) * 70.0 - 60.0
    logits = torch.full((B * S, ld), NAN, dtype=F32)
    logits[rows, :V] = z.float()
    if dtype == BF16:
        full = torch.full((B * S, ld), NAN, dtype=BF16)
        full[rows, :V] = bf16_rne(z.float())
        logits = full
    return dict(logits=logits, labels=labels, rows=rows, targets=tg, V=V, ld=ld, dtype=dtype, kind=kind,
                grad_scale=xent_grad_scale(kind))


def xent_serial_adds(V, ld, dtype):
    """-> (a thread's serial additions, its loop iterations) for the row sum."""
    k = xent_kernel_kind(V, ld, dtype)
    if k == "onchip":
        return 8 * (XREG_SLOTS + XLDS_SLOTS), XREG_SLOTS + XLDS_SLOTS
    vec = 8 if dtype == BF16 else 4
    it = -(-(ld // vec) // 256)
    return it * vec, it


def xent_ref(inp, lm=None):
    """Shifted sparse cross-entropy in float64 -> gradient [B*S, ld] (+0 in pad columns and last-position rows), row_loss
    [B*S], their bounds.  d = z - max z, p = softmax, g = (p - onehot) gs.

    One exponential carries, relative to its value, 2 U |d| on its argument (the fp32 log2(e) constant and the fma, or the
    subtraction) and 2 U of its own (1 ulp): c1 = 2 in  c1 U (1 + |d|).  The row sum inherits the p-weighted mean of that, W,
    plus its additions: a thread's serial chain, 6 butterfly levels, 3 wave sums; the two-pass kernels also rescale a thread's
    sum when its running maximum moves (the moves add up to at most the row's range: 2 U range for the arguments of those
    exponentials and of the final exp(mx - gmx), 3 U per rescale for exp and multiply).  c2 = that sum's count + 3 (the
    reciprocal, the product, grad_scale).  Target column: + 2 U gs for p gs - gs.  bf16 output: + UB |g|.
    Row loss = max + log(sum) - z_t: the sum's relative error is absolute in the log; the on-chip kernel's fl(-max log2(e))
    shifts every exponent alike (U |max|: cancels in the gradient, not here); log 2 U |lse - max|; the two additions
    U |lse| + U |loss|:  U (sum count + |max| + 2 |lse - max| + |lse| + |loss|) <= U (sum count + 3 (|max| + |lse|) + |loss|).
    ``lm`` = (x [B*S, d], w [d, ld]) bf16: tmi_linear_xent's loss log1p(R), R = sum_{k != t} exp(z_k - zt), zt = x . w[:, t]
    in float64, with the log1p form's own bound (below)."""
    V, ld, dtype, rows, tg = inp["V"], inp["ld"], inp["dtype"], inp["rows"], inp["targets"]
    gs = float(np.float32(inp["grad_scale"]))
    z = inp["logits"][rows, :V].to(F64)
    n = len(rows)
    ar = torch.arange(n)
    tcol = torch.tensor(tg)
    m = z.max(-1).values
    d = z - m[:, None]
    lse = torch.logsumexp(z, -1)
    p = torch.exp(z - lse[:, None])
    onehot = torch.zeros_like(p)
    onehot[ar, tcol] = 1.0
    g = (p - onehot) * gs
    serial, iters = xent_serial_adds(V, ld, dtype)
    W = (p * (2.0 * d.abs() + 2.0)).sum(-1)
    cnt = W + serial + 9
    if xent_kernel_kind(V, ld, dtype) != "onchip":
        cnt = cnt + 2.0 * (m - z.min(-1).values) + 3.0 * (iters + 1)
    c2 = cnt + 3
    gb = (p * gs) * (U * (2.0 * (1.0 + d.abs()) + c2[:, None]))
    gb[ar, tcol] += 2.0 * U * gs
    if dtype == BF16:
        gb = gb + UB * g.abs()
    zt = z[ar, tcol]
    loss = lse - zt
    lb = U * (cnt + 3.0 * (m.abs() + lse.abs()) + loss.abs())
    if lm is not None:
        x, w = lm
        xw = x[rows].to(F64) * w.to(F64)[:, tcol].T               # [n, d]: the products of the target logit
        ztl = xw.sum(-1)
        dzt = gam(-(-x.shape[1] // 256) + 9) * xw.abs().sum(-1)   # a thread's fma chain, 6 butterfly levels, 3 wave sums
        others = z.clone()
        others[ar, tcol] = -math.inf
        lR = torch.logsumexp(others, -1) - ztl                    # log R
        R = torch.exp(lR)
        loss = torch.log1p(R)
        # rest = sum - e_t in the units where the largest term is 1: S = sum exp(d), e_t = exp(d_t)
        S, et = torch.exp(lse - m), torch.exp(zt - m)
        rest = (S - et).clamp_min(0.0)
        drest = U * (S * cnt + et * (2.0 * d[ar, tcol].abs() + 2.0) + rest)
        dz = m - ztl
        # exp(dz): its argument's subtraction U |dz|, exp 2 U, the product 1 U; the on-chip kernel's exponent shift U |max|;
        # d loss / d zt = -R / (1 + R); log1p 2 ulp = 4 U
        lb = (torch.exp(dz) * drest + R * U * (dz.abs() + 3.0 + m.abs())) / (1.0 + R) + dzt * R / (1.0 + R) + 4.0 * U * loss
    G = torch.zeros((XENT_B * XENT_S, ld), dtype=F64)
    GB = torch.zeros_like(G)
    G[rows, :V], GB[rows, :V] = g, gb
    L = torch.zeros(XENT_B * XENT_S, dtype=F64)
    LB = torch.zeros_like(L)
    L[rows], LB[rows] = loss, lb
    return dict(g=G, g_b=GB, loss=L, loss_b=LB, p=p, z=z, max=m, lse=lse, gs=gs, c2=c2)


def ratios_xent(out, ref):
    """out: g [B*S, ld] (the logits buffer after the call), loss [B*S].  Pad columns and last-position rows have a zero bound:
    anything but 0 there is inf; that they are +0 and not -0 is checked on the bits by the caller (xent_zero_mask)."""
    return {"g": ratio(out["g"], ref["g"], ref["g_b"]), "loss": ratio(out["loss"], ref["loss"], ref["loss_b"])}


def check_xent(out, ref):
    return max(ratios_xent(out, ref).values())


def xent_zero_mask(inp):
    """[B*S, ld] bool: the entries that must come back as +0 bit for bit."""
    mk = torch.ones((XENT_B * XENT_S, inp["ld"]), dtype=torch.bool)
    mk[inp["rows"], :inp["V"]] = False
    return mk


def xent_fp32(inp):
    """An honest fp32 cross-entropy in torch.float32 -> (g in the dtype, loss fp32)."""
    V, ld, rows, tg = inp["V"], inp["ld"], inp["rows"], inp["targets"]
    z = inp["logits"][rows, :V].float()
    gs = np.float32(inp["grad_scale"])
    m = z.max(-1, keepdim=True).values
    e = torch.exp(z - m)
    s = e.sum(-1, keepdim=True)
    g = e * (1.0 / s)
    ar = torch.arange(len(rows))
    g[ar, tg] -= 1.0
    g = g * gs
    loss = (m + torch.log(s)).squeeze(-1) - z[ar, tg]
    G = torch.zeros((XENT_B * XENT_S, ld), dtype=F32)
    G[rows, :V] = g
    L = torch.zeros(XENT_B * XENT_S, dtype=F32)
    L[rows] = loss
    return dict(g=to_dtype(G, inp["dtype"]), loss=L)


def xent_lm_operands(inp):
    """x [B*S, d], w [d, ld] bf16 whose product is ``inp``'s logits rounded once: row r reads feature r only (x[r, r] = 3) and
    w[r, :] = logits[r, :] / 3 rounded to bf16, so logits' = bf16(3 w) - the target logit is off the bf16 grid, which is what
    the entry point is for.  -> x, w, the logits the GEMM must produce (pad columns NaN through w)."""
    BS, ld, V = XENT_B * XENT_S, inp["ld"], inp["V"]
    x = torch.zeros((BS, XENT_LM_D), dtype=BF16)
    x[torch.arange(BS), torch.arange(BS)] = 3.0
    w = torch.zeros((XENT_LM_D, ld), dtype=BF16)
    z = inp["logits"].float()
    z[:, :V] = torch.nan_to_num(z[:, :V], nan=0.0)   # last-position rows: finite here, set to NaN after the GEMM
    w[:BS] = bf16_rne(z / 3.0)
    logits = bf16_rne(w[:BS].float() * 3.0)          # one product, one rounding: what the GEMM stores
    out = dict(inp)
    full = logits.clone()
    last = [r for r in range(BS) if r not in inp["rows"]]
    full[last] = NAN
    full[:, V:] = NAN
    out["logits"] = full
    return x, w, logits, out


# ================================================================================================= softmax
SM_TK = [1, 63, 64, 65, 2047, 2048]
SM_MASK_T = [1, 5, 65]          # mask 1: Tq = Tk
SM_KINDS = ["normal", "dominant", "large"]
SM_BIAS_H, SM_BIAS_TQ, SM_BIAS_B = 2, 3, 3   # H * Tq = 6: a 4-row workgroup straddles two batches


def sm_tq(Tk):
    return 1 if Tk >= 2047 else 3   # rows = 3 * Tq: 3 or 9, never a multiple of 4


def sm_inputs(rows, Tk, kind="normal", seed=41):
    s = randn((rows, Tk), seed, 3.0)
    if kind == "dominant":
        s[torch.arange(rows), (torch.arange(rows) * 7) % Tk] += 30.0
    elif kind == "large":   # |s| ~ 1e4: exp overflows without the max subtraction
        s = s + 1.0e4
    return s.float()


def sm_ref(s, Tq, mask_mode=0, key_bias=None, rows_per_batch=None, mask_shift=0):
    """Row softmax in float64 of the fp32 scores as the kernel sees them: mask 1 adds -1e9 in fp32 to keys c <= q (+ shift, for
    the mutation) as the reference model does, the bias form adds key_bias[batch] in fp32.  Bound, relative to p:
    the argument's subtraction U |d|, exp 2 U, the sum's W (p-weighted mean of |d| + 2) + 31 serial + 6 butterfly additions,
    the reciprocal and the product 2:  U p (|d| + 2 + W + 39)."""
    rows, Tk = s.shape
    x = s.clone().float()
    masked = torch.zeros((rows, Tk), dtype=torch.bool)
    if mask_mode == 1:
        q = (torch.arange(rows) % Tq)[:, None]
        masked = torch.arange(Tk)[None, :] <= q + mask_shift
        x = torch.where(masked, x + np.float32(-1e9), x)
    if key_bias is not None:
        x = x + key_bias[torch.arange(rows) // rows_per_batch]
    x = x.to(F64)
    m = x.max(-1, keepdim=True).values
    d = x - m
    p = torch.softmax(x, -1)
    W = (p * (d.abs() + 2.0)).sum(-1, keepdim=True)
    full = masked.all(-1)
    return dict(p=p, p_b=U * p * (d.abs() + 2.0 + W + 39.0), masked=masked & ~full[:, None], full=full, x=x)


def check_sm_fwd(out, ref):
    return ratio(out["p"], ref["p"], ref["p_b"])


def sm_bwd_ref(p, dp):
    """dp <- p (dp - sum p dp) of the fp32 p the kernel is given.  The dot product: products 1, 31 serial + 6 butterfly additions
    (38); dp - dot and the product 2:  U (2 p |dp| + 40 p sum |p dp|) <= 40 U (p |dp| + p sum |p dp|)."""
    p, dp = p.to(F64), dp.to(F64)
    dot = (p * dp).sum(-1, keepdim=True)
    return dict(dp=p * (dp - dot), dp_b=40.0 * U * (p * dp.abs() + p * (p * dp).abs().sum(-1, keepdim=True)))


def check_sm_bwd(out, ref):
    return ratio(out["dp"], ref["dp"], ref["dp_b"])


def sm_fp32(s, Tq, mask_mode=0, key_bias=None, rows_per_batch=None):
    x = sm_ref(s, Tq, mask_mode, key_bias, rows_per_batch)["x"].float()
    e = torch.exp(x - x.max(-1, keepdim=True).values)
    return e * (1.0 / e.sum(-1, keepdim=True))


# ================================================================================================= embedding
EMB_BS = {48: (4, 12), 65: (5, 13), 130: (10, 13), 800: (8, 100)}   # n = B * S: one ballot round (<= 64), 2, 3, the step's 13
EMB_D = [8, 264, 768]            # one column pass, two (the second of 8 columns), three
EMB_ROWS = 900                   # rows of the table
EMB_START = 6
EMB_COUNTS = {1: 1, 2: 7, 3: 8, 4: 9, 5: 17}   # id -> occurrences: below, at and above the 8-deep unrolled sum, two rounds + 1


def emb_labels(n):
    """labels [B, S] int32 in [0, EMB_ROWS): ids 1..5 occur EMB_COUNTS times among the decoder inputs, one label equals the
    start id (which every sequence's position 0 holds too), every other position holds an id of its own."""
    B, S = EMB_BS[n]
    ids = [i for i, k in EMB_COUNTS.items() for _ in range(k)] + [EMB_START]
    ids += list(range(10, 10 + B * (S - 1) - len(ids)))
    perm = torch.randperm(len(ids), generator=torch.Generator().manual_seed(51)).tolist()
    lab = torch.full((B, S), EMB_ROWS - 1, dtype=torch.int32)    # labels[:, S - 1] never reach the embedding
    lab[:, :S - 1] = torch.tensor([ids[i] for i in perm], dtype=torch.int32).reshape(B, S - 1)
    return lab


def emb_ids(labels):
    B = labels.shape[0]
    return torch.cat([torch.full((B, 1), EMB_START, dtype=torch.int64), labels[:, :-1].long()], 1).reshape(-1)


def emb_inputs(n, D, dtype):
    B, S = EMB_BS[n]
    return dict(labels=emb_labels(n), table=randn((EMB_ROWS, D), 52).float(), pe=randn((S, D), 53).float(),
                dy=to_dtype(randn((n, D), 54), dtype), B=B, S=S, D=D, n=n, dtype=dtype)


def emb_ref(inp):
    """Forward: table[id] + pe[t] is ONE fp32 addition, a bf16 output its RNE rounding: bit-exact.  Backward: dtable[id] = the
    sum of dy over the id's k occurrences, k U sum |dy| per element (k - 1 additions); rows no id names are not written."""
    ids, S, D = emb_ids(inp["labels"]), inp["S"], inp["D"]
    t = torch.arange(inp["n"]) % S
    out32 = inp["table"][ids] + inp["pe"][t]
    dy = inp["dy"].to(F64)
    dt = torch.zeros((EMB_ROWS, D), dtype=F64)
    da = torch.zeros_like(dt)
    dt.index_add_(0, ids, dy)
    da.index_add_(0, ids, dy.abs())
    k = torch.bincount(ids, minlength=EMB_ROWS).to(F64)
    return dict(out=to_dtype(out32, inp["dtype"]), out64=inp["table"].to(F64)[ids] + inp["pe"].to(F64)[t], dtable=dt,
                dtable_b=k[:, None] * U * da, touched=k > 0, count=k, ids=ids)


def check_emb_bwd(out, ref):
    """out["dtable"] [EMB_ROWS, D] fp32; untouched rows are the caller's guard pattern, compared on the bits there."""
    tz = ref["touched"]
    return ratio(out["dtable"][tz], ref["dtable"][tz], ref["dtable_b"][tz])


def emb_bwd_fp32(inp):
    ids = emb_ids(inp["labels"])
    dt = torch.zeros((EMB_ROWS, inp["D"]), dtype=F32)
    dt.index_add_(0, ids, inp["dy"].float())
    return dt


# ================================================================================================= tmi_sum_scale
SUM_N = [1, 255, 256, 257, 8000]
SUM_SCALE = 0.125   # a power of two: the final multiply is exact, as the bound (ceil(n / 256) + 8) U sum |x| assumes


def sum_inputs(n):
    return randn((n,), 61).float()


def sum_ref(x):
    n = x.numel()
    return dict(out=x.to(F64).sum() * SUM_SCALE, out_b=(-(-n // 256) + 8) * U * x.to(F64).abs().sum() * SUM_SCALE)


def check_sum(out, ref):
    return ratio(out["out"], ref["out"], ref["out_b"])
