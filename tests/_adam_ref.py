"""References for the optimizer and gradient-staging kernels (csrc/adam_misc.hip).  CPU only: nothing here imports the GPU
package, so tests/test_adam_ref_cpu.py can check these references before any kernel is compared with them.

``adam_ref``           float64 Adam with the constants the kernel really uses (see below), p / m / v / bf16 mirror
``adam_terms``         the same, with the intermediates the error bounds are built from
``adam_bounds``        analytic fp32 rounding bounds on m, v, p (derivation at the function)
``adam_restate_fp32``  the kernel's operations in the kernel's order in torch.float32 on the CPU, one rounding per operation
``clip_factors``       c_g, c_s of tmi_adam_step_segments in float64
``unpack_ref``         tmi_grad_unpack as an fp32 fold in the kernel's order (bit-exact: additions and one multiply)
``bf16_rne_bits``      round-to-nearest-even to bf16 on the bit pattern, independent of torch's conversion
``adam_inputs``        the seeded p, g, g2, m, v of the GPU tests, hard elements planted

The kernel's constants.  lr, beta1, beta2, eps, weight_decay and gscale cross the C ABI as fp32, so the reference rounds
them to fp32 first.  ``1 - beta1``, ``1 - beta2`` and ``decay = 1 - lr * weight_decay`` are formed IN fp32 (adam1 writes
``1.0f - b2``; for beta2 = 0.999 that is 9.9998713e-4, 1.3e-5 relative away from 1e-3).  step_size and vcorr_inv_sqrt are formed in double from the
fp32 betas and then rounded to fp32 (tmi_adam_scalars).  Everything per element is float64.
"""
import functools
import math

import numpy as np
import torch

U = 2.0 ** -24            # unit roundoff of fp32 (round to nearest)
DENORM = 2.0 ** -149      # absolute error floor per operation should a result fall below the normal range
SECOND_ORDER = 1.0 + 2.0 ** -18   # covers the products of two first-order terms (each at most ~25 u) and float64's own 2^-53

f32 = np.float32


def gamma(k):
    """k roundings compound to at most k u / (1 - k u) (Higham, Accuracy and Stability, lemma 3.1)."""
    return k * U / (1.0 - k * U)


def adam_constants(lr, beta1, beta2, eps, step, eps_mode, weight_decay=0.0, gscale=1.0, fp32_step_scalars=True):
    """Every scalar of one step as the kernel holds it, widened back to Python floats."""
    lr, b1, b2, eps, wd, gs = (f32(x) for x in (lr, beta1, beta2, eps, weight_decay, gscale))
    omb1 = f32(1.0) - b1
    omb2 = f32(1.0) - b2
    decay = f32(1.0) - lr * wd          # fp32 product, fp32 subtraction
    c1 = 1.0 - float(b1) ** step
    c2 = 1.0 - float(b2) ** step
    if eps_mode == 0:
        step_size, vcorr = float(lr) * math.sqrt(c2) / c1, 1.0
    else:
        step_size, vcorr = float(lr) / c1, 1.0 / math.sqrt(c2)
    if fp32_step_scalars:
        step_size, vcorr = float(f32(step_size)), float(f32(vcorr))
    return dict(b1=float(b1), b2=float(b2), omb1=float(omb1), omb2=float(omb2), eps=float(eps), decay=float(decay),
                gscale=float(gs), step_size=step_size, vcorr=vcorr, eps_mode=int(eps_mode))


def bf16_rne_bits(x32):
    """fp32 tensor -> int32 tensor holding the 16 bits of bf16(x), round to nearest, ties to even (no NaN inputs)."""
    bits = x32.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    return ((bits + 0x7FFF + ((bits >> 16) & 1)) >> 16).to(torch.int32)


def bf16_bits(xbf):
    return xbf.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF


def adam_terms(p, g, m, v, *, lr, beta1, beta2, eps, step, eps_mode, weight_decay=0.0, gscale=1.0, gfactor=None,
               fp32_step_scalars=True):
    """One step in float64.  ``gfactor`` (float64, per element) multiplies g beside gscale: the clip factors of
    tmi_adam_step_segments.  Returns the results and the magnitudes ``adam_bounds`` needs."""
    c = adam_constants(lr, beta1, beta2, eps, step, eps_mode, weight_decay, gscale, fp32_step_scalars)
    p, g, m, v = (t.detach().double().cpu() for t in (p, g, m, v))
    gp = g * c["gscale"]
    if gfactor is not None:
        gp = gp * gfactor
    m_a, m_b = c["b1"] * m, c["omb1"] * gp
    m1 = m_a + m_b
    v1 = c["b2"] * v + c["omb2"] * gp * gp
    pd = p * c["decay"]
    den = v1.sqrt() * c["vcorr"] + c["eps"]     # vcorr == 1 in mode 0
    upd = c["step_size"] * m1 / den
    p1 = pd - upd
    return dict(p=p1, m=m1, v=v1, m_a=m_a, m_b=m_b, pd=pd, den=den, upd=upd, c=c)


def adam_ref(p, g, m, v, *, lr, beta1, beta2, eps, step, eps_mode, weight_decay=0.0, gscale=1.0, fp32_step_scalars=True):
    """(p, m, v, mirror) after one step: float64 tensors and the bf16 mirror of p.  ``fp32_step_scalars=False`` keeps
    step_size / vcorr_inv_sqrt in double: textbook Adam on the fp32 hyper-parameters, for the comparisons with the project's
    oracle and torch.optim, which never round them."""
    t = adam_terms(p, g, m, v, lr=lr, beta1=beta1, beta2=beta2, eps=eps, step=step, eps_mode=eps_mode,
                   weight_decay=weight_decay, gscale=gscale, fp32_step_scalars=fp32_step_scalars)
    return t["p"], t["m"], t["v"], t["p"].float().to(torch.bfloat16)


def adam_bounds(t, kg=1):
    """Per-element bounds on |kernel - float64| for m, v, p after ONE step from exactly shared inputs.

    Rounding counts of adam1 (every fp32 +, *, /, sqrtf rounds once, relative error <= u = 2^-24; hipcc rounds fp32 divide
    and sqrtf correctly by default; adam1's three fmaf each REMOVE a rounding, so the counts are upper limits and a plain
    evaluation without fused operations obeys them too).  The
    constants b1, 1-b1, b2, 1-b2, eps, decay, step_size, vcorr_inv_sqrt are the same fp32 values on both sides: no error.

      g' = g * scale                                           kg roundings (1 for the flat kernel: the one multiply)
      m  = b1*m + (1-b1)*g'     b1*m: 1, (1-b1)*g': kg + 1, the addition: 1 on both
           -> |dm| <= gamma(kg + 2) * (|b1 m| + |(1-b1) g'|)                                         k_m = kg + 2 = 3
      v  = b2*v + ((1-b2)*g')*g'   second term: g' twice (2 kg), two multiplies, the addition: 2 kg + 3; b2*v: 2; all terms
           are non-negative, so the error is relative to v itself
           -> |dv| <= gamma(2 kg + 3) * v                                                            k_v = 2 kg + 3 = 5
      p  = p*decay - (step_size*m) / (sqrtf(v) [* vcorr] + eps)
           p*decay: 1, then the subtraction: 2.  update: multiply 1, sqrtf 1, [vcorr multiply 1,] + eps 1, divide 1, the
           subtraction 1: 5 in mode 0, 6 in mode 1                                                   k_p = 5 | 6
           carried in: the kernel's update is built on ITS m and v.  dm enters linearly: step_size * |dm| / den (written
           absolutely rather than |update| * |dm| / |m|, the same number, because m may be 0 or a cancelled sum); a relative
           error e in v is e/2 in sqrtf(v), and no more than that in the denominator, eps >= 0 only diluting it.
           -> |dp| <= gamma(k_p) * (|p decay| + |update|) + step_size * bound_m / den + |update| * gamma(k_v) / 2
    Each bound is multiplied by SECOND_ORDER and given k * 2^-149 for gradual underflow (the inputs keep clear of it).
    """
    c = t["c"]
    k_m, k_v, k_p = kg + 2, 2 * kg + 3, (5 if c["eps_mode"] == 0 else 6)
    bm = gamma(k_m) * (t["m_a"].abs() + t["m_b"].abs())
    bv = gamma(k_v) * t["v"]
    carried = c["step_size"] * bm / t["den"] + t["upd"].abs() * gamma(k_v) / 2
    bp = gamma(k_p) * (t["pd"].abs() + t["upd"].abs()) + carried
    return dict(m=bm * SECOND_ORDER + k_m * DENORM, v=bv * SECOND_ORDER + k_v * DENORM, p=bp * SECOND_ORDER + k_p * DENORM,
                k=(k_m, k_v, k_p))


def bound_fraction(got, ref, bound):
    """max over elements of |got - ref| / bound (0 where both are 0): what goes through _margins.within against 1.0."""
    err = (got.detach().double().cpu() - ref).abs()
    frac = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(frac.max())


def adam_restate_fp32(p, g, m, v, *, lr, beta1, beta2, eps, step, eps_mode, weight_decay=0.0, gscale=1.0):
    """adam1 of csrc/adam_misc.hip, operation by operation in torch.float32 on the CPU: every tensor operation below rounds
    once and nothing is fused.  Returns fp32 (p, m, v, mirror)."""
    c = adam_constants(lr, beta1, beta2, eps, step, eps_mode, weight_decay, gscale)
    k = {n: torch.tensor(x, dtype=torch.float32) for n, x in c.items() if n != "eps_mode"}   # exact: all are fp32 values
    p, g, m, v = (t.detach().float().cpu().clone() for t in (p, g, m, v))
    g = g * k["gscale"]
    m = k["b1"] * m + k["omb1"] * g
    v = k["b2"] * v + (k["omb2"] * g) * g
    p = p * k["decay"]
    if eps_mode == 0:
        p = p - (k["step_size"] * m) / (v.sqrt() + k["eps"])
    else:
        p = p - (k["step_size"] * m) / (v.sqrt() * k["vcorr"] + k["eps"])
    return p, m, v, p.to(torch.bfloat16)


def clip_factors(sumsq, seg, clip_global, clip_each):
    """c_g and c_s[seg] of tmi_adam_step_segments in float64.  ``sumsq``: per-variable sums of squares of the raw gradients;
    ``seg``: int64 variable index per element (or per anything else): the per-variable factor is gathered through it."""
    ss = torch.as_tensor(sumsq).detach().double().cpu()
    c_g = 1.0
    if clip_global > 0:
        c_g = clip_global / max(math.sqrt(float(ss.sum())), clip_global)
    c_s = torch.ones_like(ss)
    if clip_each > 0:
        c_s = clip_each / torch.clamp(c_g * ss.sqrt(), min=clip_each)
    return c_g, c_s[torch.as_tensor(seg).long().cpu()]


def unpack_ref(src, nparts, part_stride, n, scale):
    """dst[i] = scale * (((0 + src[0*stride + i]) + src[1*stride + i]) + ...) in fp32, the kernel's order.  ``src``: flat
    fp32 or bf16 CPU tensor (bf16 widens exactly)."""
    s = src.detach().cpu()
    acc = torch.zeros(n, dtype=torch.float32)
    for q in range(nparts):
        acc = acc + s[q * part_stride:q * part_stride + n].float()
    return acc * torch.tensor(float(f32(scale)), dtype=torch.float32)


# ------------------------------------------------------------------------------------------------ the GPU tests' inputs
WRAPPED_N = 2 * 512 * 1024 + 4 * 300 + 3     # just over twice the 512-workgroup cap of tmi_adam_step: third grid-stride trip
ADAM_NS = (1, 3, 4, 1027, 4 * 256 * 3 + 2, WRAPPED_N)
HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-7)    # beta2 = 0.999: 1.0f - b2 is NOT 0.001f

# planted element classes, by (5 i + 7) % 16 so that even n = 3 gets a mix; everything else is Gaussian
ZERO_TIE_EVEN, ZERO_TIE_ODD, G_HUGE, G_TINY, V_LARGE_M_TINY = 0, 1, 2, 3, 4


def element_class(n):
    return (torch.arange(n, dtype=torch.int64) * 5 + 7) % 16


@functools.lru_cache(maxsize=None)
def adam_inputs(n, seed=1234):
    """fp32 CPU tensors p, g, g2 (the second step's gradient), m, v; drawn once per n and never modified (callers clone).
      ZERO_TIE_*       g = m = v = 0: the update is exactly 0, p only decays.  p there has the fp32 low half 0x8000, i.e.
                       its bf16 rounding is a tie, upper half even / odd, both signs: pins the mirror's ties-to-even
      G_HUGE / G_TINY  |g| = 1e4 / 1e-12
      V_LARGE_M_TINY   v = 1e6, m = +-1e-20
    Gaussian p has both signs; v >= 0 everywhere."""
    gen = torch.Generator().manual_seed(seed + n)
    r = lambda s: (torch.randn(n, generator=gen, dtype=torch.float64) * s).float()
    p, g, g2, m, v = r(1.0), r(0.02), r(0.02), r(0.01), r(0.01).abs()
    cls = element_class(n)
    sign = torch.where(torch.arange(n) % 2 == 0, 1.0, -1.0).float()
    for which, parity in ((ZERO_TIE_EVEN, 0), (ZERO_TIE_ODD, 1)):
        sel = cls == which
        hi = ((p.view(torch.int32).to(torch.int64) & 0xFFFFFFFF) >> 16 & 0xFFFE) | parity
        bits = (hi << 16) | 0x8000
        tie = torch.where(bits >= 2 ** 31, bits - 2 ** 32, bits).to(torch.int32).view(torch.float32)
        p = torch.where(sel, tie, p)
        g, m, v = (torch.where(sel, torch.zeros_like(t), t) for t in (g, m, v))
    g = torch.where(cls == G_HUGE, 1e4 * sign, g)
    g = torch.where(cls == G_TINY, 1e-12 * sign, g)
    g2 = torch.where(cls == G_HUGE, -1e4 * sign, g2)
    sel = cls == V_LARGE_M_TINY
    v = torch.where(sel, torch.full_like(v, 1e6), v)
    m = torch.where(sel, 1e-20 * sign, m)
    return tuple(t.contiguous() for t in (p, g, g2, m, v))


def adam_cases():
    """(n, eps_mode, weight_decay, gscale, step, zero_grad): the pruned product of the GPU test.  Each n gets six cases in
    which every value of every axis appears (eps_mode 0/1, decay off/on, step 1/2/1000, zero_grad off/on); the rows are
    rotated with n so that the pairings differ from one length to the next."""
    rows = [(0, 0, 1, False), (1, 1, 2, True), (0, 1, 1000, True), (1, 0, 1000, False), (0, 1, 2, False), (1, 0, 1, True)]
    wdg = ((0.0, 1.0), (0.1, 0.125))
    steps = (1, 2, 1000)
    out = []
    for i, n in enumerate(ADAM_NS):
        for mode, w, step, zg in rows:
            step = steps[(steps.index(step) + i) % 3]
            out.append((n, mode, wdg[w][0], wdg[w][1], step, bool(zg) ^ bool(i & 1)))
    return out
