"""Float64 reference, seeded inputs and bounds for the classification-head kernels (csrc/cls_head.hip: tmi_cls_head_fwd,
tmi_cls_head_bwd), written literally from the definitions in include/tethys_mi.h.  CPU only: nothing here imports the GPU
package, so tests/test_cls_cpu.py checks the reference (gradients against central finite differences, closed forms) before
tests/test_cls_kernels_gpu.py and tests/test_cls_gpu.py compare a kernel with it.  Keras Adam in float64 is
``_adam_ref.adam_terms`` (eps_mode 0), the dropout mask is ``oracle.dropout.keep_flat`` under
``site_seed(base, step, SITE_CLS)``.

The bounds are derived, not fitted.  U = 2^-24 is the unit roundoff of an fp32 operation; gam(n) = n U / (1 - n U) bounds a
chain of n roundings (Higham, lemma 3.1).  The device's tanhf / expf / logf are the ROCm device library's.  No accuracy
table of that library is installed beside the compiler, so, as tests/_ctc_ref.py does, this is stated as an ASSUMPTION:
the library meets the OpenCL C accuracy requirements - 5 ulp for tanh, 3 ulp for exp, 3 ulp for log in fp32 (an ulp is at
most 2^-23 of the value).  Every magnitude is taken from the float64 reference; (1 + SLACK) covers second-order terms.

Forward, per row (inputs are the same fp32 numbers on both sides: no input error):
  pre[c]    H fused multiply-adds from 0, then + bp:   E_pre = gam(H + 1) (sum_h |x_h Wp_hc| + |bp_c|)
  z         tanh' = 1 - tanh^2 <= min(1, 1 - z^2 + 2 E_pre) between the two arguments:
            E_z = E_pre min(1, 1 - z^2 + 2 E_pre) + C_TANH |z|
  y         z * scale, one rounding (p = 0: none), or an exact 0:   E_y = scale E_z + U |y|
  logits[k] P fused multiply-adds, then + bc:  E_l = sum_c E_y |Wc_ck| + gam(P + 1) (sum_c |y_c Wc_ck| + |bc_k|)
  lse       log-sum-exp is non-expansive in the sup norm: max_k E_l carries over.  Its own roundings, with d_k = l_k - m
            and S = sum exp(d_k) >= 1:  d_k rounds once (the sum moves by U sum |d_k| exp(d_k)), exp C_EXP relative, a term
            passes through at most ceil(C / 64) + 6 additions (the lane's running sum, six butterfly steps), log turns a
            relative error r of S into r (1 + r) absolute plus C_LOG |log S|, m + log S rounds once:
            E_lse = max_k E_l + r (1 + r) + C_LOG |log S| + U |lse|,  r = U sum|d| e^d / S + C_EXP + gam(ceil(C / 64) + 6)
  log_probs l_k - lse rounds once:  E_lp = E_l[k] + E_lse + U |log_probs_k|;  nll likewise at the label.
  pred / label_rank are integers: compared only where the float64 logits separate them by more than 2 max_k E_l
  (``decided``); the planted exact ties are compared everywhere.

Backward (from the DEVICE's z and log_probs: E_z and E_lp above are their errors), inv = 1 / n_valid:
  dl[k]     (expf(lp_k) - 1[k = label]) * inv:  p_k = exp(lp_k) moves by p_k (e^{E_lp} - 1), expf C_EXP p_k, the subtraction,
            the division 1 / n and the product one rounding each:  E_dl = (p_k (e^{E_lp} - 1) + C_EXP p_k + 3 U |p_k - 1[.]|) inv
  gbc[k]    N additions:  sum_r E_dl + gam(N) sum_r |dl|
  gWc[c][k] N fused multiply-adds:  sum_r (E_y |dl| + |y| E_dl + E_y E_dl) + gam(N) sum_r |y dl|
  dy[c]     C fused multiply-adds:  E_dy = sum_k E_dl |Wc_ck| + gam(C) sum_k |dl_k Wc_ck|
  t         dy * scale or 0:  E_t = scale E_dy + U |t|
  f         fmaf(-z, z, 1) = 1 - z^2, one rounding:  E_f = 2 |z| E_z + E_z^2 + U |f|
  dpre      t * f:  E_dpre = E_t |f| + |t| E_f + E_t E_f + U |dpre|
  gbp[c]    sum_r E_dpre + gam(N) sum_r |dpre|;   gWp[h][c]   sum_r |x_h| E_dpre + gam(N) sum_r |x_h dpre|
  loss      sum of N values of -lp (error E_lp each) through at most ceil(N / 256) + 9 additions, one division:
            (sum_r E_lp + gam(ceil(N / 256) + 9) sum_r |nll|) / n + 2 U |loss|
"""
import math

import numpy as np

from oracle import dropout as D

U = 2.0 ** -24
TANH_ULPS, EXP_ULPS, LOG_ULPS = 5, 3, 3
C_TANH, C_EXP, C_LOG = TANH_ULPS * 2.0 ** -23, EXP_ULPS * 2.0 ** -23, LOG_ULPS * 2.0 ** -23
SLACK = 2.0 ** -10
DENORM = 2.0 ** -126   # an absolute floor per bound: results below the normal range round absolutely, not relatively
SITE_CLS = 5


def gam(n):
    return n * U / (1.0 - n * U)


def f64(a):
    return np.asarray(a, dtype=np.float64)


def keep_mask(base_seed, step, rows, cols, p):
    """(keep bool [rows, cols], scale) of the head's dropout site in step ``step``; p = 0: everything kept, scale 1."""
    if p == 0.0:
        return np.ones((rows, cols), dtype=bool), 1.0
    return D.keep_flat(D.site_seed(base_seed, step, SITE_CLS), rows, cols, p), D.keep_scale(p)


def keep_mask_seed(seed, rows, cols, p):
    """The same for a kernel call that is given ``seed`` itself."""
    if p == 0.0:
        return np.ones((rows, cols), dtype=bool), 1.0
    return D.keep_flat(seed, rows, cols, p), D.keep_scale(p)


def label_rank(logits, labels):
    """#classes strictly above the label's logit + #equal logits at a lower index; -1 for a label outside [0, C)."""
    logits = f64(logits)
    N, C = logits.shape
    out = np.full(N, -1, dtype=np.int64)
    for r in range(N):
        lab = int(labels[r])
        if 0 <= lab < C:
            ll = logits[r, lab]
            out[r] = int((logits[r] > ll).sum() + (logits[r, :lab] == ll).sum())
    return out


def forward(x, Wp, bp, Wc, bc, labels=None, keep=None, scale=1.0):
    """Float64 forward of N rows -> dict(pre, z, y, logits, lse, log_probs, pred, nll, label_rank, valid)."""
    x, Wp, bp, Wc, bc = (f64(t) for t in (x, Wp, bp, Wc, bc))
    N, C = x.shape[0], Wc.shape[1]
    pre = x @ Wp + bp
    z = np.tanh(pre)
    y = z.copy() if keep is None else np.where(keep, z * scale, 0.0)
    logits = y @ Wc + bc
    m = logits.max(axis=1, keepdims=True)
    S = np.exp(logits - m).sum(axis=1, keepdims=True)
    lse = m + np.log(S)
    logp = logits - lse
    pred = np.argmax(logits, axis=1)   # (the first maximum: the lowest index on ties)
    lab = np.full(N, -1, dtype=np.int64) if labels is None else np.asarray(labels, dtype=np.int64)
    valid = (lab >= 0) & (lab < C)
    nll = np.where(valid, -logp[np.arange(N), np.where(valid, lab, 0)], 0.0)
    return dict(pre=pre, z=z, y=y, logits=logits, lse=lse[:, 0], S=S[:, 0], m=m[:, 0], log_probs=logp, pred=pred, nll=nll,
                label_rank=label_rank(logits, lab), valid=valid, labels=lab)


def loss_of(x, Wp, bp, Wc, bc, labels, keep=None, scale=1.0):
    f = forward(x, Wp, bp, Wc, bc, labels, keep, scale)
    n = int(f["valid"].sum())
    return float(f["nll"].sum() / n) if n else 0.0


def backward(x, Wc, f, keep=None, scale=1.0):
    """Float64 gradients of loss = sum over the labelled rows of nll / n_valid, from ``forward``'s dict ->
    dict(loss, n_valid, dl, dy, dpre, gWp, gbp, gWc, gbc)."""
    x, Wc = f64(x), f64(Wc)
    N, C = f["logits"].shape
    n = int(f["valid"].sum())
    inv = 1.0 / n if n else 0.0
    onehot = np.zeros((N, C))
    onehot[np.arange(N)[f["valid"]], f["labels"][f["valid"]]] = 1.0
    dl = np.where(f["valid"][:, None], (np.exp(f["log_probs"]) - onehot) * inv, 0.0)
    dy = dl @ Wc.T
    t = dy.copy() if keep is None else np.where(keep, dy * scale, 0.0)
    fz = 1.0 - f["z"] ** 2
    dpre = t * fz
    return dict(loss=float(f["nll"].sum() * inv), n_valid=n, inv=inv, dl=dl, dy=dy, t=t, fz=fz, dpre=dpre, gWp=x.T @ dpre,
                gbp=dpre.sum(axis=0), gWc=f["y"].T @ dl, gbc=dl.sum(axis=0), onehot=onehot)


def forward_bounds(x, Wp, bp, Wc, bc, f, keep=None, scale=1.0):
    """Per-element bounds on |device - float64| of the forward outputs (derivation at the top of the file)."""
    ax, aWp, aWc = np.abs(f64(x)), np.abs(f64(Wp)), np.abs(f64(Wc))
    H, P = aWp.shape
    C = aWc.shape[1]
    E_pre = gam(H + 1) * (ax @ aWp + np.abs(f64(bp)))
    z = f["z"]
    E_z = E_pre * np.minimum(1.0, 1.0 - z * z + 2.0 * E_pre) + C_TANH * np.abs(z)
    E_y = E_z if keep is None else np.where(keep, scale * E_z + U * np.abs(f["y"]), 0.0)   # (a dropped element is an exact 0)
    E_l = E_y @ aWc + gam(P + 1) * (np.abs(f["y"]) @ aWc + np.abs(f64(bc)))
    d = f["logits"] - f["m"][:, None]
    r = U * (np.abs(d) * np.exp(d)).sum(axis=1) / f["S"] + C_EXP + gam(math.ceil(C / 64) + 6)
    E_lse = E_l.max(axis=1) + r * (1.0 + r) + C_LOG * np.abs(np.log(f["S"])) + U * np.abs(f["lse"])
    E_lp = E_l + E_lse[:, None] + U * np.abs(f["log_probs"])
    N = z.shape[0]
    lab = np.where(f["valid"], f["labels"], 0)
    E_nll = np.where(f["valid"], E_lp[np.arange(N), lab], 0.0)
    k = 1.0 + SLACK
    return dict(pre=E_pre * k + DENORM, z=E_z * k + DENORM, y=E_y * k + DENORM, logits=E_l * k + DENORM, lse=E_lse * k + DENORM,
                log_probs=E_lp * k + DENORM, nll=E_nll * k + DENORM)


def decided(f, fb):
    """Rows whose ``pred`` and ``label_rank`` the float64 logits decide beyond the device's error: the top-two gap (pred)
    and the label's distance to every other logit (label_rank) exceed twice the row's largest logit bound.
    -> (pred_decided bool [N], rank_decided bool [N]; unlabelled rows count as decided: their rank is -1)."""
    lg = f["logits"]
    N, C = lg.shape
    e2 = 2.0 * fb["logits"].max(axis=1)
    if C == 1:
        return np.ones(N, dtype=bool), np.ones(N, dtype=bool)
    top = np.sort(lg, axis=1)
    pd = (top[:, -1] - top[:, -2]) > e2
    rd = np.ones(N, dtype=bool)
    for r in range(N):
        if f["valid"][r]:
            lab = int(f["labels"][r])
            gap = np.abs(np.delete(lg[r], lab) - lg[r, lab]).min()
            rd[r] = gap > e2[r]
    return pd, rd


def backward_bounds(x, Wc, f, g, fb, keep=None, scale=1.0):
    """Per-element bounds on |device - float64| of loss, dpre and the four gradients (derivation at the top of the file)."""
    ax, aWc = np.abs(f64(x)), np.abs(f64(Wc))
    N, C = f["logits"].shape
    inv, n = g["inv"], g["n_valid"]
    valid = f["valid"][:, None]
    p = np.exp(f["log_probs"])
    E_lp = fb["log_probs"]
    E_dl = np.where(valid, (p * np.expm1(E_lp) + C_EXP * p + 3.0 * U * np.abs(p - g["onehot"])) * inv, 0.0)
    adl, ay = np.abs(g["dl"]), np.abs(f["y"])
    E_y = fb["y"]
    B_gbc = E_dl.sum(axis=0) + gam(N) * adl.sum(axis=0)
    B_gWc = E_y.T @ adl + ay.T @ E_dl + E_y.T @ E_dl + gam(N) * (ay.T @ adl)
    E_dy = E_dl @ aWc.T + gam(C) * (adl @ aWc.T)
    E_t = E_dy if keep is None else np.where(keep, scale * E_dy + U * np.abs(g["t"]), 0.0)   # (a dropped element is an exact 0)
    az, E_z = np.abs(f["z"]), fb["z"]
    E_f = 2.0 * az * E_z + E_z * E_z + U * np.abs(g["fz"])
    adp = np.abs(g["dpre"])
    E_dp = E_t * np.abs(g["fz"]) + np.abs(g["t"]) * E_f + E_t * E_f + U * adp
    B_gbp = E_dp.sum(axis=0) + gam(N) * adp.sum(axis=0)
    B_gWp = ax.T @ E_dp + gam(N) * (ax.T @ adp)
    B_loss = ((fb["nll"].sum() + gam(math.ceil(N / 256) + 9) * np.abs(f["nll"]).sum()) * inv + 2.0 * U * abs(g["loss"])) if n else 0.0
    k = 1.0 + SLACK
    return dict(loss=B_loss * k + DENORM, dpre=E_dp * k + DENORM, gWp=B_gWp * k + DENORM, gbp=B_gbp * k + DENORM,
                gWc=B_gWc * k + DENORM, gbc=B_gbc * k + DENORM)


def ratio(got, ref, bound):
    """max over elements of |got - ref| / bound; an element equal to its reference counts 0, a NaN counts inf."""
    got, ref = f64(got).reshape(-1), f64(ref).reshape(-1)
    bound = np.broadcast_to(f64(bound).reshape(-1) if np.ndim(bound) else np.float64(bound), ref.shape)
    if got.size == 0:
        return 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(got - ref)
        q = np.where(err == 0.0, 0.0, err / bound)
    q = np.where(np.isnan(q), np.inf, q)
    return float(q.max())


def head_inputs(N, H, P, C, seed, n_src=None, scale_x=1.0):
    """Seeded fp32 inputs of one kernel call: pooled [n_src, H], Keras-like weights, labels with some -1 among them."""
    rng = np.random.default_rng(seed)
    n_src = n_src or N
    x = (rng.standard_normal((n_src, H)) * scale_x).astype(np.float32)
    Wp = (rng.uniform(-1, 1, (H, P)) * math.sqrt(6.0 / (H + P))).astype(np.float32)
    bp = (rng.standard_normal(P) * 0.1).astype(np.float32)
    Wc = (rng.uniform(-1, 1, (P, C)) * math.sqrt(6.0 / (P + C)) * 2.0).astype(np.float32)
    bc = (rng.standard_normal(C) * 0.1).astype(np.float32)
    labels = rng.integers(0, C, N).astype(np.int32)
    if N >= 3:
        labels[rng.integers(0, N)] = -1
    return dict(x=x, Wp=Wp, bp=bp, Wc=Wc, bc=bc, labels=labels)
