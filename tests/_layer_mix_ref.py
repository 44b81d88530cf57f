"""Float64 reference, seeded cases, bounds and mutations for the layer-mix kernels (csrc/layer_mix.hip: tmi_layer_mix_fwd,
tmi_layer_mix_bwd) and for the whole mixed head step (mix, head forward, tmi_ctc_posteriors, head backward, mix backward),
written literally from the definitions in include/tethys_mi.h on top of ``_ctc_head_ref`` / ``_ctc_post_ref``.  CPU only:
nothing here imports the GPU package, so tests/test_layer_mix_cpu.py checks the reference (torch's float64 autograd through
softmax, the stacked sum, linear, log_softmax and ctc_loss; central differences on the logits) and the bounds (reachable by
an honest fp32 transcription, exceeded by every listed mutation) before tests/test_layer_mix_kernels_gpu.py and
tests/test_layer_mix_gpu.py compare a kernel with it.  The dropout mask is ``oracle.dropout.keep_flat`` through
``_ctc_head_ref.keep_masks``, keyed by the position n * T_max + t in the call.

The bounds are derived, not fitted, from the constants of ``_ctc_ref`` (U = 2^-24, gam(n) = n U / (1 - n U), C_EXP, SLACK).
Inputs are the same fp32 or bf16 numbers on both sides; a bf16 input is exact in fp32 and contributes no term.
  w         d_k = a_k - m rounds once: expf sees an argument off by U |d_k|, a relative error U |d_k| of e_k, beside its own
            C_EXP:  r_k = C_EXP + U |d_k|.  s = e_0 + .. + e_{K-1}: K - 1 additions of positive terms that carry r_k each:
            r_s = sum_k w_k r_k + gam(K - 1).  w_k = e_k / s rounds once:  E_w[k] = w_k (r_k + r_s + U).  An e_k below the
            smallest normal number may be flushed: the absolute floor DENORM covers it (s >= 1).
  mixed     K fused multiply-adds from 0 (the first rounds the product): gam(K) sum_k |w_k x_k|, and the weights' own error
            sum_k E_w[k] |x_k|.
  d         gs = grad * w_n: 2 roundings (``_ctc_head_ref``); dx: V fused multiply-adds from 0 and the product with the scale
            (1 more; none at p = 0, charged anyway); then dx * x_k enters a sum in which it passes through at most
            ``chain_depth`` roundings - the thread's chain, 6 butterfly steps, 3 wave additions, the lane's chain over the
            tiles and 6 more butterfly steps, all read off the partition the header states:
            E_d[k] = gam(V + 3 + chain_depth) sum_{r, h} scale (sum_v |gs[r][v] W[h][v]|) |x_k[r][h]|.
  g_a       dot = K fused multiply-adds of w_j d_j: E_dot = sum_j (E_w[j] |d_j| + w_j E_d[j]) + gam(K) sum_j |w_j d_j|;
            diff = d_k - dot rounds once: E_diff = E_d[k] + E_dot + U |diff|;  g_a[k] = w_k diff rounds once:
            E_g[k] = w_k E_diff + E_w[k] |diff| + U |g_a[k]|.
Every bound gets the factor (1 + SLACK) and the absolute floor DENORM = 2^-126.
"""
import math

import numpy as np

import _ctc_head_ref as R
import _ctc_ref as C

U, SLACK, gam, C_EXP = C.U, C.SLACK, C.gam, C.C_EXP
DENORM = R.DENORM
f64 = R.f64
TILE_ROWS = 8        # include/tethys_mi.h: the row tile up to N * T_max = 8192
MAX_TILES = 1024

MUTATIONS = ["no_jacobian_mean",   # g_a = w_k d_k: the Jacobian's - sum_j w_j d_j term dropped
             "unnormalised",       # w = e, not e / s
             "reversed_layers",    # layer K - 1 - k weighted by w_k
             "drop_by_source",     # the dropout mask keyed by the source row instead of the position in the call
             "no_scale",           # dx of a kept element not scaled by 65536 / (65536 - thr)
             "no_wn",              # gs = grad, without w_n
             "dead_rows",          # rows past frame_lens counted in d
             "infeasible_counted",  # an infeasible item's rows counted in d
             "W_transposed"]       # W [H, V] read as if it were stored [V, H]


def tile_rows(R_):
    return TILE_ROWS * -(-R_ // (TILE_ROWS * MAX_TILES))


def tiles(R_):
    return -(-R_ // tile_rows(R_))


def chain_depth(N, T_max, H, V):
    """The most roundings a term of d_k passes through on its way into the sum, from the order the header states."""
    rows = N * T_max
    hs = 256 if V <= 32 else 128
    rp = 2048 // hs
    per_thread = -(-tile_rows(rows) // rp) * -(-H // hs) * 8
    return per_thread + 6 + 3 + -(-tiles(rows) // 64) + 6


def softmax_ref(a, mutate=None):
    """a [K] -> (w float64 [K], its bound E_w [K])."""
    a = f64(a)
    K = len(a)
    dlt = a - a.max()
    e = np.exp(dlt)
    w = e.copy() if mutate == "unnormalised" else e / e.sum()
    wt = e / e.sum()
    r = C_EXP + U * np.abs(dlt)
    r_s = float((wt * r).sum()) + gam(max(K - 1, 0))
    return w, wt * (r + r_s + U) * (1.0 + SLACK) + DENORM


def gather_layers(layers, row_index=None, N=None):
    """layers [K, n_src, T, H] -> the call's x float64 [K, N, T, H]."""
    return np.stack([R.gather(l, row_index, N) for l in layers])


def forward(x, a, frame_lens, mutate=None):
    """x float64 [K, N, T, H] (gathered) -> dict(w, b_w, mixed [N, T, H], b_mixed, live); dead rows hold zeros."""
    x = f64(x)
    K, N, T, H = x.shape
    w, b_w = softmax_ref(a, mutate)
    xs = x[::-1] if mutate == "reversed_layers" else x
    live = R.live_rows(frame_lens, T)
    z = live[None, :, :, None]
    mixed = np.where(z[0], np.einsum("k,knth->nth", w, xs), 0.0)
    mag = np.einsum("k,knth->nth", np.abs(w), np.abs(xs))
    b = (gam(K) * mag + np.einsum("k,knth->nth", b_w, np.abs(xs))) * (1.0 + SLACK) + DENORM
    return dict(w=w, b_w=b_w, mixed=mixed, b_mixed=b, live=live)


def backward(x, a, grad, infeasible, label_lens, frame_lens, reduction, L_max, W, keep=None, scale=1.0, mutate=None):
    """x float64 [K, N, T, H] (gathered), grad [N, T, V] as tmi_ctc_posteriors wrote it (anything on dead rows and for
    infeasible items: not read), W [H, V], keep [N, T, H] by position or None -> dict(d, g_a, w, and the bounds b_d, b_g)."""
    x, grad, W = f64(x), f64(grad), f64(W)
    K, N, T, H = x.shape
    V = W.shape[1]
    bad = np.asarray(infeasible) != 0
    live = R.live_rows(frame_lens, T)
    wn = R.weights(bad, label_lens, N, L_max, reduction)
    if mutate == "no_wn":
        wn = np.where(bad, 0.0, 1.0)
    if mutate == "infeasible_counted":
        wn = R.weights(np.zeros(N), label_lens, N, L_max, reduction)
    if mutate == "dead_rows":
        live = np.ones_like(live)
    if mutate == "W_transposed":
        W = W.reshape(-1).reshape(V, H).T
    gs = np.where(live[:, :, None], grad * wn[:, None, None], 0.0)
    s = 1.0 if mutate == "no_scale" else scale
    dx = gs @ W.T
    dxm = np.abs(gs) @ np.abs(W).T
    if keep is not None:
        dx, dxm = np.where(keep, dx * s, 0.0), np.where(keep, dxm * s, 0.0)
    xs = x[::-1] if mutate == "reversed_layers" else x
    d = np.einsum("nth,knth->k", dx, xs)
    b_d = gam(V + 3 + chain_depth(N, T, H, V)) * np.einsum("nth,knth->k", dxm, np.abs(xs))
    w, b_w = softmax_ref(a)
    dot = float((w * d).sum())
    diff = d - (0.0 if mutate == "no_jacobian_mean" else dot)
    g_a = w * diff
    e_dot = float((b_w * np.abs(d) + w * b_d).sum()) + gam(K) * float(np.abs(w * d).sum())
    e_diff = b_d + e_dot + U * np.abs(diff)
    b_g = w * e_diff + b_w * np.abs(diff) + U * np.abs(g_a)
    k = 1.0 + SLACK
    return dict(d=d, g_a=g_a, w=w, dx=dx, b_d=b_d * k + DENORM, b_g=b_g * k + DENORM)


def step(x, a, W, b, frame_lens, labels, label_lens, reduction, L_max, keep=None, scale=1.0, blank=0):
    """The whole mixed head step in float64 -> (mix forward dict, head forward dict, (grad, nll, infeasible), head backward
    dict, mix backward dict)."""
    mf = forward(x, a, frame_lens)
    f = R.forward(mf["mixed"], W, b, frame_lens, keep, scale)
    grad, nll, bad, _ = R.posteriors(f["logp"], labels, label_lens, frame_lens, blank)
    g = R.backward(f["xd"], grad, nll, bad, label_lens, frame_lens, reduction, L_max)
    mb = backward(x, a, grad, bad, label_lens, frame_lens, reduction, L_max, W, keep, scale)
    return mf, f, (grad, nll, bad), g, mb


def loss_of(x, a, W, b, frame_lens, labels, label_lens, reduction, L_max, keep=None, scale=1.0, blank=0):
    return step(x, a, W, b, frame_lens, labels, label_lens, reduction, L_max, keep, scale, blank)[3]["loss"]


def forward_f32(x, a, frame_lens):
    """tmi_layer_mix_fwd's operations in numpy float32, one rounding per operation (no fused multiply-add) -> (w, mixed)."""
    f32 = np.float32
    x, a = np.asarray(x, dtype=f32), np.asarray(a, dtype=f32)
    e = np.exp(a - a.max()).astype(f32)
    s = e[0]
    for k in range(1, len(a)):
        s = f32(s + e[k])
    w = (e / s).astype(f32)
    acc = np.zeros(x.shape[1:], dtype=f32)
    for k in range(len(a)):
        acc = acc + w[k] * x[k]
    return w, np.where(R.live_rows(frame_lens, x.shape[2])[:, :, None], acc, f32(0))


def backward_f32(x, a, grad, infeasible, label_lens, frame_lens, reduction, L_max, W, keep=None, scale=1.0):
    """tmi_layer_mix_bwd's operations in numpy float32 (products and sums rounded separately; the rows one by one in
    ascending order, a row's columns pairwise: another order than the kernel's, with no fewer roundings per term than
    ``chain_depth`` allows for at the sizes used) -> (d, g_a)."""
    f32 = np.float32
    x, grad, W = np.asarray(x, dtype=f32), np.asarray(grad, dtype=f32), np.asarray(W, dtype=f32)
    K, N, T, H = x.shape
    bad = np.asarray(infeasible) != 0
    L = np.clip(np.asarray(label_lens, dtype=np.int64), 1, max(L_max, 1)).astype(f32)
    wn = np.ones(N, dtype=f32) if reduction == "sum" else (f32(1) / (L * f32(N))).astype(f32)
    live = R.live_rows(frame_lens, T)
    d = np.zeros(K, dtype=f32)
    w, _ = forward_f32(x[:, :1, :1], a, [1])
    for n in range(N):
        if bad[n]:
            continue
        for t in range(T):
            if not live[n, t]:
                continue
            gs = (grad[n, t] * wn[n]).astype(f32)
            dx = np.zeros(H, dtype=f32)
            for v in range(W.shape[1]):
                dx = dx + gs[v] * W[:, v]
            if keep is not None:
                dx = np.where(keep[n, t], dx * f32(scale), f32(0))
            d = d + (dx[None, :] * x[:, n, t]).sum(axis=1, dtype=f32)
    dot = f32(0)
    for j in range(K):
        dot = f32(dot + f32(w[j] * d[j]))
    return d, (w * (d - dot)).astype(f32)


# ============================================================================================== shape classes
# name: (K, N, T_max, H, V, dtype, p, reduction, x_pad (x_st = H + x_pad), gathered through a permuted row_index)
CASES = {
    "K3 tiny perm": (3, 2, 5, 8, 2, "fp32", 0.5, "mean", 8, True),
    "K13 H72 V31 bf16 perm": (13, 3, 37, 72, 31, "bf16", 0.1, "mean", 8, True),
    "K13 H72 V31 f32": (13, 3, 37, 72, 31, "fp32", 0.1, "sum", 3, False),
    "K25 H1024 V32 bf16": (25, 2, 20, 1024, 32, "bf16", 0.1, "mean", 0, False),
    "K64 V64 f32": (64, 1, 3, 8, 64, "fp32", 0.0, "sum", 0, False),
    "R350 K5 bf16 perm": (5, 5, 70, 264, 33, "bf16", 0.5, "mean", 1, True),
    "R16500 K2 f32": (2, 33, 500, 8, 2, "fp32", 0.1, "mean", 0, False),
    "R8192 K2 bf16": (2, 2, 4096, 8, 2, "bf16", 0.1, "sum", 0, False),       # the last size with tiles of 8 rows
    "R8193 K2 bf16": (2, 3, 2731, 8, 2, "bf16", 0.1, "sum", 0, False),       # the first with tiles of 16
    "R513 K2 f32": (2, 27, 19, 8, 3, "fp32", 0.0, "mean", 0, False),         # 65 tiles: a lane of the fold adds two
}
L_MAX = 6
N_SRC_EXTRA = 2
CASE_SEED = 2727
SPECIAL_A = {"K3 tiny perm": (80.0, -80.0, 0.0)}

_INPUTS, _REF = {}, {}


def case_inputs(name):
    """The seeded inputs of a case (computed once per process, nobody writes into them): layers [K, n_src, T, H] (fp32- or
    bf16-exact, as float32), the logits a, W, row_index (a permutation with one entry out of range; the tiny case: reversed)
    or None, ragged frame_lens with one item at 0 (N >= 3) and one beyond T_max, label_lens, random fp32 grad [N, T, V] as a
    posteriors call could have left it (nonzero past the clips and for the infeasible item), infeasible with one item set
    (N >= 3)."""
    if name in _INPUTS:
        return _INPUTS[name]
    K, N, T, H, V, dtype, p, reduction, x_pad, perm = CASES[name]
    g = np.random.default_rng(sum(map(ord, name)) * 37 + K)
    n_src = N + N_SRC_EXTRA
    layers = g.standard_normal((K, n_src, T, H)).astype(np.float32)
    if dtype == "bf16":
        layers = R.bf16_round(layers)
    a = np.asarray(SPECIAL_A.get(name, g.standard_normal(K) * 1.5), dtype=np.float32)
    W = (g.uniform(-1, 1, (H, V)) * math.sqrt(6.0 / (H + V)) * 2.0).astype(np.float32)
    row_index = None
    if perm:
        row_index = g.permutation(n_src)[:N].astype(np.int32)
        if N == 2:
            row_index = np.array([n_src + 1, 0], dtype=np.int32)   # reversed, one entry out of range
        else:
            row_index[N // 2] = n_src + 3
    frame_lens = g.integers(max(1, T // 2), T + 1, N).astype(np.int32)
    frame_lens[0] = T
    if N == 2:
        frame_lens[1] = min(2, T)
    if N >= 3:
        frame_lens[1], frame_lens[2] = T + 5, 0
    label_lens = g.integers(0, L_MAX + 1, N).astype(np.int32)
    grad = (g.standard_normal((N, T, V)) * 0.3).astype(np.float32)
    infeasible = np.zeros(N, dtype=np.int32)
    if N >= 4:
        infeasible[3] = 1
    _INPUTS[name] = dict(K=K, N=N, T=T, H=H, V=V, dtype=dtype, p=p, reduction=reduction, x_st=H + x_pad, n_src=n_src, layers=layers,
                         a=a, W=W, row_index=row_index, frame_lens=frame_lens, label_lens=label_lens, grad=grad,
                         infeasible=infeasible, seed=CASE_SEED)
    return _INPUTS[name]


def case_ref(name):
    """(inputs, x gathered, keep by position or None, keep by source row, scale, forward dict, backward dict), shared."""
    if name not in _REF:
        d = case_inputs(name)
        keep, keep_src, scale = R.keep_masks(d["seed"], d["n_src"], d["row_index"], d["N"], d["T"], d["H"], d["p"])
        if d["p"] == 0.0:
            keep = keep_src = None
        x = gather_layers(d["layers"], d["row_index"], d["N"])
        f = forward(x, d["a"], d["frame_lens"])
        b = backward(x, d["a"], d["grad"], d["infeasible"], d["label_lens"], d["frame_lens"], d["reduction"], L_MAX, d["W"], keep, scale)
        _REF[name] = (d, x, keep, keep_src, scale, f, b)
    return _REF[name]


def mutated(name, mutation):
    """What a wrong implementation would return on the case -> dict of the outputs the mutation changes."""
    d, x, keep, keep_src, scale, f, b = case_ref(name)
    out = {}
    if mutation in ("unnormalised", "reversed_layers"):
        m = forward(x, d["a"], d["frame_lens"], mutate=mutation)
        out.update(w=m["w"], mixed=m["mixed"])
    if mutation != "unnormalised":
        k = keep_src if mutation == "drop_by_source" else keep
        m = backward(x, d["a"], d["grad"], d["infeasible"], d["label_lens"], d["frame_lens"], d["reduction"], L_MAX, d["W"], k, scale,
                     mutate=mutation)
        out.update(d=m["d"], g_a=m["g_a"])
    return out


# the cases on which each mutation must exceed the bounds, and the outputs that must show it
MUTATION_CASES = {
    "no_jacobian_mean": (("K13 H72 V31 bf16 perm", "K13 H72 V31 f32", "K25 H1024 V32 bf16", "R350 K5 bf16 perm"), ("g_a",)),
    "unnormalised": (("K13 H72 V31 bf16 perm", "K25 H1024 V32 bf16", "K64 V64 f32", "R350 K5 bf16 perm"), ("w", "mixed")),
    "reversed_layers": (("K13 H72 V31 bf16 perm", "K13 H72 V31 f32", "K25 H1024 V32 bf16", "R350 K5 bf16 perm"), ("mixed", "d", "g_a")),
    "drop_by_source": (("K13 H72 V31 bf16 perm", "R350 K5 bf16 perm"), ("d", "g_a")),
    "no_scale": (("K13 H72 V31 bf16 perm", "K13 H72 V31 f32", "K25 H1024 V32 bf16", "R350 K5 bf16 perm"), ("d", "g_a")),
    "no_wn": (("K13 H72 V31 bf16 perm", "K25 H1024 V32 bf16", "R350 K5 bf16 perm"), ("d", "g_a")),
    "dead_rows": (("K13 H72 V31 bf16 perm", "K13 H72 V31 f32", "R350 K5 bf16 perm"), ("d", "g_a")),
    "infeasible_counted": (("R350 K5 bf16 perm", "R513 K2 f32"), ("d", "g_a")),
    "W_transposed": (("K13 H72 V31 bf16 perm", "K13 H72 V31 f32", "K25 H1024 V32 bf16", "R350 K5 bf16 perm"), ("d", "g_a")),
}


# ============================================================================================== the planted problem
# The planted problem of ``_ctc_head_ref`` (hidden[n, t] = E[path(n, t)] + 0.5 noise) sits in ONE middle layer k* of K = 5;
# the other four layers are noise independent of the labels, of the same scale (the planted layer's variance per element is
# 1 + 0.25).  From uniform weights the fit must bring the token error rate to exactly 0 and argmax(weights) to k*.
PLANTED = dict(R.PLANTED, K=5, k_star=2, mix_lr=5e-2, noise_seed=23)
PLANTED_STEPS = 120   # the budget: twice the reference's own last failing step (60), asserted in tests/test_layer_mix_cpu.py


def planted_problem():
    """-> dict(layers float32 [K, N, T, H], frame_lens, labels, label_lens, V, H, k_star): seeded."""
    c = PLANTED
    pr = R.planted_problem()
    g = np.random.default_rng(c["noise_seed"])
    layers = (g.standard_normal((c["K"],) + pr["hidden"].shape) * math.sqrt(1.0 + c["noise"] ** 2)).astype(np.float32)
    layers[c["k_star"]] = pr["hidden"]
    return dict(pr, layers=layers, k_star=c["k_star"])


def planted_run(steps, base_seed=0, problem=None):
    """The planted problem trained with the reference alone: float64 ``step`` under the project's dropout generator
    (SITE_CTC, (base_seed, step)) on the mixed features, "mean", float64 Keras Adam on the head (lr) and on the logits
    (mix_lr), from uniform weights.  -> per step (token errors, argmax of the weights) after the update."""
    c = PLANTED
    pr = problem or planted_problem()
    N, T, V, H, K = c["N"], c["T"], c["V"], c["H"], c["K"]
    W, b = (f64(t) for t in R.glorot(H, V, 5))
    x = f64(pr["layers"])
    a = np.zeros(K)
    par = [W, b, a]
    mom = [(np.zeros_like(q), np.zeros_like(q)) for q in par]
    out = []
    for t in range(steps):
        keep, _, scale = R.keep_masks(R.step_seed(base_seed, t), N, None, N, T, H, c["dropout"])
        _, _, _, g, mb = step(x, par[2], par[0], par[1], pr["frame_lens"], pr["labels"], pr["label_lens"], "mean", c["L_max"], keep, scale)
        corr = math.sqrt(1.0 - 0.999 ** (t + 1)) / (1.0 - 0.9 ** (t + 1))
        for i, (gr, lr) in enumerate(((g["gW"], c["lr"]), (g["gb"], c["lr"]), (mb["g_a"], c["mix_lr"]))):
            m_, v_ = mom[i]
            m_, v_ = 0.9 * m_ + 0.1 * gr, 0.999 * v_ + 0.001 * gr ** 2
            mom[i] = (m_, v_)
            par[i] = par[i] - lr * corr * m_ / (np.sqrt(v_) + 1e-7)
        mf = forward(x, par[2], pr["frame_lens"])
        f = R.forward(mf["mixed"], par[0], par[1], pr["frame_lens"])
        out.append((R.token_errors(f["logp"], pr["frame_lens"], pr["labels"], pr["label_lens"]), int(np.argmax(mf["w"]))))
    return out


def last_failing_step(run, k_star):
    """The 1-based number of the last step after which the token errors are not 0 or the largest weight is not k*'s."""
    bad = [t + 1 for t, (e, k) in enumerate(run) if e != 0 or k != k_star]
    return bad[-1] if bad else 0
