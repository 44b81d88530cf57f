"""Float64 reference, seeded cases, bounds and mutations for the CTC-head kernels (csrc/ctc_head.hip: tmi_ctc_head_fwd,
tmi_ctc_head_bwd) and for the whole head step (forward, tmi_ctc_posteriors, backward), written literally from the
definitions in include/tethys_mi.h.  CPU only: nothing here imports the GPU package, so tests/test_ctc_head_cpu.py checks
the reference (torch's float64 autograd through ctc_loss, central finite differences) and the bounds (reachable by an honest
fp32 transcription, exceeded by every listed mutation) before tests/test_ctc_head_kernels_gpu.py and
tests/test_ctc_head_gpu.py compare a kernel with it.  The log-softmax and its bound are ``_ctc_ref.logsoftmax_ref``, the
posteriors and their bounds ``_ctc_post_ref.post_ref``, the dropout mask ``oracle.dropout.keep_flat`` under
``site_seed(base, step, SITE_CTC)``, keyed by the position n * T_max + t in the call.

The bounds are derived, not fitted, from the constants of ``_ctc_ref`` (U = 2^-24, gam(n) = n U / (1 - n U), SLACK; its
docstring states the assumption on the device's expf / logf).  Inputs are the same fp32 or bf16 numbers on both sides.
  xd        x * scale rounds once (p = 0: no rounding; a dropped element is an exact 0); the scale itself is the same fp32
            number on both sides.
  logits    H fused multiply-adds from 0, then + b: with the rounding of xd, gam(H + 2) (sum_h |xd_h W_hv| + |b_v|); the
            rounding of the scale product is charged once more on its own, U sum_h |xd_h W_hv|, so that the bound does not
            lean on how gam counts.
  logp      log-sum-exp is non-expansive in the sup norm, so the row's largest logit bound carries over to lse; the
            log-softmax's own roundings are ``logsoftmax_ref``'s bound;  E_lp = E_l[v] + max_v E_l + that.
  argmax    an integer: compared where the float64 top-two gap exceeds twice the row's largest logit bound (``decided``).
  gs        grad * w_n: w_n = 1 exactly ("sum"), or one division by an exact product ("mean"; max(L, 1) * N < 2^24 in every
            case here), then the product with grad: 2 roundings.
  gW, gb    a term passes through at most (live rows - 1) additions - a row that is not live adds an exact zero, and so does
            an empty chunk - after the roundings of xd and gs:  gam(rows + 3) sum_r |xd| |gs|  resp.  gam(rows + 3) sum_r |gs|,
            rows = the live rows of the call.
  loss      w_n * nll rounds as gs does (2 roundings), and of the additions of the running sums, the butterfly and the wave
            sums only those of two nonzero operands round - at most N - 1 on the way of any term:  gam(N + 1) sum |w nll|.
Every bound gets the factor (1 + SLACK) and the absolute floor DENORM = 2^-126.
"""
import math

import numpy as np

import _ctc_post_ref as P
import _ctc_ref as C
from oracle import dropout as D

U, SLACK, gam = C.U, C.SLACK, C.gam
DENORM = 2.0 ** -126
SITE_CTC = 6
ROW_CHUNK = 256      # include/tethys_mi.h: the row chunk up to N * T_max = 16384
MAX_CHUNKS = 64

MUTATIONS = ["drop_by_source",     # the dropout mask keyed by the source row instead of the position in the call
             "no_scale",           # kept elements not scaled by 65536 / (65536 - thr)
             "frames_past",        # frames past frame_lens included in gW / gb
             "mean_by_n",          # "mean" dividing by N only
             "gb_unweighted",      # gb summed without w_n
             "infeasible_loss",    # an infeasible item's nll in the loss
             "last_chunk"]         # the last row chunk dropped from gW / gb


def f64(a):
    return np.asarray(a, dtype=np.float64)


def chunk_rows(R):
    return ROW_CHUNK * -(-R // (ROW_CHUNK * MAX_CHUNKS))


def bf16_round(a):
    """float32 values rounded to the nearest bf16 (ties to even), as float32."""
    u = np.asarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def keep_masks(seed, n_src, row_index, N, T_max, H, p):
    """-> (keep by position [N, T_max, H], keep by SOURCE row [N, T_max, H] (the mutation), scale); p = 0: all kept, 1."""
    if p == 0.0:
        one = np.ones((N, T_max, H), dtype=bool)
        return one, one, 1.0
    idx = np.arange(N) if row_index is None else np.asarray(row_index, dtype=np.int64)
    rows = max(N, n_src, int(idx.max()) + 1 if len(idx) else 0) * T_max
    full = D.keep_flat(seed, rows, H, p).reshape(-1, T_max, H)
    return full[:N], full[np.clip(idx, 0, full.shape[0] - 1)], D.keep_scale(p)


def step_seed(base_seed, step):
    return D.site_seed(base_seed, step, SITE_CTC)


def gather(hidden, row_index=None, N=None):
    """hidden [n_src, >= T, H] -> the call's x float64 [N, T, H]; an index outside [0, n_src) reads as zeros."""
    hidden = f64(hidden)
    if row_index is None:
        return hidden[:N] if N is not None else hidden
    idx = np.asarray(row_index, dtype=np.int64)
    ok = (idx >= 0) & (idx < hidden.shape[0])
    return np.where(ok[:, None, None], hidden[np.where(ok, idx, 0)], 0.0)


def live_rows(frame_lens, T_max):
    """bool [N, T_max]: t < min(max(frame_lens[n], 0), T_max)."""
    T = np.clip(np.asarray(frame_lens, dtype=np.int64), 0, T_max)
    return np.arange(T_max)[None, :] < T[:, None]


def forward(x, W, b, frame_lens, keep=None, scale=1.0, mutate=None):
    """x float64 [N, T, H] (gathered), W [H, V], b [V] -> dict(xd, logits, logp, argmax, live, and the bounds b_logits,
    b_logp [N, T, V]); rows that are not live hold zeros everywhere (they are not compared)."""
    x, W, b = f64(x), f64(W), f64(b)
    N, T, H = x.shape
    live = live_rows(frame_lens, T)
    s = 1.0 if mutate == "no_scale" else scale
    xd = x.copy() if keep is None else np.where(keep, x * s, 0.0)
    xd = np.where(live[:, :, None], xd, 0.0)
    logits = xd @ W + b
    flat = logits.reshape(N * T, -1)
    logp, amax, b_ls = C.logsoftmax_ref(flat)
    mag = np.abs(xd) @ np.abs(W)
    E_l = gam(H + 2) * (mag + np.abs(b)) + (0.0 if keep is None or scale == 1.0 else U * mag)
    E_lp = E_l + E_l.max(axis=2, keepdims=True) + b_ls.reshape(logits.shape)
    k = 1.0 + SLACK
    z = live[:, :, None]
    return dict(xd=xd, logits=np.where(z, logits, 0.0), logp=np.where(z, logp.reshape(logits.shape), 0.0),
                argmax=np.where(live, amax.reshape(N, T), 0), live=live, b_logits=E_l * k + DENORM, b_logp=E_lp * k + DENORM)


def decided(f):
    """bool [N, T]: live rows whose argmax the float64 logits decide beyond the device's error."""
    top = np.sort(f["logits"], axis=2)
    return f["live"] & ((top[:, :, -1] - top[:, :, -2]) > 2.0 * f["b_logits"].max(axis=2))


def weights(infeasible, label_lens, N, L_max, reduction, mutate=None):
    L = np.clip(np.asarray(label_lens, dtype=np.int64), 1, max(L_max, 1))
    w = np.ones(N) if reduction == "sum" else (1.0 / N if mutate == "mean_by_n" else 1.0 / (L * N)) * np.ones(N)
    return np.where(np.asarray(infeasible) != 0, 0.0, w)


def backward(xd, grad, nll, infeasible, label_lens, frame_lens, reduction, L_max, mutate=None):
    """xd [N, T, H] (``forward``'s, zeros on rows that are not live), grad float64 [N, T, V] and nll [N] as
    tmi_ctc_posteriors wrote them (any values on rows that are not live and for infeasible items: they are not read) ->
    dict(gW, gb, loss, n_infeasible, and the bounds b_gW, b_gb, b_loss)."""
    xd, grad, nll = f64(xd), f64(grad), f64(nll)
    N, T, H = xd.shape
    bad = np.asarray(infeasible) != 0
    live = live_rows(frame_lens, T)
    w = weights(bad, label_lens, N, L_max, reduction, mutate)
    if mutate == "frames_past":
        live = np.ones_like(live)
    if mutate == "last_chunk":
        rc = chunk_rows(N * T)
        flat = live.reshape(-1).copy()
        flat[(N * T - 1) // rc * rc:] = False
        live = flat.reshape(N, T)
    gs = np.where(live[:, :, None], np.where(bad[:, None, None], 0.0, grad * w[:, None, None]), 0.0)
    gW = np.einsum("nth,ntv->hv", xd, gs)
    gb = gs.sum(axis=(0, 1))
    if mutate == "gb_unweighted":
        gb = np.where(live[:, :, None] & ~bad[:, None, None], grad, 0.0).sum(axis=(0, 1))
    terms = np.where(bad, 0.0, w * np.where(bad, 0.0, nll))
    if mutate == "infeasible_loss":
        terms = weights(np.zeros(N), label_lens, N, L_max, reduction) * nll
    rows = int(live.sum())
    k = 1.0 + SLACK
    b_gW = gam(rows + 3) * np.einsum("nth,ntv->hv", np.abs(xd), np.abs(gs)) * k + DENORM
    b_gb = gam(rows + 3) * np.abs(gs).sum(axis=(0, 1)) * k + DENORM
    b_loss = gam(N + 1) * np.abs(terms).sum() * k + DENORM
    return dict(gW=gW, gb=gb, loss=float(terms.sum()), n_infeasible=int(bad.sum()), w=w, gs=gs, b_gW=b_gW, b_gb=b_gb,
                b_loss=b_loss)


def posteriors(logp, labels, label_lens, frame_lens, blank=0):
    """``_ctc_post_ref.post_ref`` per item on float64 log-probs [N, T, V] -> (grad [N, T, V] (zeros where nothing is written),
    nll [N] with zero_infinity on, infeasible [N], the per-item reference dicts)."""
    logp = f64(logp)
    N, T, V = logp.shape
    grad, nll, bad, refs = np.zeros((N, T, V)), np.zeros(N), np.zeros(N, dtype=np.int64), []
    for n in range(N):
        Tn = int(np.clip(frame_lens[n], 0, T))
        r = P.post_ref(logp[n], np.asarray(labels[n])[:int(label_lens[n])], Tn, blank)
        refs.append(r)
        bad[n] = r["infeasible"]
        if not r["infeasible"]:
            nll[n] = r["nll"]
            grad[n, :Tn] = r["grad"]
    return grad, nll, bad, refs


def step(x, W, b, frame_lens, labels, label_lens, reduction, L_max, keep=None, scale=1.0, blank=0):
    """The whole head step in float64: forward, posteriors, backward -> (forward dict, (grad, nll, infeasible), backward dict)."""
    f = forward(x, W, b, frame_lens, keep, scale)
    grad, nll, bad, _ = posteriors(f["logp"], labels, label_lens, frame_lens, blank)
    return f, (grad, nll, bad), backward(f["xd"], grad, nll, bad, label_lens, frame_lens, reduction, L_max)


def loss_of(x, W, b, frame_lens, labels, label_lens, reduction, L_max, keep=None, scale=1.0, blank=0):
    return step(x, W, b, frame_lens, labels, label_lens, reduction, L_max, keep, scale, blank)[2]["loss"]


def forward_f32(x, W, b, frame_lens, keep=None, scale=1.0):
    """The kernel's operations in numpy float32, one rounding per operation (no fused multiply-add: more roundings than the
    kernel makes) -> (logits, logp) float32 [N, T, V]."""
    f32 = np.float32
    x, W, b = np.asarray(x, dtype=f32), np.asarray(W, dtype=f32), np.asarray(b, dtype=f32)
    N, T, H = x.shape
    xd = x if keep is None else np.where(keep, x * f32(scale), f32(0))
    lg = np.zeros((N, T, W.shape[1]), dtype=f32)
    for h in range(H):
        lg = lg + xd[:, :, h:h + 1] * W[h][None, None, :]
    lg = lg + b
    m = lg.max(axis=2, keepdims=True)
    s = np.zeros_like(m)
    for v in range(W.shape[1]):
        s = s + np.exp(lg[:, :, v:v + 1] - m).astype(f32)
    lse = m + np.log(s).astype(f32)
    return lg, lg - lse


def backward_f32(xd, grad, nll, infeasible, label_lens, frame_lens, reduction, L_max):
    """tmi_ctc_head_bwd's order in numpy float32 (products and sums rounded separately): chunks of ``chunk_rows`` rows, each
    a chain over its rows, then the chunks in ascending order -> (gW, gb, loss)."""
    f32 = np.float32
    xd, grad = np.asarray(xd, dtype=f32), np.asarray(grad, dtype=f32)
    N, T, H = xd.shape
    V = grad.shape[2]
    bad = np.asarray(infeasible) != 0
    L = np.clip(np.asarray(label_lens, dtype=np.int64), 1, max(L_max, 1)).astype(f32)
    w = np.ones(N, dtype=f32) if reduction == "sum" else (f32(1) / (L * f32(N))).astype(f32)
    w = np.where(bad, f32(0), w)
    live = live_rows(frame_lens, T).reshape(-1)
    X = np.where(live[:, None], xd.reshape(N * T, H), f32(0))
    G = np.where(live[:, None], (grad * w[:, None, None]).astype(f32).reshape(N * T, V), f32(0))
    rc = chunk_rows(N * T)
    gW = gb = None
    for c0 in range(0, N * T, rc):
        pw, pb = np.zeros((H, V), dtype=f32), np.zeros(V, dtype=f32)
        for r in range(c0, min(c0 + rc, N * T)):
            if live[r]:
                pw = pw + X[r][:, None] * G[r][None, :]
                pb = pb + G[r]
        gW, gb = (pw, pb) if gW is None else (gW + pw, gb + pb)
    loss = f32(0)
    for n in range(N):
        if not bad[n]:
            loss = loss + w[n] * f32(nll[n])
    return gW, gb, float(loss)


# ============================================================================================== shape classes
# name: (N, T_max, H, V, dtype, p, reduction, x_pad (x_st = H + x_pad), gathered through a permuted row_index).  N * T_max
# sits one below, at and one above the row chunk (255, 256, 257 = 257 x 1: 257 is prime); H 8 / 64 / 768; V 2 / 31 / 32 /
# 33 / 64; x_pad 0, a multiple of 8 (16-byte loads), and 1 / 3 (the element-wise loads); the last one is the largest case.
CASES = {
    "R255 H8 V2 f32": (5, 51, 8, 2, "fp32", 0.0, "sum", 0, False),
    "R256 H64 V31 bf16 perm": (4, 64, 64, 31, "bf16", 0.1, "mean", 8, True),
    "R257 H64 V33 f32": (257, 1, 64, 33, "fp32", 0.9, "mean", 3, False),
    "H768 V64 bf16 perm": (3, 40, 768, 64, "bf16", 0.1, "sum", 1, True),
    "H8 V32 bf16": (3, 20, 8, 32, "bf16", 0.9, "mean", 0, False),
    "R2400 H768 V32 bf16 perm": (8, 300, 768, 32, "bf16", 0.1, "mean", 8, True),
}
L_MAX = 6
N_SRC_EXTRA = 2   # source items beyond N: a permuted row_index reaches them
CASE_SEED = 4242


def case_inputs(name):
    """The seeded inputs of a case (computed once per process, nobody writes into them): hidden [n_src, T, H] (fp32- or
    bf16-exact, as float32), W, b, row_index (one entry out of range) or None, ragged frame_lens with one item at 0 and one at
    T_max, labels / label_lens with an L = 0 item, random fp32 grad [N, T, V] / nll [N] as a posteriors call could have left
    them (nonzero past the clips and for the infeasible item: the backward must not read those), infeasible with one item set."""
    if name in _INPUTS:
        return _INPUTS[name]
    N, T, H, V, dtype, p, reduction, x_pad, perm = CASES[name]
    g = np.random.default_rng(sum(map(ord, name)) * 31 + N)
    n_src = N + N_SRC_EXTRA
    hidden = g.standard_normal((n_src, T, H)).astype(np.float32)
    if dtype == "bf16":
        hidden = bf16_round(hidden)
    W = (g.uniform(-1, 1, (H, V)) * math.sqrt(6.0 / (H + V)) * 2.0).astype(np.float32)
    b = (g.standard_normal(V) * 0.5).astype(np.float32)
    row_index = None
    if perm:
        row_index = g.permutation(n_src)[:N].astype(np.int32)
        row_index[N // 2] = n_src + 3        # out of range: reads as zeros
    frame_lens = g.integers(max(1, T // 2), T + 1, N).astype(np.int32)
    frame_lens[0], frame_lens[min(3, N - 1)] = T, 0   # (not the last item where N allows: the last row chunk stays live)
    if N >= 4:
        frame_lens[1] = T + 5                # beyond T_max: clamped
    label_lens = g.integers(0, L_MAX + 1, N).astype(np.int32)
    label_lens[min(2, N - 1)] = 0
    labels = g.integers(1, V, (N, L_MAX)).astype(np.int32)
    grad = (g.standard_normal((N, T, V)) * 0.3).astype(np.float32)
    nll = (g.uniform(1.0, 30.0, N)).astype(np.float32)
    infeasible = np.zeros(N, dtype=np.int32)
    infeasible[1 if N > 1 else 0] = 1
    _INPUTS[name] = dict(N=N, T=T, H=H, V=V, dtype=dtype, p=p, reduction=reduction, x_st=H + x_pad, n_src=n_src, hidden=hidden,
                         W=W, b=b, row_index=row_index, frame_lens=frame_lens, label_lens=label_lens, labels=labels, grad=grad,
                         nll=nll, infeasible=infeasible, seed=CASE_SEED)
    return _INPUTS[name]


_INPUTS, _REF = {}, {}


def case_ref(name):
    """(inputs, keep by position, keep by source row, scale, float64 forward, float64 backward), computed once and shared."""
    if name not in _REF:
        d = case_inputs(name)
        keep, keep_src, scale = keep_masks(d["seed"], d["n_src"], d["row_index"], d["N"], d["T"], d["H"], d["p"])
        x = gather(d["hidden"], d["row_index"], d["N"])
        k = None if d["p"] == 0.0 else keep
        f = forward(x, d["W"], d["b"], d["frame_lens"], k, scale)
        g = backward(f["xd"], d["grad"], d["nll"], d["infeasible"], d["label_lens"], d["frame_lens"], d["reduction"], L_MAX)
        _REF[name] = (d, x, keep, keep_src, scale, f, g)
    return _REF[name]


def mutated(name, mutation):
    """What a wrong implementation would return on the case -> dict of the outputs the mutation changes."""
    d, x, keep, keep_src, scale, f, g = case_ref(name)
    k = None if d["p"] == 0.0 else keep
    if mutation == "drop_by_source":
        m = forward(x, d["W"], d["b"], d["frame_lens"], None if d["p"] == 0.0 else keep_src, scale)
        return dict(logits=m["logits"], logp=m["logp"])
    if mutation == "no_scale":
        m = forward(x, d["W"], d["b"], d["frame_lens"], k, scale, mutate="no_scale")
        return dict(logits=m["logits"], logp=m["logp"])
    xd = f["xd"]
    if mutation == "frames_past":   # the rows past the clips as a kernel that ignores frame_lens would form them
        xd = x.copy() if k is None else np.where(k, x * scale, 0.0)
    m = backward(xd, d["grad"], d["nll"], d["infeasible"], d["label_lens"], d["frame_lens"], d["reduction"], L_MAX, mutate=mutation)
    return dict(gW=m["gW"], gb=m["gb"], loss=m["loss"])


# the cases on which each mutation must exceed the bounds, and the outputs that must show it
MUTATION_CASES = {
    "drop_by_source": (("R256 H64 V31 bf16 perm", "H768 V64 bf16 perm", "R2400 H768 V32 bf16 perm"), ("logits", "logp")),
    "no_scale": (("R256 H64 V31 bf16 perm", "R257 H64 V33 f32", "H768 V64 bf16 perm", "H8 V32 bf16", "R2400 H768 V32 bf16 perm"),
                 ("logits", "logp")),
    "frames_past": (tuple(CASES), ("gW", "gb")),
    "mean_by_n": (("R256 H64 V31 bf16 perm", "R257 H64 V33 f32", "H8 V32 bf16", "R2400 H768 V32 bf16 perm"), ("gW", "gb", "loss")),
    "gb_unweighted": (("R256 H64 V31 bf16 perm", "R257 H64 V33 f32", "H8 V32 bf16", "R2400 H768 V32 bf16 perm"), ("gb",)),
    "infeasible_loss": (tuple(CASES), ("loss",)),
    "last_chunk": (("R257 H64 V33 f32", "R2400 H768 V32 bf16 perm"), ("gW", "gb")),
}


# ============================================================================================== the planted problem
# hidden[n, t] = E[path(n, t)] + 0.5 noise: every frame carries the embedding of the symbol a valid CTC path of the item's
# labels emits there, so a linear head can learn the transcript exactly.
PLANTED = dict(N=8, T=24, T_min=14, L_min=2, L_max=5, V=8, H=32, lr=1e-2, dropout=0.1, noise=0.5, seed=11)
PLANTED_STEPS = 240   # the budget: tests/test_ctc_head_cpu.py asserts it is at least twice the reference's last failing step


def planted_problem(seed=None):
    """-> dict(hidden float32 [N, T, H], frame_lens, labels [N, L_max], label_lens, V, H): seeded."""
    c = PLANTED
    g = np.random.default_rng(c["seed"] if seed is None else seed)
    N, T, V, H = c["N"], c["T"], c["V"], c["H"]
    E = g.standard_normal((V, H))
    frame_lens = g.integers(c["T_min"], T + 1, N).astype(np.int32)
    frame_lens[0] = T
    label_lens = g.integers(c["L_min"], c["L_max"] + 1, N).astype(np.int32)
    labels = np.zeros((N, c["L_max"]), dtype=np.int32)
    hidden = np.zeros((N, T, H))
    for n in range(N):
        L, Tn = int(label_lens[n]), int(frame_lens[n])
        lab = g.integers(1, V, L)
        labels[n, :L] = lab
        # a valid path: every label holds a run of frames, a blank run separates neighbours (required between equal ones)
        ext = [0]
        for s in lab:
            ext += [int(s), 0]
        cuts = np.sort(g.choice(np.arange(1, Tn), size=len(ext) - 1, replace=False))
        bounds = np.concatenate([[0], cuts, [Tn]])
        path = np.zeros(T, dtype=np.int64)
        for i, s in enumerate(ext):
            path[bounds[i]:bounds[i + 1]] = s
        hidden[n] = E[path] + c["noise"] * g.standard_normal((T, H))
    return dict(hidden=hidden.astype(np.float32), frame_lens=frame_lens, labels=labels, label_lens=label_lens, V=V, H=H)


def greedy_transcripts(logp, frame_lens, blank=0):
    out = []
    for n in range(logp.shape[0]):
        a = np.argmax(logp[n, :int(frame_lens[n])], axis=1)
        out.append([int(s) for t, s in enumerate(a) if s != blank and (t == 0 or s != a[t - 1])])
    return out


def token_errors(logp, frame_lens, labels, label_lens, blank=0):
    hyp = greedy_transcripts(logp, frame_lens, blank)
    return sum(C.levenshtein(h, list(labels[n, :int(label_lens[n])])) for n, h in enumerate(hyp))


def glorot(H, V, seed):
    g = np.random.default_rng(seed)
    return (g.uniform(-1, 1, (H, V)) * math.sqrt(6.0 / (H + V))).astype(np.float32), np.zeros(V, dtype=np.float32)


def planted_run(steps, base_seed=0, problem=None):
    """The planted problem trained with the reference alone: float64 ``step`` under the project's dropout generator
    (SITE_CTC, (base_seed, step)), "mean", float64 Keras Adam.  -> the token errors after every step (a list)."""
    c = PLANTED
    pr = problem or planted_problem()
    N, T, V, H = c["N"], c["T"], c["V"], c["H"]
    W, b = (f64(a) for a in glorot(H, V, 5))
    x = f64(pr["hidden"])
    mW, vW, mb, vb = np.zeros_like(W), np.zeros_like(W), np.zeros_like(b), np.zeros_like(b)
    errs = []
    for t in range(steps):
        keep, _, scale = keep_masks(step_seed(base_seed, t), N, None, N, T, H, c["dropout"])
        _, _, g = step(x, W, b, pr["frame_lens"], pr["labels"], pr["label_lens"], "mean", c["L_max"], keep, scale)
        lr_t = c["lr"] * math.sqrt(1.0 - 0.999 ** (t + 1)) / (1.0 - 0.9 ** (t + 1))
        mW, vW = 0.9 * mW + 0.1 * g["gW"], 0.999 * vW + 0.001 * g["gW"] ** 2
        mb, vb = 0.9 * mb + 0.1 * g["gb"], 0.999 * vb + 0.001 * g["gb"] ** 2
        W = W - lr_t * mW / (np.sqrt(vW) + 1e-7)
        b = b - lr_t * mb / (np.sqrt(vb) + 1e-7)
        f = forward(x, W, b, pr["frame_lens"])
        errs.append(token_errors(f["logp"], pr["frame_lens"], pr["labels"], pr["label_lens"]))
    return errs
