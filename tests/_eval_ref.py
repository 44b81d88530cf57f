"""tmi_logprob_fold and the evaluation sums (whisper.py evaluate / score) restated in numpy, fp64.

``fold``: per row of a logits matrix the log-sum-exp over the V real columns, the argmax (the largest logit, the smallest
column among equals, -0 == +0) and the target's log-probability (0 for target -1).  ``weighted``: the reference's masked
loss (W:596-600) and the token accuracy under the same weights.  ``score_sums``: ``score``'s per-sequence sums.
``chunked_fold`` walks the chunk schedule the way the kernel does (running max / sum, strictly-greater replacement of the
best) - in fp64 it must agree with ``fold``; that is the check that the chunking itself loses nothing.

The bound form for the kernel's fp32 arithmetic is tests/_sample_ref.py's: |x - x64| <= REL * (scale + |lse|), scale the
largest |logit| of the row."""
import numpy as np


def fold(z, V, targets, zt=None):
    """z [M, >= V] (only columns < V are read), targets [M] int (-1: not scored), zt [M] or None: the target logits
    where they do not come from ``z`` (the fp32 recomputation of the bf16 path) - the target's own term of the sum is
    then taken at zt too, tmi_linear_xent's rule: logprob = zt - log(sum_{n != target} exp(z_n) + exp(zt)).
    -> lse [M] (always of ``z`` as given), argmax [M], logprob [M]."""
    z = np.asarray(z, dtype=np.float64)[:, :V]
    targets = np.asarray(targets, dtype=np.int64)
    M = z.shape[0]
    mx = z.max(axis=1)
    lse = mx + np.log(np.exp(z - mx[:, None]).sum(axis=1))
    arg = np.argmax(z + 0.0, axis=1)  # (numpy: the first of equal maxima; -0.0 + 0.0 = +0.0)
    t = np.where(targets >= 0, targets, 0)
    if zt is None:
        logprob = np.where(targets >= 0, z[np.arange(M), t] - lse, 0.0)
    else:
        zt = np.asarray(zt, dtype=np.float64)
        others = z.copy()
        others[np.arange(M), t] = -np.inf
        om = others.max(axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            rest = np.where(np.isfinite(om), om + np.log(np.exp(others - np.where(np.isfinite(om), om, 0.0)[:, None]).sum(axis=1)), -np.inf)
        logprob = np.where(targets >= 0, zt - np.logaddexp(rest, zt), 0.0)
    return lse, arg.astype(np.int64), logprob


def chunk_schedule(V, ld, nc):
    """[(col0, ncols)]: ops.logprob_chunks restated."""
    return [(c0, min(nc, ld - c0)) for c0 in range(0, V, nc)]


def chunked_fold(z, V, ld, nc, targets):
    """``fold`` computed chunk by chunk with running state, as tmi_logprob_fold does (fp64, so order does not matter)."""
    z = np.asarray(z, dtype=np.float64)
    targets = np.asarray(targets, dtype=np.int64)
    M = z.shape[0]
    m, s = np.full(M, -np.inf), np.zeros(M)
    best_v, best_c, zt = np.full(M, -np.inf), np.full(M, -1, dtype=np.int64), np.zeros(M)
    for c0, n in chunk_schedule(V, ld, nc):
        real = min(n, V - c0)
        blk = z[:, c0:c0 + real]
        cm = blk.max(axis=1)
        cs = np.exp(blk - cm[:, None]).sum(axis=1)
        nm = np.maximum(m, cm)
        s = s * np.exp(m - nm) + cs * np.exp(cm - nm)
        m = nm
        ca = np.argmax(blk + 0.0, axis=1)
        cv = blk[np.arange(M), ca] + 0.0
        take = cv > best_v  # strictly greater: the earlier chunk wins a tie
        best_v, best_c = np.where(take, cv, best_v), np.where(take, c0 + ca, best_c)
        here = (targets >= c0) & (targets < c0 + real)
        zt = np.where(here, z[np.arange(M), np.where(here, targets, 0)], zt)
    lse = m + np.log(s)
    return lse, best_c, np.where(targets >= 0, zt - lse, 0.0)


def shift_targets(labels, mask=None):
    """evaluate's targets [B, S] and weights [B, S - 1]: row (b, t), t < S - 1, is scored against labels[b, t + 1]
    (W:585-586) with weight mask[b, t] (W:597; all ones without a mask); weight 0 and row S - 1: target -1."""
    labels = np.asarray(labels, dtype=np.int64)
    B, S = labels.shape
    w = np.ones((B, S - 1)) if mask is None else np.asarray(mask, dtype=np.float64)[:, :-1]
    t = np.full((B, S), -1, dtype=np.int64)
    t[:, :-1] = np.where(w > 0, labels[:, 1:], -1)
    return t, w


def weighted(logprob, argmax, targets, w):
    """logprob / argmax / targets [B, S] (row S - 1 unused), w [B, S - 1] -> (loss, accuracy, loss_sum, n_correct,
    n_tokens): loss = sum(w * nll) / sum(w) (W:596-600), accuracy = sum(w * (argmax == target)) / sum(w)."""
    lp = np.asarray(logprob, dtype=np.float64)[:, :-1]
    hit = (np.asarray(argmax)[:, :-1] == np.asarray(targets)[:, :-1]).astype(np.float64)
    w = np.asarray(w, dtype=np.float64)
    loss_sum, n_correct, n_tokens = float(-(w * lp).sum()), float((w * hit).sum()), float(w.sum())
    return loss_sum / n_tokens, n_correct / n_tokens, loss_sum, n_correct, n_tokens


def score_sums(token_logprobs, lengths):
    """token_logprobs [N, n], lengths [N] -> the sum over each row's first lengths[i] entries."""
    lp = np.asarray(token_logprobs, dtype=np.float64)
    keep = np.arange(lp.shape[1])[None, :] < np.asarray(lengths)[:, None]
    return (lp * keep).sum(axis=1)


def top2_gap(z, V):
    """Per row: the gap between the two largest logits over the V real columns (0 for V = 1 is never needed here)."""
    z = np.asarray(z, dtype=np.float64)[:, :V]
    part = np.partition(z, V - 2, axis=1)
    return part[:, V - 1] - part[:, V - 2]
