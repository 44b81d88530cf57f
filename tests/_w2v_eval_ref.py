"""Host restatement (float64) of Wav2Vec2 evaluation: the gathered contrastive loss of V:866-899 with the rule for padded
frames (a masked frame is not scored as a query and is dropped from every softmax as a negative), its argmax flag, the code
counts over the valid frames, the perplexity of V:653-660 as a function of counts, and the forward pass that feeds them
(tests/_w2v_infer_ref.py plus the oracle's quantiser and projection heads).  Test infrastructure only; the oracle itself is
untouched.  tests/test_w2v_eval_cpu.py checks this file against the oracle and against a naive per-row loop."""
import math

import numpy as np
import torch

import _w2v_infer_ref as R
from oracle import wav2vec2_oracle as V

U = 2.0 ** -24  # unit roundoff of fp32


def _neg3(neg, B, T, per_time):
    """[B, Nn] (one row per batch row, V:908-937) or [T, Nn] (one row per time step, whisper_single.py:789-839) -> [B, T, Nn]."""
    neg = np.asarray(neg, dtype=np.int64)
    if per_time:
        assert neg.shape[0] == T
        return np.broadcast_to(neg[None, :, :], (B, T, neg.shape[1]))
    assert neg.shape[0] == B
    return np.broadcast_to(neg[:, None, :], (B, T, neg.shape[1]))


def score(h, q, neg, temperature, mask=None, per_time=False):
    """h, q [B, T, pd], neg [B, Nn] / [T, Nn], mask [B, T] (valid iff > 0) or None -> dict of float64 / bool arrays:
    ``z`` [B, T, 1 + Nn] the logits (column 0 the positive), ``abs`` the matching sums of |h_k q_jk| / temperature (what a
    rounding bound of a logit is made of), ``keep`` which columns enter the softmax, ``valid`` [B, T], ``row_loss``,
    ``row_correct`` (int), ``gap`` = logit_0 - the largest kept negative logit (+inf where none is kept)."""
    h, q = np.asarray(h, dtype=np.float64), np.asarray(q, dtype=np.float64)
    B, T, _ = h.shape
    n3 = _neg3(neg, B, T, per_time)
    Nn = n3.shape[2]
    idx = np.concatenate([np.broadcast_to(np.arange(T)[None, :, None], (B, T, 1)), n3], axis=2)   # [B, T, 1 + Nn]
    qg = q[np.arange(B)[:, None, None], idx]                                                        # [B, T, 1 + Nn, pd]
    z = (h[:, :, None, :] * qg).sum(-1) / temperature
    ab = (np.abs(h[:, :, None, :]) * np.abs(qg)).sum(-1) / temperature
    valid = np.ones((B, T), dtype=bool) if mask is None else np.asarray(mask) > 0
    keep = valid[np.arange(B)[:, None, None], idx].copy()
    keep[:, :, 0] = True
    zk = np.where(keep, z, -np.inf)
    mx = zk.max(-1)
    lse = mx + np.log(np.exp(zk - mx[..., None]).sum(-1))
    row_loss = np.where(valid, lse - z[:, :, 0], 0.0)
    mneg = zk[:, :, 1:].max(-1) if Nn else np.full((B, T), -np.inf)
    gap = z[:, :, 0] - mneg
    row_correct = (valid & (gap >= 0)).astype(np.int64)
    return {"z": z, "abs": ab, "keep": keep, "valid": valid, "row_loss": row_loss, "row_correct": row_correct, "gap": gap}


def score_naive(h, q, neg, temperature, mask=None, per_time=False):
    """The same thing one row at a time, written without broadcasting -> (row_loss, row_correct)."""
    h, q = np.asarray(h, dtype=np.float64), np.asarray(q, dtype=np.float64)
    B, T, pd = h.shape
    loss, correct = np.zeros((B, T)), np.zeros((B, T), dtype=np.int64)
    for b in range(B):
        for t in range(T):
            if mask is not None and not mask[b][t] > 0:
                continue
            z0 = sum(float(h[b, t, k]) * float(q[b, t, k]) for k in range(pd)) / temperature
            zs = [z0]
            row = neg[t] if per_time else neg[b]
            for j in row:
                j = int(j)
                if mask is not None and not mask[b][j] > 0:
                    continue
                zs.append(sum(float(h[b, t, k]) * float(q[b, j, k]) for k in range(pd)) / temperature)
            m = max(zs)
            loss[b, t] = m + math.log(sum(math.exp(v - m) for v in zs)) - z0
            correct[b, t] = 1 if all(z0 >= v for v in zs[1:]) else 0
    return loss, correct


def bounds(ref, pd, Nn):
    """The derived fp32 bounds of tests/test_w2v_score_gpu.py from a ``score`` result: a logit's error e_j = (pd + 2) U
    sum_k |h_k q_jk| / temperature (pd roundings of the fma chain, the reciprocal of the temperature, the product with it);
    -> (row-loss bound e_0 + max kept e_n + (Nn + 8) U max(1, |loss|), flag band e_0 + max kept e_n), both [B, T]."""
    e = (pd + 2) * U * ref["abs"]
    en = np.where(ref["keep"][:, :, 1:], e[:, :, 1:], 0.0).max(-1) if Nn else np.zeros(e.shape[:2])
    band = e[:, :, 0] + en
    return band + (Nn + 8) * U * np.maximum(1.0, np.abs(ref["row_loss"])), band


def code_counts(idx, Nc, mask=None):
    """idx [rows, G] -> int64 [G, Nc]: the codes of the valid rows, indices clamped to [0, Nc) as tmi_vq_assign does."""
    idx = np.clip(np.asarray(idx, dtype=np.int64), 0, Nc - 1)
    rows, G = idx.shape
    live = np.ones(rows, dtype=bool) if mask is None else np.asarray(mask).reshape(rows) > 0
    return np.stack([np.bincount(idx[live, g], minlength=Nc) for g in range(G)]).astype(np.int64)


def perplexity_from_counts(counts):
    """V:653-660: mean_g exp(-sum_c p log(p + 1e-10)), p = clip(count / n, 1e-10, 1), written out bin by bin."""
    counts = np.asarray(counts, dtype=np.float64)
    total = 0.0
    for row in counts:
        n = float(row.sum())
        ent = 0.0
        for c in row:
            p = min(max(float(c) / n, 1e-10), 1.0)
            ent += p * math.log(p + 1e-10)
        total += math.exp(-ent)
    return total / counts.shape[0]


def forward(p, audio, cfg, mask=None, force_idx=None):
    """The evaluation forward pass in float64: tests/_w2v_infer_ref.forward (attention keys masked), the quantiser on the
    projected features (V:784) and both heads without dropout (V:550-561) -> projected_states, projected_quantized_features,
    code_indices [B, T, G]."""
    assert V.DROPOUT_PROVIDER is None
    out = R.forward(p, audio, cfg, mask)
    hproj = out["hidden_states"][0]  # the feature projection's LayerNorm output: the encoder's input
    quantized, idx, _, _ = V.quantizer(p, hproj, cfg, force_idx)
    return {"projected_states": V.projection_head(p, "project_hid", out["last_hidden_state"], cfg),
            "projected_quantized_features": V.projection_head(p, "project_q", quantized, cfg), "code_indices": idx}
