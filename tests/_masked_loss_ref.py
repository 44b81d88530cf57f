"""The reference's weighted loss (speech_jobs/whisper_dist.py W:596-598: ``sum(nll * mask[:, :-1]) / sum(mask[:, :-1])``,
used when ``call`` is given a decoder_attention_mask) restated in fp64 on top of the oracle.

``weighted_xent``: loss and dlogits in closed form.  ``loss_and_grads``: the oracle's own forward (``O.forward_loss`` - the
mask weights the loss only, the decoder keeps its triangular mask, as the project's ``evaluate`` reads W:509) with the
weighted loss on its logits, differentiated by autograd.  ``train_steps``: ``O.train_steps`` with a mask per sample - every
replica normalises by the sum of its own weights, gradients and printed losses are summed over replicas (W:829-836).

Convention where the reference divides 0 by 0 (every weight 0): loss 0 and zero gradients."""
import numpy as np
import torch

from oracle import whisper_oracle as O


def weights_of(mask):
    """mask [B, S] -> w [B, S] fp64 with column S - 1 zeroed (W:597 slices it off)."""
    w = torch.as_tensor(np.asarray(mask, dtype=np.float64)).clone()
    w[:, -1] = 0.0
    return w


def weighted_xent(logits, labels, mask, loss_scale=1.0):
    """logits [B, S, V], labels [B, S] int, mask [B, S] -> (loss, dlogits [B, S, V]) in fp64:
    dlogits[b, t] = loss_scale * w[b, t] / wsum * (softmax(logits[b, t]) - onehot(labels[b, t + 1])), row S - 1 zero.
    Rows of weight 0 contribute nothing whatever they hold (non-finite values included)."""
    z = torch.as_tensor(logits).double()
    B, S, V = z.shape
    lab = torch.as_tensor(np.asarray(labels)).long()
    w = weights_of(mask)
    wsum = float(w.sum())
    d = torch.zeros_like(z)
    if not wsum > 0.0:
        return 0.0, d
    tgt = torch.cat([lab[:, 1:], torch.zeros(B, 1, dtype=torch.long)], dim=1)
    scored = w > 0
    zs = torch.where(scored.unsqueeze(-1), z, torch.zeros_like(z))  # (an unscored row is never looked at)
    logp = torch.log_softmax(zs, dim=-1)
    nll = -logp.gather(-1, tgt.unsqueeze(-1)).squeeze(-1)
    loss = float((torch.where(scored, w * nll, torch.zeros_like(nll))).sum() / wsum)
    g = logp.exp()
    g.scatter_add_(-1, tgt.unsqueeze(-1), -torch.ones(B, S, 1, dtype=torch.float64))
    d = torch.where(scored.unsqueeze(-1), g * (loss_scale * w / wsum).unsqueeze(-1), d)
    return loss, d


def forward_loss(p, feats, labels, mask, cfg, training=True):
    """W:585-598 on the oracle's logits -> (loss tensor, logits)."""
    _, logits = O.forward_loss(p, feats, labels, cfg, training)
    w = weights_of(mask)[:, :-1].to(logits.dtype)
    V = logits.shape[-1]
    nll = torch.nn.functional.cross_entropy(logits[:, :-1].reshape(-1, V), labels[:, 1:].long().reshape(-1),
                                            reduction="none").reshape(w.shape)
    wsum = w.sum()
    if not float(wsum) > 0.0:
        return (logits * 0.0).sum(), logits
    return (nll * w).sum() / wsum, logits


def loss_and_grads(p, feats, labels, mask, cfg, training=True):
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
    loss, _ = forward_loss(leaves, feats, labels, mask, cfg, training)
    loss.backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()}
    return loss.detach(), grads


def train_steps(cfg, params, pool_feats, pool_labels, pool_mask, batch_size, num_steps, lr=1e-4, n_replicas=1):
    """``O.train_steps`` (dropout off) with ``pool_mask`` [N, S] batched alongside the pool."""
    cfg = O.make_config_like(cfg, dropout=0.0, attention_dropout=0.0, activation_dropout=0.0)
    state = O.AdamState()
    n, gb = pool_feats.shape[0], batch_size * n_replicas
    starts = list(range(0, n, gb))
    losses = []
    for i in range(num_steps):
        s = starts[i % len(starts)]
        f, l, m = pool_feats[s:s + gb], pool_labels[s:s + gb], pool_mask[s:s + gb]
        tot_loss, tot = 0.0, None
        for r in range(n_replicas):
            sl = slice(r * batch_size, (r + 1) * batch_size)
            if f[sl].shape[0] == 0:
                continue
            loss, g = loss_and_grads(params, torch.from_numpy(np.ascontiguousarray(f[sl])),
                                     torch.from_numpy(np.ascontiguousarray(l[sl])), m[sl], cfg)
            tot_loss += float(loss)
            tot = g if tot is None else {k: tot[k] + g[k] for k in g}
        O.adam_step(params, tot, state, lr=lr)
        losses.append(tot_loss)
    return losses, state
