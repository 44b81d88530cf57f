"""Host restatement (float64) of the reference's ``Wav2Vec2Model.call(..., training=False)`` (V:768-825) with an
``attention_mask``: the oracle's ``feature_extractor``, ``dense``, ``layer_norm`` and ``gelu_erf`` with an attention of its
own that adds (1 - mask) * -10000 to the scores before the softmax (V:352-355), and the masked mean over time of the
classification head (V:1031-1042).  Test infrastructure only; the oracle itself is untouched."""
import math

import torch

from oracle import wav2vec2_oracle as V
from oracle.whisper_oracle import dense, gelu_erf, layer_norm

MASK_VALUE = -10000.0  # V:354


def masked_attention(q, k, v, scale, mask=None):
    """q [B, H, Tq, hd], k / v [B, H, Tk, hd], mask [B, Tk] in [0, 1] or None -> (context [B, H, Tq, hd], probabilities)."""
    s = (q @ k.transpose(-1, -2)) * scale
    if mask is not None:
        s = s + ((1.0 - mask.to(s.dtype)) * MASK_VALUE)[:, None, None, :]
    p = torch.softmax(s, dim=-1)
    return p @ v, p


def masked_attention_naive(q, k, v, scale, mask=None):
    """The same thing one row at a time, written without broadcasting (the check of ``masked_attention``)."""
    B, H, Tq, hd = q.shape
    Tk = k.shape[2]
    out = torch.zeros(B, H, Tq, hd, dtype=q.dtype)
    for b in range(B):
        for h in range(H):
            for i in range(Tq):
                row = torch.empty(Tk, dtype=q.dtype)
                for j in range(Tk):
                    row[j] = float((q[b, h, i] * k[b, h, j]).sum()) * scale
                    if mask is not None:
                        row[j] += (1.0 - float(mask[b, j])) * MASK_VALUE
                e = torch.exp(row - row.max())
                out[b, h, i] = (e / e.sum()) @ v[b, h]
    return out


def attention(p, prefix, x, num_heads, mask=None):
    """V:333-376 with an attention_mask."""
    B, T, H = x.shape
    hd = H // num_heads

    def split(t):
        return t.reshape(B, T, num_heads, hd).permute(0, 2, 1, 3)

    q = split(dense(x, p[f"{prefix}.q_proj.kernel"], p[f"{prefix}.q_proj.bias"]))
    k = split(dense(x, p[f"{prefix}.k_proj.kernel"], p[f"{prefix}.k_proj.bias"]))
    v = split(dense(x, p[f"{prefix}.v_proj.kernel"], p[f"{prefix}.v_proj.bias"]))
    ctx, _ = masked_attention(q, k, v, 1.0 / math.sqrt(hd), mask)
    ctx = ctx.permute(0, 2, 1, 3).reshape(B, T, H)
    return dense(ctx, p[f"{prefix}.out_proj.kernel"], p[f"{prefix}.out_proj.bias"])


def encoder_layer(p, prefix, x, cfg, mask=None):
    """V:419-439 (stable layer norm), training=False."""
    h = layer_norm(x, p[f"{prefix}.attention_layer_norm.gamma"], p[f"{prefix}.attention_layer_norm.beta"], cfg.layer_norm_eps)
    x = x + attention(p, f"{prefix}.attention", h, cfg.num_attention_heads, mask)
    h = layer_norm(x, p[f"{prefix}.feed_forward_layer_norm.gamma"], p[f"{prefix}.feed_forward_layer_norm.beta"], cfg.layer_norm_eps)
    h = gelu_erf(dense(h, p[f"{prefix}.feed_forward.intermediate_dense.kernel"], p[f"{prefix}.feed_forward.intermediate_dense.bias"]))
    return x + dense(h, p[f"{prefix}.feed_forward.output_dense.kernel"], p[f"{prefix}.feed_forward.output_dense.bias"])


def masked_mean(x, mask=None):
    """V:1031-1042: sum_t x mask / sum_t mask; the plain mean without a mask."""
    if mask is None:
        return x.mean(dim=1)
    m = mask.to(x.dtype)
    return (x * m[:, :, None]).sum(dim=1) / m.sum(dim=1, keepdim=True)


def forward(p, audio, cfg, mask=None):
    """V:768-825 with training=False -> last_hidden_state, extract_features, hidden_states (V:488-537), pooled_output."""
    assert V.DROPOUT_PROVIDER is None
    dtype = p["feature_projection.kernel"].dtype
    feats = V.feature_extractor(p, audio.to(dtype), cfg)
    h = dense(feats, p["feature_projection.kernel"], p["feature_projection.bias"])
    x = layer_norm(h, p["feature_projection_layer_norm.gamma"], p["feature_projection_layer_norm.beta"], cfg.layer_norm_eps)
    hidden = []
    for i in range(cfg.num_hidden_layers):
        hidden.append(x)
        x = encoder_layer(p, f"encoder.layers.{i}", x, cfg, mask)
    hidden.append(x)
    return {"last_hidden_state": x, "extract_features": feats, "hidden_states": tuple(hidden), "pooled_output": masked_mean(x, mask)}
