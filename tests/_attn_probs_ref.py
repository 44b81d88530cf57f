"""Float64 truth for the attention weights (tmi_attn_probs, ``output_attentions``).  Test infrastructure only.

Kernel level: ``probs_ref`` - the softmax of scale * q.k^T on bf16-rounded q, k in float64.  mask_mode 1 follows
``test_attention_forms_gpu._scores`` (the reference's -1e9 added in fp32 to keys j <= i, which absorbs the score); mask_mode
2 adds ``key_bias`` [B, Tk] to the scores of every head and query.

Model level: float64 forwards of both models that also return every layer's attention weights and input.  They are built
from the unchanged oracle primitives (``dense``, ``layer_norm``, ``gelu_erf``, ``conv1d_same``, ``feed_forward``,
``decoder_mask``, the Wav2Vec2 feature extractor) and the pieces of tests/_w2v_infer_ref.py; only the attention function
is restated, because the oracle's ``mha`` does not return ``probs``.  tests/test_attn_probs_cpu.py holds the restated
forwards against the oracle's own."""
import math

import torch

import _w2v_infer_ref as R
from oracle import wav2vec2_oracle as V
from oracle import whisper_oracle as O
from oracle.whisper_oracle import dense, layer_norm

LOG2E = 1.4426950408889634


# ----------------------------------------------------------------------------- kernel level
def scores_ref(q, k, mask_mode, scale, key_bias=None):
    """q [B, H, Tq, 64], k [B, H, Tk, 64] float64 -> the scores the softmax sees, natural-log units, [B, H, Tq, Tk]."""
    s = (q @ k.transpose(-1, -2)) * scale
    if mask_mode == 1:
        i, j = torch.arange(q.shape[-2]), torch.arange(k.shape[-2])
        masked = j[None, :] <= i[:, None]
        s = torch.where(masked, (s.float() + torch.tensor(-1e9, dtype=torch.float32)).double(), s)
    elif mask_mode == 2:
        s = s + key_bias.double()[:, None, None, :]
    return s


def probs_ref(q, k, mask_mode, scale, key_bias=None):
    return torch.softmax(scores_ref(q, k, mask_mode, scale, key_bias), dim=-1)


# ----------------------------------------------------------------------------- Whisper
def whisper_mha(p, prefix, hidden, kv_states, mask, num_heads):
    """W:106-176 with training=False, returning (output, attention_probs [B, H, Tq, Tk]) as W:176 does.  The mask is added
    in float32, as in the oracle's ``mha``."""
    B, Tq, d = hidden.shape
    hd = d // num_heads
    src = hidden if kv_states is None else kv_states
    k = dense(src, p[f"{prefix}.k_proj.kernel"], p[f"{prefix}.k_proj.bias"])
    v = dense(src, p[f"{prefix}.v_proj.kernel"], p[f"{prefix}.v_proj.bias"])
    q = dense(hidden, p[f"{prefix}.q_proj.kernel"], p[f"{prefix}.q_proj.bias"]) * hd ** -0.5

    def split(t):
        return t.reshape(B, -1, num_heads, hd).permute(0, 2, 1, 3)

    q, k, v = split(q), split(k), split(v)
    scores = q @ k.transpose(-1, -2)
    if mask is not None:
        add = (1.0 - mask.to(torch.float32)) * O.MASK_VALUE
        summed32 = scores.to(torch.float32) + add
        scores = torch.where((add != 0).expand_as(scores), summed32.to(scores.dtype), scores)
    probs = torch.softmax(scores, dim=-1)
    ctx = (probs @ v).permute(0, 2, 1, 3).reshape(B, Tq, d)
    return dense(ctx, p[f"{prefix}.out_proj.kernel"], p[f"{prefix}.out_proj.bias"]), probs


def _ln(p, name, x, cfg):
    return layer_norm(x, p[f"{name}.gamma"], p[f"{name}.beta"], cfg.layer_norm_eps)


def whisper_forward(p, feats, dec_ids, cfg):
    """W:547-616 with training=False on decoder input ``dec_ids`` [B, S] -> the outputs of the reference's call: logits,
    last_hidden_state, encoder_last_hidden_state, and per layer encoder_attentions, decoder_attentions, cross_attentions,
    encoder_hidden_states, decoder_hidden_states (the INPUT of every layer, W:348-349 / W:427-428)."""
    assert O.DROPOUT_PROVIDER is None and O.FP32_MASK_ROUNDING
    dtype = p["lm_head.kernel"].dtype
    x = feats.to(dtype).transpose(1, 2)
    x = O.gelu_erf(O.conv1d_same(x, p["encoder.conv1.kernel"], p["encoder.conv1.bias"], 1))
    x = O.gelu_erf(O.conv1d_same(x, p["encoder.conv2.kernel"], p["encoder.conv2.bias"], 2))
    x = x + torch.from_numpy(O.positional_encoding(cfg.n_ctx, cfg.d_model)).to(dtype)[: x.shape[1]]
    out = {k: [] for k in ("encoder_attentions", "decoder_attentions", "cross_attentions", "encoder_hidden_states",
                           "decoder_hidden_states")}
    for i in range(cfg.encoder_layers):
        pre = f"encoder.layers.{i}"
        out["encoder_hidden_states"].append(x)
        h, probs = whisper_mha(p, f"{pre}.self_attn", _ln(p, f"{pre}.self_attn_layer_norm", x, cfg), None, None,
                               cfg.encoder_attention_heads)
        out["encoder_attentions"].append(probs)
        x = x + h
        x = x + O.feed_forward(p, f"{pre}.feed_forward", _ln(p, f"{pre}.final_layer_norm", x, cfg), cfg, False)
    enc = _ln(p, "encoder.layer_norm", x, cfg)

    y = p["decoder.embed_tokens.embeddings"][dec_ids.long()]
    y = y + torch.from_numpy(O.positional_encoding(cfg.max_target_positions, cfg.d_model)).to(dtype)[: y.shape[1]]
    mask = torch.from_numpy(O.decoder_mask(dec_ids.shape[1]))[None]
    Hd = cfg.decoder_attention_heads
    for i in range(cfg.decoder_layers):
        pre = f"decoder.layers.{i}"
        out["decoder_hidden_states"].append(y)
        h, probs = whisper_mha(p, f"{pre}.self_attn", _ln(p, f"{pre}.self_attn_layer_norm", y, cfg), None, mask, Hd)
        out["decoder_attentions"].append(probs)
        y = y + h
        h, probs = whisper_mha(p, f"{pre}.encoder_attn", _ln(p, f"{pre}.encoder_attn_layer_norm", y, cfg), enc, None, Hd)
        out["cross_attentions"].append(probs)
        y = y + h
        y = y + O.feed_forward(p, f"{pre}.feed_forward", _ln(p, f"{pre}.final_layer_norm", y, cfg), cfg, False)
    last = _ln(p, "decoder.layer_norm", y, cfg)
    res = {k: tuple(v) for k, v in out.items()}
    res.update(logits=last @ p["lm_head.kernel"], last_hidden_state=last, encoder_last_hidden_state=enc)
    return res


# ----------------------------------------------------------------------------- Wav2Vec2
def w2v_attention(p, prefix, x, num_heads, mask=None):
    """V:333-376 with an attention_mask, returning (output, probabilities [B, Hh, T, T])."""
    B, T, H = x.shape
    hd = H // num_heads

    def split(t):
        return t.reshape(B, T, num_heads, hd).permute(0, 2, 1, 3)

    q = split(dense(x, p[f"{prefix}.q_proj.kernel"], p[f"{prefix}.q_proj.bias"]))
    k = split(dense(x, p[f"{prefix}.k_proj.kernel"], p[f"{prefix}.k_proj.bias"]))
    v = split(dense(x, p[f"{prefix}.v_proj.kernel"], p[f"{prefix}.v_proj.bias"]))
    ctx, probs = R.masked_attention(q, k, v, 1.0 / math.sqrt(hd), mask)
    ctx = ctx.permute(0, 2, 1, 3).reshape(B, T, H)
    return dense(ctx, p[f"{prefix}.out_proj.kernel"], p[f"{prefix}.out_proj.bias"]), probs


def w2v_forward(p, audio, cfg, mask=None):
    """V:768-825 with training=False -> last_hidden_state, extract_features, hidden_states (the input of every layer and the
    output of the last), attentions (one [B, Hh, T, T] per layer)."""
    assert V.DROPOUT_PROVIDER is None
    dtype = p["feature_projection.kernel"].dtype
    feats = V.feature_extractor(p, audio.to(dtype), cfg)
    h = dense(feats, p["feature_projection.kernel"], p["feature_projection.bias"])
    x = _ln(p, "feature_projection_layer_norm", h, cfg)
    hidden, atts = [], []
    for i in range(cfg.num_hidden_layers):
        pre = f"encoder.layers.{i}"
        hidden.append(x)
        a, probs = w2v_attention(p, f"{pre}.attention", _ln(p, f"{pre}.attention_layer_norm", x, cfg), cfg.num_attention_heads, mask)
        atts.append(probs)
        x = x + a
        h = O.gelu_erf(dense(_ln(p, f"{pre}.feed_forward_layer_norm", x, cfg), p[f"{pre}.feed_forward.intermediate_dense.kernel"],
                             p[f"{pre}.feed_forward.intermediate_dense.bias"]))
        x = x + dense(h, p[f"{pre}.feed_forward.output_dense.kernel"], p[f"{pre}.feed_forward.output_dense.bias"])
    hidden.append(x)
    return {"last_hidden_state": x, "extract_features": feats, "hidden_states": tuple(hidden), "attentions": tuple(atts)}
