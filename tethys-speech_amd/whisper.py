"""Whisper encoder-decoder training step on the HIP kernels (host orchestration).

Mirrors the reference's operator API for this path (speech_jobs/whisper_dist.py, "W:"):
``WhisperConfig`` (W:10-45), ``create_whisper_model(model_type)`` (W:852-890) and a model
object whose ``forward_backward(features, labels)`` does what ``model(features,
labels=..., training=True)`` + ``tape.gradient`` do at W:826-833.  The forward/backward is
written out by hand (no autograd): every tensor op is a C-ABI call from ``ops``.

Two precisions:
  "fp32"  parity mode — fp32 activations, exact-fp32 MFMA GEMMs reading the fp32 master
          weights, attention in the reference's own materialised-score shape (W:147-167).
  "bf16"  perf mode — bf16 activations and bf16 weight shadows, fused flash attention,
          fp32 accumulation, fp32 gradients/optimizer state.
Dropout (W:29-30) is off by default (parity mode: TF's RNG stream cannot be reproduced, so a step with
dropout has no parity definition against the reference).  ``enable_dropout`` turns on the
reference's training-mode sites (W:160, W:205, W:342, W:411) on the bf16 path with counter-based masks
(tmi_dropout / the fused attention kernels); the oracle fed the same masks is the checker.

Beam search (``generate(num_beams=K)``, 2 <= K <= 8; the reference leaves it a ``pass`` at W:696-698).  Row r = b*K + k
is beam k of batch item b.  Step t (1-based) reads prefix columns [0, t) and writes column t.  lp_r(v) =
log_softmax(z_r / temperature)[v] over the V real columns (temperature as at W:678; top_k, top_p and min_length are
accepted and ignored, as in greedy); with decode constraints z_r is the constrained logit z' of include/tethys_mi.h, the
softmax runs over the columns that are not banned, and with a prompt of P tokens every prefix is P longer while t, the
scores and t**length_penalty keep counting generated tokens.
  Start: running sums s_{b,0} = 0, s_{b,k>0} = -inf; every beam holds [decoder_start_token_id].
  Per step, for each item not done: the candidates (k, v, s_k + lp_k(v)) ordered by score desc, then k*V + v asc; the
    first 2K are kept (each row's top 2K of lp_k suffices).  Walk the ranks j = 0 .. 2K-1: an EOS candidate at j < K is
    offered to the pool (the parent prefix + EOS, length t, score s / t**length_penalty), at j >= K it is skipped; any
    other candidate becomes the next live beam, in rank order, until K are live (there are always K: each beam has one
    EOS column).
  Pool: at most K hypotheses per item, ordered by score desc then insertion asc; admitted while not full, then one
    replaces the last entry only with a strictly greater score.
  Done: the pool is full and either early_stopping, or its worst score >= max(new live sums) / t**length_penalty (the
    early_stopping=False heuristic).  A done item is frozen: later steps change none of its state, its live rows keep
    valid ids (so a step queued after the stop is harmless).
  Stop: at the first step where every item is done (read one step late, as greedy), or after max_length steps.
  Finalize: every item not done offers its live beams, k = 0 .. K-1, to its pool (length n, score s_k / n**length_penalty).
  Output: the best num_return_sequences R of each item, int32 [B*R, 1 + n_out] (start token first, pad_token_id after
    the hypothesis, n_out the longest returned length); return_dict_in_generate: {"sequences", "sequences_scores" fp32
    [B*R], "lengths"}.  eos_token_id = -1: no hypothesis ends early.
The t**length_penalty factors are rounded to fp32 once, on the host; the kernels' only arithmetic on scores is one fp32
add per candidate and correctly rounded divisions.
"""
from __future__ import annotations

import json
import math
import os
from dataclasses import dataclass
from typing import Dict, List, Tuple

import numpy as np
import torch

from . import ops
from .blocks import Arena, KernelBlocks, _round_up


# ----------------------------------------------------------------------------- config
# dropout site ids (seed = f(base, step, site), KernelBlocks._site_seed; restated in oracle/dropout.py)
SITE_ENC_STEM, SITE_DEC_EMBED = 1, 2
SITE_ENC_ATTN, SITE_ENC_FFN, SITE_DEC_SELF, SITE_DEC_CROSS, SITE_DEC_FFN = 100, 200, 300, 400, 500
_STEM_SLACK = 2  # rows of zero slack behind the padded stem inputs, so the padded-K tail reads of the last window stay in bounds


@dataclass
class WhisperConfig:  # W:10-45
    d_model: int = 768
    encoder_layers: int = 4
    encoder_attention_heads: int = 12
    decoder_layers: int = 4
    decoder_attention_heads: int = 12
    d_ff: int = 3072
    n_mels: int = 80
    n_ctx: int = 1500
    vocab_size: int = 51865
    max_target_positions: int = 448
    dropout: float = 0.1
    attention_dropout: float = 0.1
    activation_dropout: float = 0.0
    layer_norm_eps: float = 1e-5
    pad_token_id: int = 0
    bos_token_id: int = 1
    eos_token_id: int = 2
    decoder_start_token_id: int = 50257


_SIZES = {  # W:859-886
    "tiny": dict(d_model=384, encoder_layers=4, encoder_attention_heads=6, decoder_layers=4,
                 decoder_attention_heads=6, d_ff=1536),
    "base": dict(d_model=512, encoder_layers=6, encoder_attention_heads=8, decoder_layers=6,
                 decoder_attention_heads=8, d_ff=2048),
    "small": dict(),
    "medium": dict(d_model=1024, encoder_layers=24, encoder_attention_heads=16, decoder_layers=24,
                   decoder_attention_heads=16, d_ff=4096),
    "large": dict(d_model=1280, encoder_layers=32, encoder_attention_heads=20, decoder_layers=32,
                  decoder_attention_heads=20, d_ff=5120),
}


def make_config(model_type: str = "small", **overrides) -> WhisperConfig:
    cfg = WhisperConfig()
    for k, v in _SIZES.get(model_type, {}).items():
        setattr(cfg, k, v)
    for k, v in overrides.items():
        setattr(cfg, k, v)
    return cfg


def same_pad(T: int, k: int, s: int) -> Tuple[int, int, int]:
    """TensorFlow "SAME": -> (T_out, pad_left, pad_right)."""
    out = -(-T // s)
    total = max((out - 1) * s + k - T, 0)
    return out, total // 2, total - total // 2


def _repeat_rows_per_item(kv: torch.Tensor, B: int, K: int):
    """In place on ``kv`` [B*K, ...] whose first B row blocks hold one block per item: item b's block -> the blocks
    b*K .. b*K + K - 1 (K beams or return sequences per item), from the back so that no source is overwritten first."""
    for b in range(B - 1, -1, -1):
        kv[b * K + (1 if b == 0 else 0):(b + 1) * K].copy_(kv[b:b + 1].expand(K - (1 if b == 0 else 0), -1, -1))


def positional_encoding(max_len: int, d_model: int) -> np.ndarray:
    """W:49-69."""
    pe = np.zeros((max_len, d_model))
    position = np.arange(0, max_len)[:, np.newaxis]
    div_term = np.exp(np.arange(0, d_model, 2) * -(np.log(10000.0) / d_model))
    pe[:, 0::2] = np.sin(position * div_term)
    pe[:, 1::2] = np.cos(position * div_term)
    return pe.astype(np.float32)


# ----------------------------------------------------------------------------- parameters
class ParamArena(Arena):
    """All trainable parameters in ONE flat fp32 buffer (plus same-shaped grad / Adam m / v
    buffers), in forward order so that backward fills the gradient arena from its end
    towards its start: all-reduce buckets are contiguous slices, ready in reverse order.

    Storage tensors fuse the reference's separate q/k/v Dense kernels column-wise
    ([d, 3d] for self-attention, [d, 2d] k|v for cross-attention); ``ref_views`` exposes
    them under the reference's own variable paths as strided views.
    """

    def __init__(self, cfg: WhisperConfig, device):
        self.cfg = cfg
        d, ff, V = cfg.d_model, cfg.d_ff, cfg.vocab_size
        spec: List[Tuple[str, Tuple[int, ...]]] = []

        def ln(p):
            spec.append((f"{p}.gamma", (d,)))
            spec.append((f"{p}.beta", (d,)))

        def ffn(p):
            spec.extend([(f"{p}.fc1.kernel", (d, ff)), (f"{p}.fc1.bias", (ff,)),
                         (f"{p}.fc2.kernel", (ff, d)), (f"{p}.fc2.bias", (d,))])

        spec.append(("encoder.conv1.kernel", (3, cfg.n_mels, d)))
        spec.append(("encoder.conv1.bias", (d,)))
        spec.append(("encoder.conv2.kernel", (3, d, d)))
        spec.append(("encoder.conv2.bias", (d,)))
        for i in range(cfg.encoder_layers):
            p = f"encoder.layers.{i}"
            ln(f"{p}.self_attn_layer_norm")
            spec.extend([(f"{p}.self_attn.qkv.kernel", (d, 3 * d)), (f"{p}.self_attn.qkv.bias", (3 * d,)),
                         (f"{p}.self_attn.out_proj.kernel", (d, d)), (f"{p}.self_attn.out_proj.bias", (d,))])
            ln(f"{p}.final_layer_norm")
            ffn(f"{p}.feed_forward")
        ln("encoder.layer_norm")
        spec.append(("decoder.embed_tokens.embeddings", (V, d)))
        # W:122-123 projects the encoder output to k/v in every decoder layer: the L kernels are stored
        # side by side as one [d, L*2d] matrix, so those projections (forward, dgrad, wgrad) are one GEMM
        # each per step instead of L (reference variables = column slices, see Arena.ref_views)
        if cfg.decoder_layers:
            spec.extend([("decoder.cross_kv.kernel", (d, cfg.decoder_layers * 2 * d)),
                         ("decoder.cross_kv.bias", (cfg.decoder_layers * 2 * d,))])
        for i in range(cfg.decoder_layers):
            p = f"decoder.layers.{i}"
            ln(f"{p}.self_attn_layer_norm")
            spec.extend([(f"{p}.self_attn.qkv.kernel", (d, 3 * d)), (f"{p}.self_attn.qkv.bias", (3 * d,)),
                         (f"{p}.self_attn.out_proj.kernel", (d, d)), (f"{p}.self_attn.out_proj.bias", (d,))])
            ln(f"{p}.encoder_attn_layer_norm")
            spec.extend([(f"{p}.encoder_attn.q_proj.kernel", (d, d)), (f"{p}.encoder_attn.q_proj.bias", (d,)),
                         (f"{p}.encoder_attn.out_proj.kernel", (d, d)), (f"{p}.encoder_attn.out_proj.bias", (d,))])
            ln(f"{p}.final_layer_norm")
            ffn(f"{p}.feed_forward")
        ln("decoder.layer_norm")
        # the LM head is STORED with its vocab axis padded to a multiple of 64 (zero columns that
        # stay zero under Adam: g = 0 => m = v = 0 => no update), so logits / dlogits rows are
        # 16-byte aligned and the vocab-long reductions are whole K tiles; logical shape (d, V)
        self.v_pad = _round_up(V, 64)
        spec.append(("lm_head.kernel", (d, self.v_pad)))
        self.logical: Dict[str, Tuple[int, ...]] = {"lm_head.kernel": (d, V)}

        super().__init__(spec, device, logical=self.logical, fuse_width=d)


# ----------------------------------------------------------------------------- model
class WhisperForConditionalGeneration(KernelBlocks):
    """W:536-616: the training step, the forward-only pass and greedy generate.  Holds parameters, bf16 shadows and all activation
    workspaces; sized lazily for a batch size on first use."""

    def __init__(self, config: WhisperConfig, device="cuda:0", precision: str = "bf16", seed: int = 1234):
        if precision not in ("fp32", "bf16"):
            raise ValueError("precision must be 'fp32' or 'bf16'")
        ops.lib()  # fail loudly now if the HIP library is missing
        self.config = config
        self.device = torch.device(device)
        self.precision = precision
        self.dtype = torch.float32 if precision == "fp32" else torch.bfloat16
        self.hidden = config.d_model
        self.layer_norm_eps = config.layer_norm_eps
        self.arena = ParamArena(config, self.device)
        self.arena.init_keras_defaults(seed)
        d = config.d_model
        if d % config.encoder_attention_heads or d % config.decoder_attention_heads:
            raise ValueError("d_model must divide by the head counts")
        if precision == "bf16" and (d // config.encoder_attention_heads != 64 or d // config.decoder_attention_heads != 64):
            raise ValueError("the fused attention kernel is built for head_dim 64")
        self.pe_enc = torch.from_numpy(positional_encoding(config.n_ctx, d)).to(self.device)
        self.pe_dec = torch.from_numpy(positional_encoding(config.max_target_positions, d)).to(self.device)
        self.pe_enc_t = self.pe_enc.to(self.dtype)
        self._ws_key = None
        self.ws: Dict[str, torch.Tensor] = {}
        self._ws_sets: Dict[tuple, Dict[str, torch.Tensor]] = {}
        # bf16 mirror of the whole parameter arena (perf mode), same flat indexing: every
        # kernel in its natural Keras [in, out] layout.  Forward reads it k-strided (hardware
        # transposed LDS reads), dgrad reads it k-contiguous.  Written by the Adam kernel itself.
        self.mirror = None
        if precision == "bf16":
            self.mirror = torch.zeros(self.arena.numel, dtype=torch.bfloat16, device=self.device)
            self.refresh_shadows()
        # weight / bias gradients on a second stream beside the dgrad chain (blocks.KernelBlocks)
        self.enable_wgrad_stream(os.environ.get("TMI_WGRAD_STREAM", "1") != "0")

    # -- workspaces --------------------------------------------------------------------
    def _stem_geometry(self, T_in: int) -> dict:
        """TF "SAME" geometry of the conv stem (W:329-339) for ``T_in`` frames: conv1 (stride 1) gives T1 rows from the
        padded input of Tp0 rows, conv2 (stride 2) the encoder length T from Tp1.  Shared by training and inference."""
        cfg = self.config
        T1, pl1, pr1 = same_pad(T_in, 3, 1)
        T, pl2, pr2 = same_pad(T1, 3, 2)
        if T > cfg.n_ctx:
            raise ValueError("encoder length exceeds n_ctx")
        # conv1's reduction length 3*n_mels (240) is not a multiple of the GEMM's 64-deep K tile: the bf16
        # path multiplies against a copy of the kernel padded with zero rows, so the tile-aligned kernels
        # apply; the extra A columns are the next frames of xp0 (finite, inside the slack) times zero
        K1p = -(-3 * cfg.n_mels // 64) * 64
        w1pad = self.precision == "bf16" and K1p != 3 * cfg.n_mels and K1p - 3 * cfg.n_mels <= _STEM_SLACK * cfg.n_mels
        return {"T1": T1, "pl1": pl1, "pr1": pr1, "T": T, "pl2": pl2, "pr2": pr2, "Tp0": T_in + pl1 + pr1,
                "Tp1": T1 + pl2 + pr2, "K1p": K1p, "w1pad": w1pad}

    def _stem_bufs(self, B: int, geo: dict):
        """The stem's inputs: the padded features, conv1's padded output, the padded conv1 kernel (bf16)."""
        d, z = self.config.d_model, dict(zero=True)
        self._buf("xp0", (B, geo["Tp0"] + _STEM_SLACK, self.config.n_mels), **z)
        self._buf("h1pad", (B, geo["Tp1"] + _STEM_SLACK, d), **z)
        if geo["w1pad"]:
            self._buf("w1pad", (geo["K1p"], d), **z)
        else:
            self.ws.pop("w1pad", None)

    def _prepare(self, B: int, T_in: int, S: int):
        if self._select_ws_set((B, T_in, S)):
            return
        cfg = self.config
        if S > cfg.max_target_positions:
            raise ValueError("target length exceeds max_target_positions")
        geo = self._geo = self._stem_geometry(T_in)
        # (the shape attributes model.T, model.T1, ...: tests, tools and bench read them)
        self.T1, self.pl1, self.pr1, self.T, self.pl2, self.pr2, self.Tp0, self.Tp1, self.K1p = (
            geo[n] for n in ("T1", "pl1", "pr1", "T", "pl2", "pr2", "Tp0", "Tp1", "K1p"))
        d, ff = cfg.d_model, cfg.d_ff
        f32 = torch.float32
        z = dict(zero=True)
        self._stem_bufs(B, geo)
        self._buf("u1pad", (B, self.Tp1 + _STEM_SLACK, d), **z)
        self._buf("dh1pad", (B, self.Tp1 + _STEM_SLACK, d), **z)
        self._buf("u2", (B, self.T, d))
        self._buf("du2pad", (B, self.T + 1, d), **z)
        R, Rd = B * self.T, B * S
        # decoder: the operands of the six weight gradients per layer live at a constant layer stride (one allocation per
        # kind) - the saved activations xn1 / ctx / xn2 / ctxc / xn3 / g and the gradients dqkv / dyos / dqc / dyoc / dU /
        # dyf each Dense layer receives - so that ONE batched GEMM per kind computes it for all layers after the decoder's
        # backward loop (KernelBlocks._wgrad_batched; the encoder's layers are chip-sized GEMMs and keep their own launches)
        for n, shp in (("xn1", (Rd, d)), ("ctx", (Rd, d)), ("xn2", (Rd, d)), ("ctxc", (Rd, d)), ("xn3", (Rd, d)), ("g", (Rd, ff)),
                       ("dqkv", (Rd, 3 * d)), ("dyos", (Rd, d)), ("dqc", (Rd, d)), ("dyoc", (Rd, d)), ("dU", (Rd, ff)),
                       ("dyf", (Rd, d))):
            self._buf_layers("dec", cfg.decoder_layers, n, shp)
        for side, L, rows in (("enc", cfg.encoder_layers, R), ("dec", cfg.decoder_layers, Rd)):
            for i in range(L):
                p = f"{side}{i}."
                self._buf(p + "x_in", (rows, d))
                if side == "enc":
                    self._buf(p + "xn1", (rows, d))
                    self._buf(p + "ctx", (rows, d))
                    self._buf(p + "xn2", (rows, d))
                    self._buf(p + "g", (rows, ff))
                self._buf(p + "qkv", (rows, 3 * d))
                self._buf(p + "x_mid", (rows, d))
                self._buf(p + "u", (rows, ff))
                for s_ in ("ln1", "ln2"):
                    self._buf(p + s_ + ".mean", (rows,), f32)
                    self._buf(p + s_ + ".rstd", (rows,), f32)
                if side == "dec":
                    self._buf(p + "x_mid2", (rows, d))
                    self._buf(p + "qc", (rows, d))
                    self._buf(p + "ln3.mean", (rows,), f32)
                    self._buf(p + "ln3.rstd", (rows,), f32)
        self._buf("enc_x", (R, d))
        self._buf("enc_out", (R, d))
        self._buf("enc_ln.mean", (R,), f32)
        self._buf("enc_ln.rstd", (R,), f32)
        self._buf("dec_x", (Rd, d))
        self._buf("dec_out", (Rd, d))
        self._buf("dec_ln.mean", (Rd,), f32)
        self._buf("dec_ln.rstd", (Rd,), f32)
        self.ldl = self.arena.v_pad
        self._buf("logits", (Rd, self.ldl), **z)
        self._buf("row_loss", (Rd,), f32)
        self._buf("loss", (1,), f32)
        # the weighted loss (decoder_attention_mask): row weights and 1 / their sum, written on the device each step; part of
        # every set so that a plan recorded with a mask finds them at the addresses it baked in
        self._buf("row_w", (Rd,), f32)
        self._buf("inv_wsum", (1,), f32)
        # backward scratch, shared by every layer
        Rm = max(R, Rd)
        self._buf("dres_enc", (R, d))
        self._buf("dres_dec", (Rd, d))
        self._buf("d_enc_out", (R, d))
        self._buf("dtmp", (Rm, d))
        if self.precision == "bf16":
            self._buf("lmh_dx32", (Rd, d), f32)  # split-K accumulator of the LM-head dgrad
        self._buf("dctx", (Rm, d))
        self._buf("dctxc0", (B * S, d)); self._buf("dctxc1", (B * S, d))  # dO of the cross-attention backward (alternating by layer)
        if self._drop_p > 0.0:
            # masked copies of the residual-stream gradient (dropout mode): two buffers used by alternate layers, so a
            # layer's mask pass does not have to wait for the previous layer's weight gradient, which still reads its copy
            self._buf("dyd0", (Rm, d))
            self._buf("dyd1", (Rm, d))
        self._buf("dqkv", (Rm, 3 * d))
        Lkv = max(1, cfg.decoder_layers) * 2 * d
        self._buf("kvc_all", (R, Lkv))   # cross-attention k/v of every decoder layer, side by side
        self._buf("dkv_all", (R, Lkv))
        self._buf("dU", (Rm, ff))
        He, Hd = cfg.encoder_attention_heads, cfg.decoder_attention_heads
        if self.precision == "bf16":
            for i in range(cfg.encoder_layers):
                self._buf(f"enc{i}.stats", (B, He, self.T, 2), f32)
            for i in range(cfg.decoder_layers):
                self._buf(f"dec{i}.stats", (B, Hd, S, 2), f32)
                self._buf(f"dec{i}.statsc", (B, Hd, S, 2), f32)
            self._buf("delta", (B, max(He, Hd), max(self.T, S)), f32)
        else:
            for i in range(cfg.encoder_layers):
                self._buf(f"enc{i}.P", (B, He, self.T, self.T), f32)
            for i in range(cfg.decoder_layers):
                self._buf(f"dec{i}.P", (B, Hd, S, S), f32)
                self._buf(f"dec{i}.Pc", (B, Hd, S, self.T), f32)
            self._buf("dP", (B, max(He, Hd), max(self.T, S), self.T), f32)

    # -- forward blocks, shared by the training step and the forward-only pass ---------------------------------------
    # Each takes a map of its buffers: training passes the layer's own workspace entries (kept for backward), inference
    # buffers every layer shares, without the GELU pre-activation ``u`` (None).  ``sites``: the dropout sites apply (the
    # training step; inference runs without dropout even after enable_dropout).  Buffer-map keys: activations x_in, xn1,
    # qkv, ctx, x_mid, xn2, g, u (encoder layer, decoder self block; qc for the cross-attention query), ctxc, x_mid2, xn3
    # (decoder cross block), x_out (the next layer's input), kvc (every decoder layer's cross-attention k|v); the names of
    # the LayerNorm statistics ln1 / ln2 / ln3 and of the attention scratch att / attc.

    def _stem(self, features, geo, x, u1pad=None, u2=None):
        """W:329-339: conv1 + GELU into ws["h1pad"] (its pad rows stay zero), conv2 + GELU + positional encoding into
        ``x`` [B*T, d].  ``u1pad`` / ``u2``: where training keeps the pre-activations for backward."""
        ws, a, d = self.ws, self.arena, self.config.d_model
        B, Cn, T_in = features.shape
        xp0, h1pad, w1pad = ws["xp0"], ws["h1pad"], ws.get("w1pad")
        ops.feat_to_channels_last(features, xp0, B, Cn, T_in, geo["pl1"], geo["pr1"] + (xp0.shape[1] - geo["Tp0"]))
        conv1_out = dict(ldc=d, nbatch=B, a_sb=xp0.stride(0), c_sb=h1pad.stride(0), c_off=geo["pl2"] * d,
                         bias=a.param("encoder.conv1.bias"), act=1, aux_out=u1pad)
        if w1pad is not None:
            ops.copy(w1pad[:3 * Cn], self.W("encoder.conv1.kernel")[0])
            ops.gemm(xp0, w1pad, h1pad, geo["T1"], d, geo["K1p"], Cn, 1, d, 1, **conv1_out)
        else:
            self._gemm_xw(xp0, "encoder.conv1.kernel", h1pad, geo["T1"], d, 3 * Cn, Cn, **conv1_out)
        T = geo["T"]
        self._gemm_xw(h1pad, "encoder.conv2.kernel", x, T, d, 3 * d, 2 * d, ldc=d, nbatch=B, a_sb=h1pad.stride(0),
                      c_sb=T * d, bias=a.param("encoder.conv2.bias"), act=1, aux_out=u2, resid=self.pe_enc_t,
                      r_ld=d, r_sb=0)

    def _enc_layer(self, i, b, B, T, sites, capture=None):
        """W:218-236: encoder layer i, b["x_in"] -> b["x_out"].  ``capture`` (inference, ``_Capture``): collects the layer's
        input and its attention weights when they were asked for."""
        cfg, d = self.config, self.config.d_model
        p, He = f"encoder.layers.{i}", cfg.encoder_attention_heads
        if capture is not None:
            capture.layer_input("encoder", b["x_in"], B, T, d)
        self._ln_fwd(b["x_in"], p + ".self_attn_layer_norm", b["xn1"], b["ln1"])
        self._dense_fwd(b["xn1"], p + ".self_attn.qkv.kernel", b["qkv"], scale_cols=d, scale=(d // He) ** -0.5)
        qkv = b["qkv"]
        self._attn_fwd(b["att"], (qkv, 0), (qkv, d), (qkv, 2 * d), b["ctx"], B, He, T, T, 0,
                       site=SITE_ENC_ATTN + i if sites else None)
        if capture is not None and capture.wants("encoder"):
            capture.attention("encoder", self._attn_probs(b["att"], (qkv, 0), (qkv, d), B, He, T, T, 0, dtype=capture.dtype))
        self._dense_fwd(b["ctx"], p + ".self_attn.out_proj.kernel", b["x_mid"], resid=b["x_in"], r_ld=d)
        self._ln_fwd(b["x_mid"], p + ".final_layer_norm", b["xn2"], b["ln2"])
        self._dense_fwd(b["xn2"], p + ".feed_forward.fc1.kernel", b["g"], act=1, aux_out=b["u"])
        # W:205: x_mid + Dropout(fc2(g)): the mask is a term of the GEMM epilogue (before the residual add)
        self._dense_fwd(b["g"], p + ".feed_forward.fc2.kernel", b["x_out"], resid=b["x_mid"], r_ld=d,
                        **(self._drop_epi(SITE_ENC_FFN + i) if sites else {}))

    def _dec_self_block(self, i, b, B, S, sites, capture=None):
        """Decoder layer i (W:394-466) up to the cross-attention query: needs nothing from the encoder."""
        cfg, d = self.config, self.config.d_model
        p, Hd = f"decoder.layers.{i}", cfg.decoder_attention_heads
        scal = (d // Hd) ** -0.5
        if capture is not None:
            capture.layer_input("decoder", b["x_in"], B, S, d)
        self._ln_fwd(b["x_in"], p + ".self_attn_layer_norm", b["xn1"], b["ln1"])
        self._dense_fwd(b["xn1"], p + ".self_attn.qkv.kernel", b["qkv"], scale_cols=d, scale=scal)
        qkv = b["qkv"]
        # the inverted mask of W:416-418 (mask_mode 1): each query sees the strictly later positions only
        self._attn_fwd(b["att"], (qkv, 0), (qkv, d), (qkv, 2 * d), b["ctx"], B, Hd, S, S, 1,
                       site=SITE_DEC_SELF + i if sites else None)
        if capture is not None and capture.wants("decoder"):
            capture.attention("decoder", self._attn_probs(b["att"], (qkv, 0), (qkv, d), B, Hd, S, S, 1, dtype=capture.dtype))
        self._dense_fwd(b["ctx"], p + ".self_attn.out_proj.kernel", b["x_mid"], resid=b["x_in"], r_ld=d)
        # cross attention (W:278-290): k/v projections of the encoder output in every layer
        self._ln_fwd(b["x_mid"], p + ".encoder_attn_layer_norm", b["xn2"], b["ln2"])
        self._dense_fwd(b["xn2"], p + ".encoder_attn.q_proj.kernel", b["qc"], scale_cols=d, scale=scal)

    def _dec_cross_ffn(self, i, b, B, S, T, sites, capture=None):
        """Decoder layer i from its cross-attention on: b["x_mid"] -> b["x_out"]."""
        cfg, d = self.config, self.config.d_model
        p, Hd, kvc = f"decoder.layers.{i}", cfg.decoder_attention_heads, b["kvc"]
        self._attn_fwd(b["attc"], (b["qc"], 0), (kvc, 2 * i * d), (kvc, (2 * i + 1) * d), b["ctxc"], B, Hd, S, T, 0,
                       site=SITE_DEC_CROSS + i if sites else None)
        if capture is not None and capture.wants("cross"):
            capture.attention("cross", self._attn_probs(b["attc"], (b["qc"], 0), (kvc, 2 * i * d), B, Hd, S, T, 0,
                                                        dtype=capture.dtype))
        self._dense_fwd(b["ctxc"], p + ".encoder_attn.out_proj.kernel", b["x_mid2"], resid=b["x_mid"], r_ld=d)
        self._ln_fwd(b["x_mid2"], p + ".final_layer_norm", b["xn3"], b["ln3"])
        self._dense_fwd(b["xn3"], p + ".feed_forward.fc1.kernel", b["g"], act=1, aux_out=b["u"])
        self._dense_fwd(b["g"], p + ".feed_forward.fc2.kernel", b["x_out"], resid=b["x_mid2"], r_ld=d,
                        **(self._drop_epi(SITE_DEC_FFN + i) if sites else {}))

    def _train_bufs(self, side, i, L):
        """Training's buffer map of layer i of ``side`` ("enc" / "dec", L layers): the layer's own workspace entries."""
        ws, k = self.ws, f"{side}{i}."
        att = ("stats", "statsc") if self.precision == "bf16" else ("P", "Pc")
        b = {n: ws[k + n] for n in ("x_in", "xn1", "qkv", "ctx", "x_mid", "xn2", "g", "u")}
        b.update(ln1=k + "ln1", ln2=k + "ln2", att=k + att[0],
                 x_out=ws[f"{side}{i + 1}.x_in"] if i + 1 < L else ws[f"{side}_x"])
        if side == "dec":
            b.update({n: ws[k + n] for n in ("qc", "ctxc", "x_mid2", "xn3")})
            b.update(ln3=k + "ln3", attc=k + att[1], kvc=ws["kvc_all"])
        return b

    def embedding_tables(self):
        """(arena offset, rows, row length) of the tf.keras.layers.Embedding tables (W:382): rows that never see a
        gradient are skipped by the optimizer (optim.Adam._update)."""
        name = "decoder.embed_tokens.embeddings"
        V, d = self.arena.shapes[name]
        return [(self.arena.offsets[name], V, d)]

    def grad_ready_names(self) -> List[str]:
        """The parameters at which backward reports "everything stored at or after this one is final", in the
        order it reports them (arena order reversed).  The data-parallel strategy launches its buckets from
        these reports, so a replica with nothing to compute (an empty slice of a short final batch) walks the
        same list: every rank then issues the same collectives in the same order."""
        cfg = self.config
        names = ["decoder.layer_norm.gamma"]
        names += [f"decoder.layers.{i}.self_attn_layer_norm.gamma" for i in reversed(range(cfg.decoder_layers))]
        if cfg.decoder_layers:
            names.append("decoder.cross_kv.kernel")
        names += ["decoder.embed_tokens.embeddings", "encoder.layer_norm.gamma"]
        names += [f"encoder.layers.{i}.self_attn_layer_norm.gamma" for i in reversed(range(cfg.encoder_layers))]
        names.append("encoder.conv1.kernel")
        return names

    def report_zero_gradients(self, grad_ready=None):
        """The gradient arena of a replica whose slice of the batch is empty: zeros, reported through
        ``grad_ready`` range by range exactly as a real backward would."""
        a = self.arena
        a.g.zero_()
        a.g_clean = False
        hi = a.numel
        for name in self.grad_ready_names():
            lo = a.offsets[name]
            if grad_ready is not None and lo < hi:
                grad_ready(lo, hi)
                hi = lo

    # -- forward -------------------------------------------------------------------------
    def late_adam_range(self):
        """Arena range whose first reader in a step is the decoder, a whole encoder forward after the step began: the
        cross-attention k/v projection, the decoder layers and the decoder's final LayerNorm (the embedding table before
        it and the LM head after it are the EARLY slices).  None when there is no such range (no decoder layers)."""
        a = self.arena
        if not self.config.decoder_layers or "decoder.cross_kv.kernel" not in a.offsets:
            return None
        # (an "enc" slice for the upper encoder layers, ahead of this one on the stream and waited for at its first layer, was
        # measured too: from layer 1 the chain waits for it, +0.3 ms; from layer 2 it is level, 8.30 vs 8.32 ms - not kept)
        return [(a.offsets["decoder.cross_kv.kernel"], a.offsets["lm_head.kernel"], "dec")]

    def early_adam_ranges(self):
        """The two variables whose gradients are final while the decoder's backward still runs (the EARLY slices):
        the LM head (last in the arena) and the decoder's embedding table."""
        a = self.arena
        e_lo = a.offsets["decoder.embed_tokens.embeddings"]
        return [(a.offsets["lm_head.kernel"], a.numel), (e_lo, e_lo + a.grad("decoder.embed_tokens.embeddings").numel())]

    def forward_backward(self, features: torch.Tensor, labels: torch.Tensor, loss_scale: float = 1.0,
                         grad_ready=None, early_update=None, decoder_attention_mask=None):
        """Pins the launch stream for the duration of the step (KernelBlocks.begin_step), then runs
        ``_forward_backward``.

        ``decoder_attention_mask`` [B, S] (None: the plain mean over B*(S-1) positions, W:600): the reference's weighted
        loss (W:596-598), wgt = mask[:, :-1] (column S-1 is ignored),
          loss = sum(wgt * nll) / sum(wgt)
        with non-negative real weights, not only 0/1, as in ``evaluate``.  The mask weights the LOSS only: the decoder keeps
        the reference's inverted triangular mask (W:509 hands the [B, S] mask to the decoder in place of the [1, S, S] one,
        which cannot broadcast - the same reading as ``evaluate``).  A float32 device tensor is used as it is; a bool /
        integer / other float mask is converted once, here, before the step; a host array goes through
        ``check_evaluate_args`` (shape, no negative entry) and is uploaded.  Shape and dtype errors raise on the host; the
        step never reads the mask, or its sum, back: the normaliser stays in device memory (tmi_xent_weights), so one
        recorded launch plan serves every mask.  Rows of weight 0 are not read by the loss kernel (gradient +0, whatever
        the logits hold).  A mask whose weights are all 0 gives loss 0 and zero gradients - the reference would divide 0 by
        0; an empty replica already contributes zeros the same way.  With replicas every replica normalises by the sum of
        its OWN weights and the gradients are summed (W:829-836)."""
        mask = None
        if decoder_attention_mask is not None:
            mask = prepare_loss_mask(self.config, tuple(labels.shape), decoder_attention_mask, self.device)
        self.begin_step()
        try:
            return self._forward_backward(features, labels, loss_scale, grad_ready, early_update, mask)
        finally:
            self.end_step()
            self._drop_step += 1  # next step draws fresh masks

    def _forward_backward(self, features: torch.Tensor, labels: torch.Tensor, loss_scale: float = 1.0,
                         grad_ready=None, early_update=None, loss_mask=None):
        """One replica's forward + backward (W:826-833).  features [B, n_mels, T_in] fp32,
        labels [B, S] int32, both on the device.  Gradients land in ``arena.g`` (which is
        zeroed first); returns the device scalar loss (mean over B*(S-1), W:600).
        ``grad_ready(lo, hi)`` is called during backward each time the gradients of the arena
        range [lo, hi) are final, last range first (the data-parallel strategy all-reduces them
        under the rest of backward).  ``loss_mask``: ``forward_backward``'s decoder_attention_mask as a float32 [B, S] device
        tensor (the weighted mean of W:596-598 instead).  ``early_update(lo, hi)`` (optim.Adam.begin_early, one replica): the optimizer
        update of an arena range, called on the second stream as soon as that range's gradients are final and its
        weights have been read for the last time in this step - the LM head and the embedding table, under the
        decoder's backward chain."""
        cfg = self.config
        B, Cn, T_in = features.shape
        S = labels.shape[1]
        if Cn != cfg.n_mels or labels.shape[0] != B:
            raise ValueError("bad batch shapes")
        if features.dtype != torch.float32 or labels.dtype != torch.int32:
            raise TypeError("features must be float32 and labels int32")
        self._prepare(B, T_in, S)
        ws, a, d = self.ws, self.arena, cfg.d_model
        T, Hd = self.T, cfg.decoder_attention_heads
        if not getattr(a, "g_clean", False):
            self._wait_late()  # (a pending late Adam slice reads the gradients this fill would overwrite)
            ops.fill_zero(a.g)  # (an optimizer step with zero_grad leaves the arena clean: no fill pass)
        a.g_clean = False
        done = [a.numel]
        expected = iter(self.grad_ready_names())

        def ready(name):
            """Everything stored at or after parameter ``name`` now has its final gradient."""
            if name != next(expected, None):
                raise RuntimeError(f"backward reported {name} out of the order grad_ready_names() promises")
            lo = a.offsets[name]
            if grad_ready is not None and lo < done[0]:
                # (a consumer that acts on the range at once must first order itself after the
                # weight-gradient stream: DataParallelStrategy does so through its pre_launch hook)
                grad_ready(lo, done[0])
                done[0] = lo

        drop = self._drop_p > 0.0
        Le, Ld = cfg.encoder_layers, cfg.decoder_layers
        dec_bufs = [self._train_bufs("dec", i, Ld) for i in range(Ld)]

        def dec_embed():
            """ids = [start, labels[:, :-1]] (W:559-563) inside the embedding kernel."""
            y = ws["dec0.x_in"] if Ld else ws["dec_x"]
            ops.embed_fwd(labels, a.param("decoder.embed_tokens.embeddings"), self.pe_dec, y, B, S, d,
                          cfg.decoder_start_token_id)
            if drop:
                self._dropout(y, y, SITE_DEC_EMBED)  # W:411

        # The decoder's embedding and layer 0 up to its cross-attention query depend on the labels only: a chain of
        # ~10 decoder-sized kernels that would otherwise sit, alone on the chip, between the encoder and the decoder.
        # They run on the second stream beside the encoder's forward.
        early_dec = self._side is not None and Ld > 0 and self._main is not None
        if early_dec:
            self._run_on_side(lambda: (dec_embed(), self._dec_self_block(0, dec_bufs[0], B, S, True)), labels)
            early_ev = self._pop_side_reads(labels)
        # ---- encoder stem (W:329-339) and layers (W:218-236)
        x = ws["enc0.x_in"] if Le else ws["enc_x"]
        self._stem(features, self._geo, x, u1pad=ws["u1pad"], u2=ws["u2"])
        if drop:
            self._dropout(x, x, SITE_ENC_STEM)  # W:342
        for i in range(Le):
            self._enc_layer(i, self._train_bufs("enc", i, Le), B, T, True)
        self._ln_fwd(ws["enc_x"], "encoder.layer_norm", ws["enc_out"], "enc_ln")
        enc_out = ws["enc_out"]

        # ---- decoder (W:394-466)
        self._wait_late()  # the previous step's late Adam slices, if they were left running (train.ADAM_LATE)
        if not early_dec:
            dec_embed()
        kvc, kv_rest = ws["kvc_all"], None
        if Ld:
            if self._side is not None and Ld > 1:
                # W:122-123 for all layers: layer 0's k/v now (its cross-attention is next), the other layers' as ONE
                # GEMM on the second stream under decoder layer 0's chain of small kernels
                self._dense_fwd(enc_out, "decoder.cross_kv.kernel", kvc, n_off=0, n_cols=2 * d)
                self._run_on_side(lambda: self._dense_fwd(enc_out, "decoder.cross_kv.kernel", kvc[:, 2 * d:], n_off=2 * d,
                                                          n_cols=(Ld - 1) * 2 * d), enc_out)
                kv_rest = self._pop_side_reads(enc_out)
            else:
                self._dense_fwd(enc_out, "decoder.cross_kv.kernel", kvc)
        for i in range(Ld):
            if not (early_dec and i == 0):
                self._dec_self_block(i, dec_bufs[i], B, S, True)
            else:
                self._wait_events(early_ev)  # layer 0's self-attention block ran beside the encoder
            if i == 1 and kv_rest is not None:
                self._wait_events(kv_rest)
            self._dec_cross_ffn(i, dec_bufs[i], B, S, T, True)
        self._ln_fwd(ws["dec_x"], "decoder.layer_norm", ws["dec_out"], "dec_ln")

        # ---- LM head + shifted cross-entropy (W:579-600); logits become dlogits in place
        V = cfg.vocab_size
        logits = ws["logits"]
        wl, ldw = self.W("lm_head.kernel")
        Vp = self.ldl  # pad columns of the stored kernel are zero: their logits are 0 and ignored by xent
        self._gemm_xw(ws["dec_out"], "lm_head.kernel", logits, B * S, Vp, d, d, ldc=Vp)
        lm = (ws["dec_out"], d, wl, ldw, 1, d)
        if loss_mask is None:
            gs = loss_scale / (B * (S - 1))
            # (tmi_linear_xent: the loss's target logit in fp32 from the LM head's own operands - bf16 logits have lost its low bits)
            ops.xent_fwd_bwd(logits, self.ldl, labels, ws["row_loss"], B, S, V, gs, lm=lm)
            ops.sum_scale(ws["row_loss"], ws["loss"], B * S, 1.0 / (B * (S - 1)))
        else:
            # W:596-598: the per-row scale loss_scale * w / sum(w) is formed on the device (no host read of the sum)
            ops.xent_weights(loss_mask, B, S, ws["row_w"], ws["inv_wsum"])
            ops.xent_fwd_bwd_weighted(logits, self.ldl, labels, ws["row_w"], ws["inv_wsum"], ws["row_loss"], B, S, V, loss_scale,
                                      lm=lm)
            ops.sum_scale_dev(ws["row_loss"], ws["loss"], B * S, ws["inv_wsum"])

        # ================= backward =================
        dres = ws["dres_dec"]
        dW = a.grad("lm_head.kernel")
        # the LM head's weight gradient (K = B*S rows against a [d, 51904] output: 120 us) feeds nothing on the chain: second
        # stream, under the decoder's backward (a chain of decoder-sized kernels on a mostly idle chip)
        self._run_on_side(lambda: ops.gemm(ws["dec_out"], logits, dW, d, Vp, B * S, 1, d, Vp, 1, Vp, splitk=0), logits)
        dtmp = ws["dtmp"][:B * S]
        # dgrad over the padded vocab (pad columns of dlogits are zero): a whole number of K tiles
        # (K = 51904 against only B*S x d outputs: in bf16 mode reduce it split-K into fp32 and round once)
        if self.precision == "bf16":
            acc = ws["lmh_dx32"]
            ops.fill_zero(acc)
            ops.gemm(logits, wl, acc, B * S, d, Vp, Vp, 1, 1, ldw, d, splitk=0)
            ops.cast_bf16(acc, d, dtmp, d, B * S, d)
        else:
            # (fp32 mode: the same split of the 51904-deep reduction, straight into the fp32 result)
            self._guard_write(dtmp)
            ops.fill_zero(dtmp)
            ops.gemm(logits, wl, dtmp, B * S, d, Vp, Vp, 1, 1, ldw, d, splitk=0)
        if early_update is not None:
            # lm_head: gradient final (weight gradient above, same stream), weights read for the last time by the dgrad just
            # enqueued on the main stream (the event _run_on_side records here orders the update behind it)
            lm_lo = a.offsets["lm_head.kernel"]
            # (keyed by a buffer nothing in backward rewrites: a _guard_write on the key would make the chain wait for Adam)
            self._run_on_side(lambda: early_update(lm_lo, a.numel), ws["row_loss"])
        # Column sums (bias gradients) and Dropout-masked copies of the residual-stream gradient come out of the LayerNorm
        # backward that produces it (tmi_layernorm_bwd_emit): ffn_emit(side, i) = what layer i's fc2 needs of the dres
        # handed down to it - its bias gradient and its dy: in the decoder, dres (under the mask of W:205 with dropout) in
        # the layer's own buffer, which the batched weight gradient reads after the loop; in the encoder, with dropout,
        # the masked dres in one of two alternating buffers (a layer's weight gradient on the second stream may still be
        # reading the other one)
        def ffn_emit(side, i, rows):
            if i < 0:
                return None
            if side == "dec":
                return (a.grad(f"decoder.layers.{i}.feed_forward.fc2.bias"), ws[f"dec{i}.dyf"], SITE_DEC_FFN + i)
            return (a.grad(f"encoder.layers.{i}.feed_forward.fc2.bias"), ws[f"dyd{i & 1}"][:rows] if drop else None,
                    SITE_ENC_FFN + i)

        self._ln_bwd(dtmp, ws["dec_x"], "decoder.layer_norm", dres, "dec_ln", False, emit=ffn_emit("dec", Ld - 1, B * S))
        ready("decoder.layer_norm.gamma")

        # Decoder weight gradients are batched over the layers after the loop: 24 launches of 13-26 us on B*S = 800 rows
        # become 6 with L times the tiles (KernelBlocks._wgrad_batched).  Every Dense layer's dy is kept in a per-layer
        # buffer: dU / dqc / dqkv are written there by the kernels that produce them, the residual-stream gradients (dyf,
        # dyoc, dyos) are the second output of the LayerNorm backward above them.
        d_enc, dkv = ws["d_enc_out"], ws["dkv_all"]
        Rd = B * S
        dt_, dctx = ws["dtmp"][:Rd], ws["dctx"][:Rd]
        for i in reversed(range(Ld)):
            p, k = f"decoder.layers.{i}", f"dec{i}."
            # FFN (with dropout the branch sees the masked gradient: the same mask, regenerated)
            self._dense_bwd(ws[k + "g"], ws[k + "dyf"], p + ".feed_forward.fc2.kernel", ws[k + "dU"], aux_in=ws[k + "u"],
                            wgrad=False)
            self._dense_bwd(ws[k + "xn3"], ws[k + "dU"], p + ".feed_forward.fc1.kernel", dt_, wgrad=False)
            self._ln_bwd(dt_, ws[k + "x_mid2"], p + ".final_layer_norm", dres, k + "ln3", True,
                         emit=(a.grad(p + ".encoder_attn.out_proj.bias"), ws[k + "dyoc"], None))
            # cross attention: dK / dV feed only the shared k/v projections' backward after the loop, so their pass runs on the
            # second stream (its dO lives in a buffer of its own: the chain rewrites ws["dctx"] two kernels later)
            dctxc = ws[f"dctxc{i & 1}"][:Rd]
            self._dense_bwd(ws[k + "ctxc"], ws[k + "dyoc"], p + ".encoder_attn.out_proj.kernel", dctxc, wgrad=False)
            dqc = ws[k + "dqc"]
            self._attn_bwd(k + ("statsc" if self.precision == "bf16" else "Pc"), (ws[k + "qc"], 0),
                           (kvc, 2 * i * d), (kvc, (2 * i + 1) * d), ws[k + "ctxc"], dctxc, (dqc, 0),
                           (dkv, 2 * i * d), (dkv, (2 * i + 1) * d), B, Hd, S, T, 0, site=SITE_DEC_CROSS + i,
                           dkv_on_side=True)
            self._dense_bwd(ws[k + "xn2"], dqc, p + ".encoder_attn.q_proj.kernel", dctx, wgrad=False)
            self._ln_bwd(dctx, ws[k + "x_mid"], p + ".encoder_attn_layer_norm", dres, k + "ln2", True,
                         emit=(a.grad(p + ".self_attn.out_proj.bias"), ws[k + "dyos"], None))
            # self attention
            self._dense_bwd(ws[k + "ctx"], ws[k + "dyos"], p + ".self_attn.out_proj.kernel", dctx, wgrad=False)
            qkv, dqkv = ws[k + "qkv"], ws[k + "dqkv"]
            self._attn_bwd(k + ("stats" if self.precision == "bf16" else "P"), (qkv, 0), (qkv, d), (qkv, 2 * d),
                           ws[k + "ctx"], dctx, (dqkv, 0), (dqkv, d), (dqkv, 2 * d), B, Hd, S, S, 1, site=SITE_DEC_SELF + i)
            self._dense_bwd(ws[k + "xn1"], dqkv, p + ".self_attn.qkv.kernel", dt_, wgrad=False)
            self._ln_bwd(dt_, ws[k + "x_in"], p + ".self_attn_layer_norm", dres, k + "ln1", True, emit=ffn_emit("dec", i - 1, Rd))
        if Ld:
            # every layer's dk / dv is in place (their passes ran on the second stream: join it): one weight gradient, one
            # bias gradient and one dgrad (K = L*2d) for the cross-attention k/v projections of all layers
            self._join_side()
            self._dense_bwd(enc_out, dkv, "decoder.cross_kv.kernel", d_enc)
            st = {n: ws[f"dec*.{n}"] for n in ("xn1", "ctx", "xn2", "ctxc", "xn3", "g", "dqkv", "dyos", "dqc", "dyoc", "dU", "dyf")}
            lay = "decoder.layers.{}"

            def decoder_weight_grads():
                # (the biases of the residual-stream layers came out of the LayerNorm backward)
                self._wgrad_batched(st["g"], st["dyf"], lay + ".feed_forward.fc2.kernel", Ld, bias=False)
                self._wgrad_batched(st["xn3"], st["dU"], lay + ".feed_forward.fc1.kernel", Ld)
                self._wgrad_batched(st["ctxc"], st["dyoc"], lay + ".encoder_attn.out_proj.kernel", Ld, bias=False)
                self._wgrad_batched(st["xn2"], st["dqc"], lay + ".encoder_attn.q_proj.kernel", Ld)
                self._wgrad_batched(st["ctx"], st["dyos"], lay + ".self_attn.out_proj.kernel", Ld, bias=False)
                self._wgrad_batched(st["xn1"], st["dqkv"], lay + ".self_attn.qkv.kernel", Ld)
            # on the second stream, under the start of the encoder's backward
            self._run_on_side(decoder_weight_grads, st["dqkv"])
            for i in reversed(range(Ld)):
                ready(f"decoder.layers.{i}.self_attn_layer_norm.gamma")
            ready("decoder.cross_kv.kernel")
        # the embedding's backward (mask of W:411, scatter of the rows) feeds nothing on the chain: second stream
        gemb, dres_dec = a.grad("decoder.embed_tokens.embeddings"), dres

        def embed_backward():
            if drop:
                ops.dropout(dres_dec, dres_dec, dres_dec.shape[0], dres_dec.shape[1], self._drop_p, self._site_seed(SITE_DEC_EMBED))
            ops.embed_bwd(labels, dres_dec, gemb, B, S, d, cfg.decoder_start_token_id)
            if early_update is not None:  # the table's gradient is final; its forward read happened long ago
                e_lo = a.offsets["decoder.embed_tokens.embeddings"]
                early_update(e_lo, e_lo + gemb.numel())
        self._run_on_side(embed_backward, dres_dec)
        ready("decoder.embed_tokens.embeddings")

        # ---- encoder backward
        dres = ws["dres_enc"]
        if Ld == 0:
            ops.fill_zero(d_enc)
        R, He = B * T, cfg.encoder_attention_heads
        self._ln_bwd(d_enc, ws["enc_x"], "encoder.layer_norm", dres, "enc_ln", False, emit=ffn_emit("enc", Le - 1, R))
        ready("encoder.layer_norm.gamma")
        dU, dt_, dctx, dqkv = ws["dU"][:R], ws["dtmp"][:R], ws["dctx"][:R], ws["dqkv"][:R]
        for i in reversed(range(Le)):
            p, k = f"encoder.layers.{i}", f"enc{i}."
            dy = ws[f"dyd{i & 1}"][:R] if drop else dres
            self._dense_bwd(ws[k + "g"], dy, p + ".feed_forward.fc2.kernel", dU, aux_in=ws[k + "u"], bias_done=True)
            self._dense_bwd(ws[k + "xn2"], dU, p + ".feed_forward.fc1.kernel", dt_)
            self._ln_bwd(dt_, ws[k + "x_mid"], p + ".final_layer_norm", dres, k + "ln2", True,
                         emit=(a.grad(p + ".self_attn.out_proj.bias"), None, None))
            self._dense_bwd(ws[k + "ctx"], dres, p + ".self_attn.out_proj.kernel", dctx, bias_done=True)
            qkv = ws[k + "qkv"]
            self._attn_bwd(k + ("stats" if self.precision == "bf16" else "P"), (qkv, 0), (qkv, d), (qkv, 2 * d),
                           ws[k + "ctx"], dctx, (dqkv, 0), (dqkv, d), (dqkv, 2 * d), B, He, T, T, 0, site=SITE_ENC_ATTN + i)
            self._dense_bwd(ws[k + "xn1"], dqkv, p + ".self_attn.qkv.kernel", dt_)
            self._ln_bwd(dt_, ws[k + "x_in"], p + ".self_attn_layer_norm", dres, k + "ln1", True, emit=ffn_emit("enc", i - 1, R))
            ready(p + ".self_attn_layer_norm.gamma")

        # ---- stem backward: x0 = gelu(u2) + PE ; u2 = conv2(h1) ; h1 = gelu(u1) ; u1 = conv1(x)
        if drop:
            self._dropout(dres, dres, SITE_ENC_STEM)
        xp0, h1pad, u1pad, du2pad, dh1pad = ws["xp0"], ws["h1pad"], ws["u1pad"], ws["du2pad"], ws["dh1pad"]
        du2 = du2pad[:, 1:]  # row 0 of every batch stays zero (the "t-1" term of the first output)
        # one launch over the B per-sample spans (du2 skips the zero row 0 of every sample)
        ops.gelu_bwd_batched(dres, ws["u2"], du2, T * d, B, T * d, T * d, du2pad.stride(0))
        # the pad rows of du2pad are zero, so the bias gradient is one column sum over the whole buffer
        gw2 = a.grad("encoder.conv2.kernel").view(3 * d, d)

        def conv2_weight_grads():
            ops.bias_grad(du2pad.view(-1, d), a.grad("encoder.conv2.bias"))
            ops.gemm(h1pad, du2pad, gw2, 3 * d, d, T, 1, 2 * d, d, 1, d, kbatch=B, a_skb=h1pad.stride(0),
                     b_skb=du2pad.stride(0), b_off=d, splitk=0)
        # conv2's weight gradient (88 us + its split-K reduce) feeds nothing on the chain: beside the two dgrad launches
        # below (du2pad and h1pad are not rewritten before the join)
        self._run_on_side(conv2_weight_grads, du2pad)
        w2, ld2 = self.W("encoder.conv2.kernel")
        sd = du2pad.stride(0)
        # even padded rows u = 2j: dY[j]·W0ᵀ + dY[j-1]·W2ᵀ  (kbatch walks the two kernel taps)
        ops.gemm(du2pad, w2, dh1pad, T, d, d, d, 1, 1, ld2, 2 * d, nbatch=B, a_sb=sd, c_sb=dh1pad.stride(0),
                 kbatch=2, a_skb=-d, b_skb=2 * d * ld2, a_off=d, aux_in=u1pad)
        # odd padded rows u = 2j + 1: dY[j]·W1ᵀ
        ops.gemm(du2pad, w2, dh1pad, T, d, d, d, 1, 1, ld2, 2 * d, nbatch=B, a_sb=sd, c_sb=dh1pad.stride(0),
                 a_off=d, b_off=d * ld2, c_off=d, aux_in=u1pad)
        if self.pl2:
            ops.fill_zero(dh1pad[:, :self.pl2])
        ops.fill_zero(dh1pad[:, self.pl2 + self.T1:])
        ops.bias_grad(dh1pad.view(-1, d), a.grad("encoder.conv1.bias"))  # (pad rows were just zeroed)
        gw1 = a.grad("encoder.conv1.kernel").view(3 * Cn, d)
        ops.gemm(xp0, dh1pad, gw1, 3 * Cn, d, self.T1, 1, Cn, d, 1, d, kbatch=B, a_skb=xp0.stride(0),
                 b_skb=dh1pad.stride(0), b_off=self.pl2 * d, splitk=0)
        ready("encoder.conv1.kernel")
        self._join_side()
        return ws["loss"]

    def __call__(self, features, decoder_input_ids=None, labels=None, training=None, output_attentions=False,
                 output_hidden_states=False, attentions_dtype=None, decoder_attention_mask=None):
        """Reference call surface (W:547-616).  ``training=True`` (the default when labels are given): the training step,
        {"loss": ...} with the gradients as a side effect (W:829).  ``training=False``: the forward pass alone (no dropout,
        no gradients, nothing of the training state touched) -> {"loss": None, "logits" [B, S, V], "last_hidden_state"
        [B, S, d], "encoder_last_hidden_state" [B, T, d]}, in the model's compute dtype.  The decoder reads
        ``decoder_input_ids`` [B, S] (their first column must be the start token: every sequence the reference feeds its
        decoder starts with it, W:559-563 / W:663), else ``labels`` shifted right behind the start token (W:555-563), else
        the start token alone.  ``output_attentions`` / ``output_hidden_states`` / ``attentions_dtype``: the inference call's
        extra outputs, see ``forward_infer``.  ``decoder_attention_mask`` [B, S]: the loss weights of the training step
        (W:596-598, see ``forward_backward``); the forward-only call computes no loss and refuses it (``evaluate`` takes it)."""
        if training is None:
            training = labels is not None
        if training:
            if labels is None or decoder_input_ids is not None:
                raise ValueError("the training path takes labels (and forms the decoder input from them itself)")
            if output_attentions or output_hidden_states or attentions_dtype is not None:
                raise ValueError("output_attentions, output_hidden_states and attentions_dtype belong to the inference call "
                                 "(training=False)")
            return {"loss": self.forward_backward(features, labels, decoder_attention_mask=decoder_attention_mask)}
        if decoder_attention_mask is not None:
            raise ValueError("decoder_attention_mask weights the loss: it belongs to the training call and to evaluate()")
        return self.forward_infer(features, decoder_input_ids=decoder_input_ids, labels=labels,
                                  output_attentions=output_attentions, output_hidden_states=output_hidden_states,
                                  attentions_dtype=attentions_dtype)

    # -- inference (forward only): W:547-616 with training=False, greedy generate W:636-709 --------------------------
    # Its own workspace set (``_inf``), never one of ``_ws_sets``: the per-layer activations training keeps for backward are
    # not needed, so every layer of a stack shares one set of buffers, sized for the encoder's B*T rows or the decoder's
    # B*max_target_positions rows, whichever is more; one attention scratch (softmax statistics, or the fp32 path's P) serves
    # every attention call.  Swapped in as ``self.ws`` only for the duration of an inference call (the blocks read
    # ``self.ws``); nothing else of the training state (``_ws_key``, the shape attributes, ``_drop_step``, the optimizer,
    # recorded plans) is read or written, and no dropout site is passed (dropout is off even after enable_dropout).

    def _infer_prepare(self, B: int, T_in: int, K: int = 1) -> dict:
        """The inference workspace for B encoder rows and B * K decoder rows (K beams per item; K = 1: greedy)."""
        cfg = self.config
        inf = self.__dict__.get("_inf")
        if inf is not None and inf["key"] == (B, T_in, K):
            return inf
        self._inf = None  # (the previous set is released first)
        geo = self._stem_geometry(T_in)
        T, d, ff, Smax = geo["T"], cfg.d_model, cfg.d_ff, cfg.max_target_positions
        He, Hd = cfg.encoder_attention_heads, cfg.decoder_attention_heads
        inf = dict(geo, key=(B, T_in, K))
        saved, self.ws = self.ws, {}
        try:
            self._stem_bufs(B, geo)
            BK = B * K
            R, Rd = B * T, BK * Smax
            Rm = max(R, Rd)
            for n, w in (("x", d), ("x_mid", d), ("x_mid2", d), ("xn", d), ("ctx", d), ("qc", d), ("qkv", 3 * d), ("g", ff)):
                self._buf(n, (Rm, w))
            self._buf("ln.mean", (Rm,), torch.float32)
            self._buf("ln.rstd", (Rm,), torch.float32)
            self._buf("enc_out", (R, d))
            self._buf("kvc_all", (BK * T, max(1, cfg.decoder_layers) * 2 * d))  # (k|v of item b in rows of b * K .. + K)
            if self.precision == "bf16":
                n_att = BK * max(He, Hd) * max(T, Smax) * 2
            else:
                n_att = max(B * He * T * T, BK * Hd * Smax * max(Smax, T))
            self._buf("att_flat", (n_att,), torch.float32)
            self._buf("labels", (Rd,), torch.int32)
            self._buf("argmax_ws", (B + 1,), torch.int64, zero=True)  # tmi_lm_head_argmax leaves it zero again
            if K > 1:  # tmi_lm_head_topk's, N = 2K candidates per row; left zero again too
                self._buf("topk_ws", (ops.lm_head_topk_workspace_elems(BK, cfg.vocab_size, 2 * K),), torch.int64, zero=True)
            inf["ws"] = self.ws
        finally:
            self.ws = saved
        self._inf = inf
        return inf

    def _sample_workspace(self, inf, B: int, top_k: int):
        """tmi_lm_head_sample's workspace for B rows and this top_k, added to the inference set ``inf`` on the sampled path
        only (nothing else of the set depends on the mode); zero before the first call, left zero by every call."""
        need = ops.lm_head_sample_workspace_elems(B, self.config.vocab_size, top_k)
        have = inf["ws"].get("sample_ws")
        if have is None or have.numel() < need:
            inf["ws"]["sample_ws"] = torch.zeros(need, dtype=torch.int64, device=self.device)

    def _att(self, key, B, H, Tq, Tk):
        """The shared attention scratch as call ``key``'s statistics [B, H, Tq, 2] (bf16) or scores [B, H, Tq, Tk] (fp32)."""
        flat = self.ws["att_flat"]
        shape = (B, H, Tq, 2) if self.precision == "bf16" else (B, H, Tq, Tk)
        self.ws[key] = flat[:int(np.prod(shape))].view(shape)
        return key

    def _infer_bufs(self, rows):
        """Inference's buffer map: every layer of a stack works in the same shared buffers, ``rows`` rows of each; one
        LayerNorm-statistics buffer, no GELU pre-activation, each layer's output overwrites its input."""
        x, x_mid, x_mid2, xn, ctx, qc, qkv, g = (self.ws[n][:rows] for n in ("x", "x_mid", "x_mid2", "xn", "ctx", "qc", "qkv", "g"))
        return {"x_in": x, "xn1": xn, "qkv": qkv, "ctx": ctx, "x_mid": x_mid, "xn2": xn, "g": g, "u": None, "qc": qc,
                "ctxc": ctx, "x_mid2": x_mid2, "xn3": xn, "x_out": x, "ln1": "ln", "ln2": "ln", "ln3": "ln"}

    def _encode_infer(self, features, inf, capture=None):
        """W:324-372 with training=False into ws["enc_out"] [B*T, d]: the training forward's blocks, the pre-activations
        backward would need not saved."""
        cfg = self.config
        B, T = features.shape[0], inf["T"]
        b = self._infer_bufs(B * T)
        b["att"] = self._att("att", B, cfg.encoder_attention_heads, T, T)
        self._stem(features, inf, b["x_in"])
        for i in range(cfg.encoder_layers):
            self._enc_layer(i, b, B, T, False, capture)
        self._ln_fwd(b["x_in"], "encoder.layer_norm", self.ws["enc_out"], "ln")
        return self.ws["enc_out"]

    def _cross_kv_infer(self, enc_out):
        """W:122-123 for every decoder layer at once: the cross-attention k|v, computed once per encoder output."""
        if self.config.decoder_layers:
            self._dense_fwd(enc_out, "decoder.cross_kv.kernel", self.ws["kvc_all"][:enc_out.shape[0]])

    def _decode_infer(self, labels, B, S, T, capture=None, kvc=None):
        """W:394-466 (training=False) over S positions without the final LayerNorm: returns the residual stream
        [B*S, d].  ``labels`` [B, S] int32: the decoder reads [start, labels[:, :-1]] (tmi_embed_fwd's shift).  ``kvc``: the
        cross-attention k|v rows [B*T, layers * 2d] of these B rows when they are not the first B of ws["kvc_all"]."""
        cfg = self.config
        Hd = cfg.decoder_attention_heads
        b = self._infer_bufs(B * S)
        b.update(att=self._att("att", B, Hd, S, S), attc=self._att("attc", B, Hd, S, T),
                 kvc=self.ws["kvc_all"][:B * T] if kvc is None else kvc)
        ops.embed_fwd(labels, self.arena.param("decoder.embed_tokens.embeddings"), self.pe_dec, b["x_in"], B, S, cfg.d_model,
                      cfg.decoder_start_token_id)
        for i in range(cfg.decoder_layers):
            self._dec_self_block(i, b, B, S, False, capture)
            self._dec_cross_ffn(i, b, B, S, T, False, capture)
        return b["x_in"]

    def _check_features(self, features):
        if features.dim() != 3 or features.shape[1] != self.config.n_mels:
            raise ValueError(f"features must be [B, {self.config.n_mels}, T_in]")
        if features.dtype != torch.float32:
            raise TypeError("features must be float32")
        if features.shape[0] < 1:
            raise ValueError("empty batch")
        return features.to(self.device).contiguous()

    @torch.no_grad()
    def forward_infer(self, features, decoder_input_ids=None, labels=None, output_attentions=False,
                      output_hidden_states=False, attentions_dtype=None):
        """The forward pass alone (W:547-616, training=False); see ``__call__``.

        ``output_attentions``: True, or a subset of ("encoder", "decoder", "cross") - the encoder's weights are about 99 % of
        the bytes, and token-to-frame alignment needs only "cross".  Adds, per kind asked for, a tuple with one tensor per
        layer (W:345-371, W:420-466): ``encoder_attentions`` [B, He, T, T], ``decoder_attentions`` [B, Hd, S, S] (under the
        inverted mask of W:416-418: row i holds exact zeros at keys j <= i, the last row is uniform), ``cross_attentions``
        [B, Hd, S, T]; the probabilities before dropout, in ``attentions_dtype`` (None: the compute dtype; torch.float32 is
        allowed on the bf16 model).  ``output_hidden_states`` adds ``encoder_hidden_states`` / ``decoder_hidden_states``: the
        input of every layer (W:348-349, W:427-428; ``encoder_layers`` / ``decoder_layers`` tensors [B, T or S, d]); the
        post-LayerNorm output stays in ``*last_hidden_state``.  Keys that were not asked for are absent."""
        cfg = self.config
        kinds = check_output_attentions(cfg, output_attentions)
        if attentions_dtype not in (None, torch.float32, torch.bfloat16):
            raise ValueError("attentions_dtype must be None, torch.float32 or torch.bfloat16")
        capture = _Capture(kinds, bool(output_hidden_states), attentions_dtype or self.dtype) if (kinds or output_hidden_states) else None
        features = self._check_features(features)
        B = features.shape[0]
        start = cfg.decoder_start_token_id
        if decoder_input_ids is not None:
            dec = torch.as_tensor(decoder_input_ids).to(device=self.device, dtype=torch.int32)
            if dec.dim() != 2 or dec.shape[0] != B or dec.shape[1] < 1:
                raise ValueError("decoder_input_ids must be [B, S]")
            if not bool((dec[:, 0] == start).all()):
                raise ValueError("decoder_input_ids must start with decoder_start_token_id")
            S = dec.shape[1]
            shifted = torch.cat([dec[:, 1:], dec[:, :1]], dim=1)  # (the last column is never read)
        elif labels is not None:
            shifted = torch.as_tensor(labels).to(device=self.device, dtype=torch.int32)
            if shifted.dim() != 2 or shifted.shape[0] != B:
                raise ValueError("labels must be [B, S]")
            S = shifted.shape[1]
        else:
            S, shifted = 1, torch.zeros(B, 1, dtype=torch.int32, device=self.device)
        if not 1 <= S <= cfg.max_target_positions:
            raise ValueError("target length exceeds max_target_positions")
        inf = self._infer_prepare(B, features.shape[2])
        with self._inference(inf):
            ws, d, T = self.ws, cfg.d_model, inf["T"]
            lab = ws["labels"][:B * S].view(B, S)
            lab.copy_(shifted)
            enc_out = self._encode_infer(features, inf, capture)
            self._cross_kv_infer(enc_out)
            h = self._decode_infer(lab, B, S, T, capture)
            out = torch.empty(B * S, d, dtype=self.dtype, device=self.device)
            self._ln_fwd(h, "decoder.layer_norm", out, "ln")
            Vp = self.arena.v_pad
            logits = torch.empty(B * S, Vp, dtype=self.dtype, device=self.device)
            self._gemm_xw(out, "lm_head.kernel", logits, B * S, Vp, d, d, ldc=Vp)  # W:579
            result = {"loss": None,
                      "logits": logits.view(B, S, Vp)[:, :, :cfg.vocab_size],
                      "last_hidden_state": out.view(B, S, d),
                      "encoder_last_hidden_state": enc_out.view(B, T, d).clone()}
            if capture is not None:
                result.update(capture.results())
        return result

    @torch.no_grad()
    def generate(self, input_features, max_length=None, min_length=None, num_beams=None, temperature=1.0, top_k=None,
                 top_p=None, repetition_penalty=None, attention_mask=None, eos_token_id=None, length_penalty=1.0,
                 early_stopping=False, num_return_sequences=1, return_dict_in_generate=False, do_sample=False, seed=0,
                 return_token_timestamps=False, no_repeat_ngram_size=None, suppress_tokens=None, begin_suppress_tokens=None,
                 prompt_ids=None, segment_timestamps=None, max_initial_timestamp=1.0, timestamp_begin=None,
                 no_timestamps_token_id=None):
        """Greedy decoding (W:636-709) -> int32 ids [B, 1 + n] on the device, the start token first.  ``num_beams`` of 2 to
        8: beam search (``_generate_beam``; the reference accepts num_beams at W:637 and leaves it as a ``pass`` at
        W:696-698); None or 1: greedy (``_generate_greedy``).  Every mode runs the one step loop of ``_decode_steps``.

        As in the reference: the encoder runs once; every step runs the WHOLE decoder over the whole prefix (under the
        inverted mask of W:416-418 appending a token changes every earlier position's state from layer 1 up, so there is
        no valid KV cache) and appends argmax(lm_head(decoder_out)[:, -1, :]) to every row; the loop stops when every
        row's token of the same step is EOS, or after ``max_length`` steps.  Temperature and top-k do not change an argmax;
        the other options are accepted and ignored (W:643-648).  Fixed against the reference: the logits come from the LM
        head (W:675 reads a key WhisperModel does not return), ``max_length`` above max_target_positions raises up front
        instead of overrunning the positional table (W:383).  ``eos_token_id`` (not in the reference's signature):
        overrides config.eos_token_id; -1 disables the stop.  ``do_sample=True``: sampled decoding (``_generate_sample``),
        the one mode in which temperature, top_k, top_p and min_length take effect.

        Per step: the embedding of [start, tokens so far] (tmi_embed_fwd), the decoder over the prefix, and
        tmi_lm_head_argmax on the B last rows (final LayerNorm, LM head and argmax in one launch).  The EOS count of a step
        is read one step late (``greedy_loop``), so the device never idles on the host's check.

        ``return_token_timestamps=True`` (every mode): the result is the dict form - {"sequences"} and what the mode's
        ``return_dict_in_generate`` adds - with the outputs of ``align`` for the returned sequences (over "lengths" where
        the mode reports them) added: one more encoder pass and one teacher-forced decoder pass per distinct length.
        Aligning token n needs position n of the decoder, so ``max_length`` is then at most max_target_positions - 1 (and
        defaults to it).  False: nothing changes.

        Decode constraints and prompts (every mode; the rule is include/tethys_mi.h's "Decode constraints", applied to the
        logits BEFORE the temperature; ``check_constraint_args`` states the bounds).  ``repetition_penalty`` p (None or 1:
        off): the logit of every token already in the row - start token, prompt and generated tokens alike - is divided
        by p when positive and multiplied by p otherwise.  ``no_repeat_ngram_size`` n (None or 0: off): a token that would
        complete an n-gram the row already holds cannot be emitted.  ``suppress_tokens``: ids that can never be emitted;
        ``begin_suppress_tokens``: ids that cannot be the first generated token.  ``prompt_ids`` int [P] or [B, P], P >= 1:
        these tokens follow the start token (in beam search every beam of an item starts from them).  The result is then
        ids [B, 1 + P + n]; "lengths" counts prompt plus generated tokens (sequences[b, 1 : 1 + lengths[b]] stays the row's
        tokens), while "token_logprobs" [B, n], "sequences_scores", the beam length penalty, ``max_length`` and
        ``min_length`` count generated tokens only, with P + max_length <= max_target_positions.  Per step there is one
        tmi_decode_constraints launch on the step's prefixes (so beams may reorder freely) and the _c form of the mode's
        LM head.  With every one of these at its default the call takes the path it took without them: the same kernels
        and launches, no other buffer.

        ``segment_timestamps=True`` (every mode; None or False: nothing changes, the same kernels, launches and bits):
        the row is decoded under Whisper's timestamp grammar ``<|t0|> text <|t1|><|t1|> text <|t2|> ..`` - include/
        tethys_mi.h's "Timestamp rules" a - g, acting on the logits before the temperature.  The timestamp ids are
        [``timestamp_begin``, vocab_size) (None: vocab_size - 1501), id timestamp_begin + u standing for u * 0.02 s;
        ``no_timestamps_token_id`` (None: timestamp_begin - 1; -1: none) is never emitted; the first timestamp is at most
        ``max_initial_timestamp`` seconds (None: no cap) and no timestamp is past the features' encoder frame count
        (at most 1500).  Per step two more launches follow tmi_decode_constraints - tmi_timestamp_rules and
        tmi_lm_head_timestamp_gate, which streams the LM head once more - and the mode's _c head runs on the resulting
        set.  The result is then the dict form with "segments": per returned row the list ``parse_timestamp_segments``
        gives for its generated tokens (times in units of 0.02 s), and "advance" [rows] (units).  ``min_length`` must be
        unset; ``check_timestamp_rule_args`` states the bounds.  Independent of ``return_token_timestamps``."""
        cfg = self.config
        ts = check_timestamp_rule_args(cfg, segment_timestamps, max_initial_timestamp, timestamp_begin, no_timestamps_token_id,
                                       suppress_tokens=suppress_tokens, min_length=min_length, eos_token_id=eos_token_id)
        cons = check_constraint_args(cfg, max_length, num_beams, repetition_penalty=repetition_penalty,
                                     no_repeat_ngram_size=no_repeat_ngram_size, suppress_tokens=suppress_tokens,
                                     begin_suppress_tokens=begin_suppress_tokens, prompt_ids=prompt_ids,
                                     eos_token_id=eos_token_id, return_token_timestamps=return_token_timestamps)
        if ts is not None and cons is None:  # (the grammar alone: an active constraint with nothing else in it)
            cons = {"penalty": 1.0, "ngram": 0, "suppress": [], "begin": [], "prompt": None, "P": 0, "active": True,
                    "max_length": check_timestamp_length(cfg, max_length) if return_token_timestamps else
                    check_generate_args(cfg, max_length, None, 1.0)}
        if cons is not None:
            max_length = cons["max_length"]
        ts_args = dict(segment_timestamps=segment_timestamps, max_initial_timestamp=max_initial_timestamp,
                       timestamp_begin=timestamp_begin, no_timestamps_token_id=no_timestamps_token_id)
        if return_token_timestamps:
            max_length = check_timestamp_length(cfg, max_length)
            out = self.generate(input_features, max_length=max_length, min_length=min_length, num_beams=num_beams,
                                temperature=temperature, top_k=top_k, top_p=top_p, repetition_penalty=repetition_penalty,
                                attention_mask=attention_mask, eos_token_id=eos_token_id, length_penalty=length_penalty,
                                early_stopping=early_stopping, num_return_sequences=num_return_sequences,
                                return_dict_in_generate=True, do_sample=do_sample, seed=seed,
                                no_repeat_ngram_size=no_repeat_ngram_size, suppress_tokens=suppress_tokens,
                                begin_suppress_tokens=begin_suppress_tokens, prompt_ids=prompt_ids, **ts_args)
            if not isinstance(out, dict):  # (the greedy path has no dict form of its own)
                out = {"sequences": out}
            out.update(self.align(input_features, out["sequences"], out.get("lengths")))
            return out
        beam = not do_sample and num_beams is not None and int(num_beams) > 1
        if do_sample:
            max_length, top_k, top_p, min_length = sample_args(cfg, max_length, num_beams, temperature, top_k, top_p, min_length)
        elif beam:  # (ahead of check_generate_args: it still raises for num_beams > 1)
            max_length = check_beam_args(cfg, max_length, num_beams, temperature, length_penalty, num_return_sequences)
        else:
            max_length = check_generate_args(cfg, max_length, num_beams, temperature)
        eos = cfg.eos_token_id if eos_token_id is None else int(eos_token_id)
        features = self._check_features(input_features)
        if ts is not None:
            ts = dict(ts, eos=eos, max_ts=min(TIMESTAMP_MAX_UNITS, self._stem_geometry(features.shape[2])["T"]))
            cons = dict(cons, active=True, ts=ts)
            return_dict_in_generate = True
        if do_sample:
            out = self._generate_sample(features, max_length, float(temperature), top_k, top_p, min_length, eos, int(seed),
                                        bool(return_dict_in_generate), cons)
        elif beam:
            out = self._generate_beam(features, max_length, int(num_beams), float(temperature), eos, float(length_penalty),
                                      bool(early_stopping), int(num_return_sequences), bool(return_dict_in_generate), cons)
        else:
            out = self._generate_greedy(features, max_length, eos, cons)
        if ts is None:
            return out
        if not isinstance(out, dict):  # (the greedy path has no dict form of its own)
            out = {"sequences": out}
        seq, P = out["sequences"].cpu().numpy(), cons["P"]
        lens = out["lengths"].cpu().numpy() if "lengths" in out else np.full(seq.shape[0], seq.shape[1] - 1)
        parsed = [parse_timestamp_segments(seq[r, 1 + P:1 + int(lens[r])], ts["tb"], ts["max_ts"], eos)
                  for r in range(seq.shape[0])]
        out["segments"], out["advance"] = [p[0] for p in parsed], [p[1] for p in parsed]
        return out

    def _constraint_state(self, cons, rows: int, K: int = 1):
        """The device side of ``cons`` (check_constraint_args; None: nothing, -> (0, None, None)) for ``rows`` decoded rows, K
        rows per batch item: the prompt's length P, the prompt as int32 [rows, P] (or None), and ``apply(prefix, ld, t,
        first, shared, ln)`` -> the keyword arguments of the step's _c LM head, after one tmi_decode_constraints launch on the
        rows' prefixes of length t (``first``: the first generated step, where begin_suppress_tokens are banned too).
        ``shared`` and ``ln`` are the step's hidden-state arguments (``_decode_steps``: what every head takes); they are
        read only under the timestamp grammar (``cons["ts"]``, generate's ``segment_timestamps``), whose two launches -
        tmi_timestamp_rules and tmi_lm_head_timestamp_gate - then follow on the banned set.  Without an active constraint
        (a prompt alone) ``apply`` is None and the mode keeps its unconstrained LM head."""
        if cons is None:
            return 0, None, None
        dev, V = self.device, self.config.vocab_size
        prompt = None
        if cons["P"]:
            pr = torch.from_numpy(cons["prompt"]).to(dev)
            if pr.dim() == 1:
                pr = pr[None, :].expand(rows // K, -1)
            elif pr.shape[0] != rows // K:
                raise ValueError(f"prompt_ids has {pr.shape[0]} rows for a batch of {rows // K}")
            prompt = pr.repeat_interleave(K, dim=0).contiguous()
        if not cons["active"]:
            return cons["P"], prompt, None
        W = ops.constraint_words(V)
        sets = torch.empty(2, rows, W, dtype=torch.int32, device=dev)
        words = lambda ids: torch.from_numpy(token_bitset(ids, V)).to(dev) if ids else None  # noqa: E731
        static, static_first = words(cons["suppress"]), words(sorted(set(cons["suppress"]) | set(cons["begin"])))
        penalty, ngram = cons["penalty"], cons["ngram"]
        ts, P = cons.get("ts"), cons["P"]
        if ts is not None:  # the timestamp grammar: the rule launch's scratch and the gate's workspace (left zero by every call)
            fired = torch.zeros(rows, dtype=torch.int32, device=dev)
            gate_ws = torch.zeros(ops.lm_head_timestamp_gate_workspace_elems(rows, V), dtype=torch.int64, device=dev)

        def apply(prefix, ld, t, first, shared=None, ln=None):
            ops.decode_constraints(prefix, ld, rows, t, V, sets[0], sets[1], ngram=ngram,
                                   static_banned=static_first if first else static)
            if ts is not None:  # rules a - f, then rule g over the step's own hidden states: ``shared`` is the head's
                ops.timestamp_rules(prefix, ld, rows, t, P, V, ts["tb"], sets[1], no_timestamps_id=ts["no_ts"],
                                    eos_id=ts["eos"], max_initial=ts["max_initial"], max_ts=ts["max_ts"])
                ops.lm_head_timestamp_gate(*shared, ts["tb"], fired, gate_ws, seen=sets[0], banned=sets[1], penalty=penalty,
                                           **ln)
            return dict(seen=sets[0], banned=sets[1], penalty=penalty)

        return cons["P"], prompt, apply

    def _decode_steps(self, features, K, P, max_length, eos, apply, prefix_of, heads, head, prepare=None, finish=None):
        """The step loop every decoding mode shares -> n, the number of generated steps to keep (``greedy_loop``).

        ``features`` [B, n_mels, T_in] as ``_check_features`` returns them; K decoder rows per item (beams; otherwise 1); P
        prompt tokens behind the start token; ``max_length`` >= 1.  The encoder and the cross-attention k|v run once on the
        B items (the k|v rows then repeated for the K rows of each item).  Generated step t = 1, 2, .. works on prefixes of
        length tp = P + t and queues
          - the relayout of ``prefix_of(t)``, the mode's int32 prefix rows [B*K, 1 + P + max_length] of that step, into the
            decoder's labels, and the decoder over the tp positions;
          - ``head(t, tp, cur, lm_head, shared, kw)``, the mode's own part.  It calls ``lm_head(*shared, <its own
            arguments>, **kw)`` once: the LM head on the B*K last positions - ``heads[0]``, or behind the step's
            tmi_decode_constraints launch on ``cur`` its _c form ``heads[1]`` when a constraint is active (``apply`` of
            ``_constraint_state``; None, also for a prompt alone: heads[0]); ``shared`` and ``kw`` are the arguments
            every head takes (the final LayerNorm's and the constraint's among them).  It queues whatever follows the
            head, and returns the step's one-element device count (rows at EOS, rows finished, items done);
          - the count's copy to pinned memory and an event.
        The count is read one step late (``greedy_loop``), so the device never idles on the host's check, and the extra
        queued step's column is dropped; ``eos`` < 0: never read.  ``prepare(inf)`` adds a mode's scratch to the inference
        set before the scope opens; ``finish(n)`` queues what follows the last step inside it.  Ends synchronized."""
        cfg = self.config
        B, dev = features.shape[0], self.device
        rows, L1 = B * K, 1 + P + max_length
        inf = self._infer_prepare(B, features.shape[2], K)
        if prepare is not None:
            prepare(inf)
        host = torch.zeros(1 + max_length, dtype=torch.int32, pin_memory=True)
        events = [torch.cuda.Event(), torch.cuda.Event()]
        with self._inference(inf):
            ws, d, T, V = self.ws, cfg.d_model, inf["T"], cfg.vocab_size
            enc_out = self._encode_infer(features, inf)
            self._cross_kv_infer(enc_out)
            if K > 1 and cfg.decoder_layers:
                _repeat_rows_per_item(ws["kvc_all"].view(rows, T, -1), B, K)
            lab_flat = ws["labels"]
            wl, ldw = self.W("lm_head.kernel")
            ln = dict(gamma=self.arena.param("decoder.layer_norm.gamma"), beta=self.arena.param("decoder.layer_norm.beta"),
                      eps=cfg.layer_norm_eps)
            main = self._main or torch.cuda.current_stream(dev)
            lm_head = heads[0] if apply is None else heads[1]

            def step(t):
                tp, cur = P + t, prefix_of(t)
                lab = lab_flat[:rows * tp].view(rows, tp)
                if tp > 1:
                    lab[:, :tp - 1].copy_(cur[:, 1:tp])  # (index relayout only: the embedding shift reads rows of stride tp)
                h = self._decode_infer(lab, rows, tp, T)
                shared = (h[tp - 1:], tp * d, wl, ldw, rows, d, V)
                kw = ln if apply is None else dict(ln, **apply(cur, L1, tp, t == 1, shared, ln))
                count = head(t, tp, cur, lm_head, shared, kw)
                host[t:t + 1].copy_(count, non_blocking=True)
                events[t & 1].record(main)

            def read_count(t):
                events[t & 1].synchronize()
                return int(host[t])

            n = greedy_loop(max_length, B, step, read_count if eos >= 0 else None)
            if finish is not None:
                finish(n)
        torch.cuda.current_stream(dev).synchronize()
        return n

    def _generate_greedy(self, features, max_length, eos, cons):
        """Greedy decoding (``generate``'s docstring) -> ids [B, 1 + P + n]: tmi_lm_head_argmax as the choice, the count of
        rows at EOS as the stop.  Generated step t (1-based) reads the prefix columns [0, P + t) and writes column P + t.
        ``cons`` (check_constraint_args; None: none): a prompt of P tokens behind the start token and / or decode
        constraints - one tmi_decode_constraints launch per step and tmi_lm_head_argmax_c."""
        B, dev = features.shape[0], self.device
        P, prompt, apply = self._constraint_state(cons, B)
        L1 = 1 + P + max_length
        ids = torch.empty(B, L1, dtype=torch.int32, device=dev)
        ids[:, 0] = self.config.decoder_start_token_id
        if P:
            ids[:, 1:1 + P] = prompt
        if max_length == 0:
            return ids
        counts = torch.zeros(1 + max_length, dtype=torch.int32, device=dev)

        def head(t, tp, cur, lm_head, shared, kw):
            lm_head(*shared, ids[:, tp:], L1, self.ws["argmax_ws"], eos_id=eos, eos_count=counts[t:], **kw)
            return counts[t:t + 1]

        n = self._decode_steps(features, 1, P, max_length, eos, apply, lambda t: ids,
                               (ops.lm_head_argmax, ops.lm_head_argmax_c), head)
        return ids[:, :1 + P + n].clone()

    def _generate_sample(self, features, max_length, temperature, top_k, top_p, min_length, eos, seed, return_dict,
                         cons=None):
        """Sampled decoding: the greedy loop with tmi_lm_head_sample as the choice rule (include/tethys_mi.h states it:
        top_k >= 1 keeps the top_k largest scores and their top_p nucleus and draws by inverse CDF, top_k == 0 draws from
        the whole vocabulary by Gumbel-max).  Step t (1-based) draws with the seed (seed + t * 0x9E3779B97F4A7C15) mod
        2^64, row b with row key b, so a seeded call repeats; EOS is suppressed while t <= min_length.  A row that draws
        EOS is finished: its later columns are pad_token_id (which it also feeds its own decoder; the rows of a batch do
        not see each other) and their log-probabilities 0.  The loop stops once every row is finished (the count is read
        one step late) or after max_length steps.  -> ids [B, 1 + n], or with ``return_dict`` {"sequences",
        "token_logprobs" [B, n] (log-softmax of logits / temperature at the token: the uncut distribution),
        "sequences_scores" [B] (their sum up to and including the row's EOS), "lengths" [B] (tokens up to and including
        EOS)}.  ``cons`` (check_constraint_args; None: none): a prompt of P tokens behind the start token and / or decode
        constraints - step t then reads the prefix columns [0, P + t) and writes column P + t, ids are [B, 1 + P + n],
        "lengths" counts the prompt too, everything else above (the step seeds, min_length, the log-probabilities) still
        counts generated tokens."""
        cfg = self.config
        B, dev = features.shape[0], self.device
        P, prompt, apply = self._constraint_state(cons, B)
        L1 = 1 + P + max_length
        ids = torch.empty(B, L1, dtype=torch.int32, device=dev)
        ids[:, 0] = cfg.decoder_start_token_id
        if P:
            ids[:, 1:1 + P] = prompt
        lps = torch.zeros(1 + max_length, B, device=dev)  # (a step's log-probabilities are one contiguous row)
        n = 0
        if max_length > 0:
            finished = torch.zeros(B, dtype=torch.int32, device=dev)
            counts = torch.zeros(1 + max_length, dtype=torch.int32, device=dev)

            def head(t, tp, cur, lm_head, shared, kw):
                lm_head(*shared, ids[:, tp:], L1, finished, counts[t:], self.ws["sample_ws"], temperature=temperature,
                        top_k=top_k, top_p=top_p, seed=sample_step_seed(seed, t), suppress_id=eos if t <= min_length else -1,
                        eos_id=eos, pad_id=cfg.pad_token_id, logprob=lps[t], **kw)
                return counts[t:t + 1]

            n = self._decode_steps(features, 1, P, max_length, eos, apply, lambda t: ids,
                                   (ops.lm_head_sample, ops.lm_head_sample_c), head,
                                   prepare=lambda inf: self._sample_workspace(inf, B, top_k))
        seq = ids[:, :1 + P + n].clone()
        if not return_dict:
            return seq
        tok_lp = lps[1:1 + n].t().contiguous()
        is_eos = (seq[:, 1 + P:] == eos) if eos >= 0 else torch.zeros(B, n, dtype=torch.bool, device=dev)
        first = torch.where(is_eos.any(dim=1), is_eos.int().argmax(dim=1) + 1, n) if n else torch.zeros(B, dtype=torch.int64, device=dev)
        return {"sequences": seq, "token_logprobs": tok_lp, "sequences_scores": tok_lp.sum(dim=1),
                "lengths": (first + P).to(torch.int32)}

    def _generate_beam(self, features, max_length, K, temperature, eos, length_penalty, early_stopping, R, return_dict,
                       cons=None):
        """Beam search; the rule is the module docstring's "Beam search".  The encoder and the cross-attention k|v run once
        on the B items, the k|v rows are then repeated for the K beams of each item; every step runs the decoder over the
        B*K prefixes, tmi_lm_head_topk (N = 2K candidates per row: final LayerNorm, LM head, log-softmax and top-N in one
        launch) and tmi_beam_step (one workgroup per item: the walk, the pool, the next prefixes in a second buffer, the
        done flags and count).  The done count is read one step late (``greedy_loop``); the only other host work is
        queueing.  Finalize (the live beams of the items not done, offered to the pools) is a mode of tmi_beam_step.
        ``cons`` (check_constraint_args; None: none): every beam starts from [start, prompt] (P tokens), step t works on
        prefixes of length P + t, the scores and the length penalty t ** length_penalty count generated tokens, the
        lengths count the prompt too; with an active constraint the candidates come from tmi_lm_head_topk_c on the sets
        tmi_decode_constraints builds from the step's own prefix rows."""
        cfg = self.config
        B, dev = features.shape[0], self.device
        BK, N = B * K, 2 * K
        P, prompt, apply = self._constraint_state(cons, BK, K)
        L1 = 1 + P + max_length
        start, pad = cfg.decoder_start_token_id, cfg.pad_token_id
        if max_length == 0:
            seq = torch.full((B * R, 1 + P), start, dtype=torch.int32, device=dev)
            if P:
                seq[:, 1:] = prompt.view(B, K, P)[:, :R].reshape(B * R, P)
            zeros = torch.zeros(B * R, device=dev)
            if return_dict:
                return {"sequences": seq, "sequences_scores": zeros, "lengths": torch.full((B * R,), P, dtype=torch.int32, device=dev)}
            return seq
        i32 = dict(dtype=torch.int32, device=dev)
        prefix = torch.full((2, BK, L1), start, **i32)  # double-buffered prefixes; every entry a valid token id
        if P:
            prefix[:, :, 1:1 + P] = prompt
        sums = torch.zeros(B, K, device=dev)
        sums[:, 1:] = float("-inf")
        sums = sums.view(BK)
        pool_ids = torch.full((B, K, L1), pad, **i32)
        pool_scores = torch.zeros(B, K, device=dev)
        pool_len = torch.zeros(B, K, **i32)
        pool_cnt, done, n_done = torch.zeros(B, **i32), torch.zeros(B, **i32), torch.zeros(1, **i32)
        cand_ids, cand_lp = torch.empty(BK, N, **i32), torch.empty(BK, N, device=dev)
        len_pow = lambda n: float(np.float32(float(n) ** length_penalty))  # noqa: E731
        pool = (pool_ids, pool_scores, pool_len, pool_cnt, done, n_done)

        def head(t, tp, cur, lm_head, shared, kw):
            lm_head(*shared, N, cand_ids, cand_lp, self.ws["topk_ws"], temperature=temperature, **kw)
            ops.beam_step(cand_ids, cand_lp, N, B, K, sums, cur, prefix[(t + 1) & 1], L1, tp, eos, len_pow(t), early_stopping,
                          *pool)
            return n_done

        def finalize(n):
            ops.beam_step(None, None, N, B, K, sums, prefix[(n + 1) & 1], None, L1, P + n, eos, len_pow(n), early_stopping,
                          *pool, finalize=True)

        self._decode_steps(features, K, P, max_length, eos, apply, lambda t: prefix[t & 1],
                           (ops.lm_head_topk, ops.lm_head_topk_c), head, finish=finalize)
        lengths = pool_len[:, :R].reshape(B * R)
        n_out = int(lengths.max())
        seq = pool_ids[:, :R, :1 + n_out].reshape(B * R, 1 + n_out)
        seq = torch.where(torch.arange(1 + n_out, device=dev)[None, :] > lengths[:, None], pad, seq)
        if return_dict:
            return {"sequences": seq, "sequences_scores": pool_scores[:, :R].reshape(B * R).clone(),
                    "lengths": lengths.clone()}
        return seq


    # -- evaluation (forward only): teacher-forced loss / accuracy (W:596-600, W:904-907) and sequence scoring -------------
    def _score_workspace(self, inf, M: int, ldc: int):
        """The scratch of the chunked LM head for M rows at chunk stride ``ldc``, added to the inference set ``inf`` on the
        evaluation paths only (as ``_sample_workspace``): the logits chunk [M, ldc] in the compute dtype, tmi_logprob_fold's
        state (any contents) and its three outputs, and the targets."""
        ws, dev = inf["ws"], self.device
        have = ws.get("lp_chunk")
        if have is None or have.shape[0] < M or have.shape[1] != ldc:
            ws["lp_chunk"] = torch.empty(M, ldc, dtype=self.dtype, device=dev)
        have = ws.get("lp_lse")
        if have is None or have.numel() < M:
            ws["lp_state"] = torch.empty(ops.logprob_state_elems(M), dtype=torch.int64, device=dev)
            ws["lp_lse"], ws["lp_logprob"] = torch.empty(M, device=dev), torch.empty(M, device=dev)
            ws["lp_argmax"], ws["lp_targets"] = (torch.empty(M, dtype=torch.int32, device=dev) for _ in range(2))

    def _lm_head_fold(self, xn, M: int, nc: int):
        """(lse, logprob, argmax) of the M normalised rows ``xn`` [M, d] against ws["lp_targets"]: the LM head (W:579) chunk
        by chunk with tmi_gemm into ws["lp_chunk"], each chunk folded by tmi_logprob_fold; no [M, V] buffer exists."""
        cfg, ws, d = self.config, self.ws, self.config.d_model
        Vp, chunk = self.arena.v_pad, ws["lp_chunk"]
        ldc = chunk.stride(0)
        wl, ldw = self.W("lm_head.kernel")
        lm = (xn, d, wl, ldw, 1, d) if self.precision == "bf16" else None
        sched = ops.logprob_chunks(cfg.vocab_size, Vp, nc)
        for i, (c0, n) in enumerate(sched):
            self._gemm_xw(xn, "lm_head.kernel", chunk, M, n, d, d, ldc=ldc, n_off=c0)
            ops.logprob_fold(chunk, ldc, M, cfg.vocab_size, c0, n, ws["lp_targets"], ws["lp_state"], i == 0,
                             i == len(sched) - 1, ws["lp_lse"], ws["lp_logprob"], ws["lp_argmax"], lm=lm, validate=False)
        return ws["lp_lse"][:M], ws["lp_logprob"][:M], ws["lp_argmax"][:M]

    def _chunk_cols(self, nc=None) -> int:
        nc = ops.logprob_chunk_cols() if nc is None else int(nc)
        if nc < 64 or nc % 64:
            raise ValueError("the chunk width must be a positive multiple of 64")
        return nc

    @torch.no_grad()
    def evaluate(self, features, labels, decoder_attention_mask=None, return_token_logprobs=False, chunk_cols=None):
        """Forward-only teacher-forced evaluation of one batch: the loss of ``call()`` (W:585-600) and the token accuracy
        ``train_whisper`` compiles the model with (W:904-907), with no gradient, no dropout (even after ``enable_dropout``)
        and nothing of the training state touched (the inference workspace, as ``generate``).

        features [B, n_mels, T_in] fp32, labels [B, S] int32 (2 <= S <= max_target_positions).  As in training the decoder
        reads [start, labels[:, :-1]] (W:559-563) and row (b, t), t < S - 1, is scored against labels[b, t + 1] (W:585-586)
        - the reference's double shift; row S - 1 is unused.  ``decoder_attention_mask`` [B, S] (None: all ones) gives the
        weights wgt = mask[:, :-1] (W:597):
          loss     = sum(wgt * nll) / sum(wgt)                     (W:596-600; the plain mean without a mask)
          accuracy = sum(wgt * (argmax == target)) / sum(wgt)      (argmax: the smallest column among equal logits)
        -> {"loss", "accuracy" (floats), "loss_sum", "n_correct", "n_tokens" (the three sums, fp64 on the host: add them
        over batches or shards and divide once), and with ``return_token_logprobs`` "token_logprobs" [B, S - 1] fp32 (0 where
        the weight is 0)}.  The encoder and the decoder run once over the S positions; the LM head is evaluated in chunks of
        ``chunk_cols`` columns (default tmi_logprob_chunk_cols) folded by tmi_logprob_fold, so the [B*S, vocab] logits are
        never stored.  bf16: the target logit is the fp32 recomputation tmi_linear_xent uses for the training loss.
        ``chunk_cols`` is a benchmark hook (tools/eval_bench.py sweeps it to choose the library constant): leave it at None;
        the outputs are bit-reproducible for one width, not across widths."""
        cfg = self.config
        features = self._check_features(features)
        B = features.shape[0]
        labels = torch.as_tensor(labels).to(device=self.device)
        mask = None if decoder_attention_mask is None else torch.as_tensor(decoder_attention_mask).to(device=self.device)
        if labels.dtype != torch.int32:
            raise TypeError("labels must be int32")
        wgt = None
        if mask is not None:
            check_evaluate_args(cfg, tuple(labels.shape), tuple(mask.shape))
            wgt = mask[:, :-1].to(torch.float64)
            check_evaluate_args(cfg, tuple(labels.shape), tuple(mask.shape), mask_sum=float(wgt.sum()),
                                mask_min=float(wgt.min()))
        else:
            check_evaluate_args(cfg, tuple(labels.shape), None)
        if labels.shape[0] != B:
            raise ValueError("features and labels disagree on the batch size")
        S, V, nc = labels.shape[1], cfg.vocab_size, self._chunk_cols(chunk_cols)
        lo, hi = int(labels.min()), int(labels.max())
        if lo < 0 or hi >= V:
            raise ValueError(f"labels must be in [0, {V})")
        targets = torch.full((B, S), -1, dtype=torch.int32, device=self.device)
        targets[:, :-1] = labels[:, 1:] if wgt is None else torch.where(wgt > 0, labels[:, 1:], -1)
        M = B * S
        inf = self._infer_prepare(B, features.shape[2])
        self._score_workspace(inf, M, min(nc, self.arena.v_pad))
        with self._inference(inf):
            ws, T = self.ws, inf["T"]
            lab = ws["labels"][:M].view(B, S)
            lab.copy_(labels)
            ws["lp_targets"][:M].copy_(targets.view(-1))
            enc_out = self._encode_infer(features, inf)
            self._cross_kv_infer(enc_out)
            h = self._decode_infer(lab, B, S, T)
            xn = ws["xn"][:M]
            self._ln_fwd(h, "decoder.layer_norm", xn, "ln")
            _, logprob, argmax = self._lm_head_fold(xn, M, nc)
            lp = logprob.view(B, S)[:, :-1].clone()
            hit = (argmax.view(B, S)[:, :-1] == targets[:, :-1])
        lp64, hit64 = lp.double().cpu(), hit.double().cpu()
        w64 = torch.ones(B, S - 1, dtype=torch.float64) if wgt is None else wgt.cpu()
        loss_sum, n_correct, n_tokens = float(-(w64 * lp64).sum()), float((w64 * hit64).sum()), float(w64.sum())
        out = {"loss": loss_sum / n_tokens, "accuracy": n_correct / n_tokens, "loss_sum": loss_sum, "n_correct": n_correct,
               "n_tokens": n_tokens}
        if return_token_logprobs:
            out["token_logprobs"] = lp
        return out

    @torch.no_grad()
    def evaluate_generate(self, features, labels, label_lengths=None, return_items=False, return_alignment=False,
                          **generate_kwargs):
        """The token error rate of what ``generate`` emits for one batch against ``labels``: ``generate`` in any mode
        (greedy, beam with ``num_return_sequences=R``, sampled, constrained, prompted, ``segment_timestamps``; every
        keyword but ``return_token_timestamps`` and ``return_dict_in_generate`` is passed on), then ONE tmi_edit_distance
        launch on the device tensors (include/tethys_mi.h states the rule) and one read-back of its sums.

        NOT THE TRAINING SHIFT.  The labels are compared AS GIVEN with the generated tokens: no column is shifted or
        dropped, unlike ``evaluate``'s double shift.  Which labels to pass (with or without a leading start token or
        prompt) is the caller's business.

        Hypothesis of returned row r: columns [1 + P, ..) of "sequences" (P: the prompt's length), lengths[r] - P of them
        where the mode reports "lengths", otherwise every generated column; cut before the first EOS (``eos_token_id``,
        else the config's; -1: no cut).  Reference of item b: labels[b, :label_lengths[b]] (int32 [B, S]; lengths None: S),
        cut before EOS in the same way.  Under ``segment_timestamps`` the ids [timestamp_begin, vocab_size) are dropped
        from both sides.  Row r belongs to item r // R.
        -> Python floats (fp64 sums: add them over batches or shards and divide once): "n_edits", "n_sub", "n_del",
        "n_ins", "n_ref_tokens", "n_hyp_tokens", "n_exact" (items with d == 0), "n_items" and "token_error_rate" =
        n_edits / n_ref_tokens, all over the FIRST returned sequence of every item; "n_oracle_edits" and
        "oracle_error_rate": the per-item minimum of d over its R sequences (the same as the above when R == 1).
        ``return_items`` adds the device tensors "edits" int32 [B * R, 6] = (d, sub, del, ins, n, m) per row,
        "sequences" and "lengths" (None where the mode reports none).  No text normalisation.

        ``return_alignment=True``: ONE tmi_edit_align launch takes the place of the tmi_edit_distance launch (the same
        counts) and, after one more read-back, the result gains "alignment": per item, for its FIRST returned sequence,
        a dictionary "steps": [(op, hyp_token, ref_token)] in order - op 0 match, 1 substitution, 2 deletion, 3 insertion
        (``ops.EDIT_OPS`` names them), None for the missing side -, "hyp_positions": the column of every step's
        hypothesis token in that row of "sequences" (None for a deletion) and "ref_positions": the column of its
        reference token in ``labels`` (None for an insertion).  The positions index whatever else is kept per token
        (``token_timestamps`` of a later ``generate`` call on the same row).  With ``return_items`` also the device tensors
        "steps" int32 [B * R, n_cols + S, 3] (columns relative to sequences[:, 1 + P:]) and "n_steps" int32 [B * R]."""
        cfg = self.config
        labels = torch.as_tensor(labels)
        lens_host = None
        if label_lengths is not None:
            ll = torch.as_tensor(label_lengths)
            lens_host = ll.cpu().numpy()
        P = check_evaluate_generate_args(cfg, tuple(labels.shape), labels.dtype, lens_host, generate_kwargs,
                                         return_alignment=return_alignment)
        labels = labels.to(self.device)
        B, S = labels.shape
        eos = generate_kwargs.get("eos_token_id")
        eos = cfg.eos_token_id if eos is None else int(eos)
        ref_len = None if label_lengths is None else torch.as_tensor(label_lengths).to(device=self.device, dtype=torch.int32).contiguous()
        out = self.generate(features, return_dict_in_generate=True, **generate_kwargs)
        if not isinstance(out, dict):  # (the greedy path has no dict form of its own)
            out = {"sequences": out}
        seq, lengths = out["sequences"], out.get("lengths")
        if seq.shape[0] % B:
            raise ValueError("features and labels disagree on the batch size")
        R = seq.shape[0] // B
        hyp_len = None if lengths is None else (lengths.to(torch.int32) - P).contiguous()
        skip = (0, 0)
        if generate_kwargs.get("segment_timestamps"):
            tb = generate_kwargs.get("timestamp_begin")
            skip = (cfg.vocab_size - TIMESTAMP_TOKENS if tb is None else int(tb), cfg.vocab_size)
        if return_alignment:
            edits, steps, n_steps = ops.edit_align(seq[:, 1 + P:], labels, hyp_len, ref_len, R=R, stop_id=eos, skip=skip)
        else:
            edits = ops.edit_distance(seq[:, 1 + P:], labels, hyp_len, ref_len, R=R, stop_id=eos, skip=skip)
        res = ops.edit_counts(edits, R)
        check_evaluate_generate_args(cfg, (B, S), labels.dtype, lens_host, generate_kwargs, n_ref_tokens=res["n_ref_tokens"])
        if return_alignment:
            items = ops.edit_alignment_items(steps, n_steps, seq[:, 1 + P:], labels, R)
            res["alignment"] = [{"steps": [(op, h, r) for op, h, r, _, _ in it],
                                 "hyp_positions": [None if hc is None else hc + 1 + P for _, _, _, hc, _ in it],
                                 "ref_positions": [rc for _, _, _, _, rc in it]} for it in items]
        if return_items:
            res.update(edits=edits, sequences=seq, lengths=lengths)
            if return_alignment:
                res.update(steps=steps, n_steps=n_steps)
        return res

    @torch.no_grad()
    def score(self, features, sequences, lengths=None, chunk_cols=None):
        """Log-probability of given token sequences under the model, as ``generate`` would have scored them.

        NOT THE TRAINING SHIFT.  This is the plain next-token log-probability: position j predicts sequences[:, j + 1],
        token t (1-based) is scored by the decoder run over the prefix sequences[:, :t], exactly the state ``generate`` had
        when it chose that token (under the inverted mask of W:416-418 a position's state depends on the later positions,
        so every prefix is its own decoder run, as in ``generate``).  ``evaluate`` follows the reference's training loss
        instead, which shifts twice (decoder input [start, labels[:, :-1]] AND target labels[:, t + 1]).  The two methods
        share the kernel, not the shift.

        sequences [N, 1 + n] int32, the start token first, as ``generate`` returns them; ``lengths`` [N] (None: n
        everywhere): row i is scored on its first lengths[i] tokens, whatever follows (pad_token_id) is ignored.
        features [N, n_mels, T_in], or [B, n_mels, T_in] with N = B * R: row i belongs to item i // R (the layout of
        ``generate(num_return_sequences=R)``; the encoder then runs once per item).
        -> {"token_logprobs" [N, n] fp32 (log_softmax of the logits at the token, temperature 1; 0 beyond lengths[i]),
        "sequences_logprob" [N] fp32 (their sum over the first lengths[i] tokens)}.  ``chunk_cols``: the benchmark hook of
        ``evaluate``; leave it at None."""
        cfg = self.config
        features = self._check_features(features)
        B, dev, V = features.shape[0], self.device, cfg.vocab_size
        seq = torch.as_tensor(sequences).to(device=dev)
        if seq.dtype != torch.int32 or seq.dim() != 2 or seq.shape[1] < 2 or seq.shape[0] < 1 or seq.shape[0] % B:
            raise ValueError("sequences must be int32 [N, 1 + n], n >= 1, N a multiple of the feature batch")
        N, n = seq.shape[0], seq.shape[1] - 1
        R = N // B
        if n > cfg.max_target_positions:
            raise ValueError("sequence length exceeds max_target_positions")
        if not bool((seq[:, 0] == cfg.decoder_start_token_id).all()):
            raise ValueError("sequences must start with decoder_start_token_id")
        lens = torch.full((N,), n, dtype=torch.int64, device=dev) if lengths is None else torch.as_tensor(lengths).to(dev).long()
        if lens.shape != (N,) or int(lens.min()) < 0 or int(lens.max()) > n:
            raise ValueError("lengths must be [N] with entries in [0, n]")
        n_eff, nc = int(lens.max()), self._chunk_cols(chunk_cols)
        tok_lp = torch.zeros(N, n, device=dev)
        if n_eff == 0:
            return {"token_logprobs": tok_lp, "sequences_logprob": torch.zeros(N, device=dev)}
        steps = torch.arange(1, n_eff + 1, device=dev)
        scored = steps[None, :] <= lens[:, None]                                  # [N, n_eff]
        toks = seq[:, 1:1 + n_eff]
        if int(toks[scored].min()) < 0 or int(toks[scored].max()) >= V:
            raise ValueError(f"scored tokens must be in [0, {V})")
        feed = torch.where(scored, toks, cfg.pad_token_id).to(torch.int32)         # what the decoder reads: valid ids only
        targets = torch.where(scored, toks, -1).to(torch.int32).t().contiguous()  # step-major [n_eff, N]
        M, d = n_eff * N, cfg.d_model
        inf = self._infer_prepare(B, features.shape[2], R)
        self._score_workspace(inf, M, min(nc, self.arena.v_pad))
        have = inf["ws"].get("score_h")
        if have is None or have.numel() < M * d:
            inf["ws"]["score_h"] = torch.empty(M * d, dtype=self.dtype, device=dev)
        with self._inference(inf):
            ws, T = self.ws, inf["T"]
            enc_out = self._encode_infer(features, inf)
            self._cross_kv_infer(enc_out)
            if cfg.decoder_layers and R > 1:  # (as beam search)
                _repeat_rows_per_item(ws["kvc_all"].view(N, T, -1), B, R)
            ws["lp_targets"][:M].copy_(targets.view(-1))
            lab_flat, hs = ws["labels"], ws["score_h"][:M * d].view(n_eff, N, d)
            for t in range(1, n_eff + 1):
                lab = lab_flat[:N * t].view(N, t)
                if t > 1:
                    lab[:, :t - 1].copy_(feed[:, :t - 1])
                h = self._decode_infer(lab, N, t, T)
                hs[t - 1].copy_(h.view(N, t, d)[:, t - 1])  # the prefix's last position: the row generate's LM head reads
            xn = ws["xn"][:M]
            self._ln_fwd(hs.view(M, d), "decoder.layer_norm", xn, "ln")
            _, logprob, _ = self._lm_head_fold(xn, M, nc)
            tok_lp[:, :n_eff] = logprob.view(n_eff, N).t()
        return {"token_logprobs": tok_lp, "sequences_logprob": tok_lp.sum(dim=1)}

    # -- token timestamps: DTW over the cross-attention weights -------------------------------------------------------
    @torch.no_grad()
    def align(self, features, sequences, lengths=None, num_frames=None, alignment_heads=None, medfilt_width=7,
              normalize=True, return_path=False):
        """When each token of given sequences was spoken: dynamic time warping over the cross-attention weights.

        ``features``, ``sequences`` [N, 1 + n] int32 (the start token first) and ``lengths`` [N] are what ``score`` takes,
        the N = B * R layout of ``generate(num_return_sequences=R)`` included.  ``num_frames`` [N] or [B]: the valid
        encoder frames of each clip (default: all T); the warp of a row ends at its clip's last valid frame.
        ``alignment_heads``: None - every head of the upper half of the decoder layers - or (layer, head) pairs; each
        selected head weighs 1 / their number.  ``medfilt_width``: odd, 1 to 9.

        Row i: the decoder reads sequences[i, :1 + lengths[i]] in one teacher-forced pass - the computation of generate's
        last step - the start token's row of the weights is dropped and rows 1 .. lengths[i] align tokens 1 .. lengths[i],
        so 1 + lengths[i] <= max_target_positions.  Under the inverted mask of W:416-418 a row attends to the LATER
        positions, so padding behind a shorter row would change its weights: the rows are grouped by length and every
        distinct length is one decoder pass over its rows.  The encoder and the cross-attention k|v run once.  Per pass
        and selected layer the weights (fp32, tmi_attn_probs on the bf16 model) are folded into the cost at once by
        tmi_align_cost (normalise over the tokens, median filter along the frames, minus the weighted mean of the heads:
        include/tethys_mi.h has the exact definition) and released; one tmi_dtw launch then warps every row.  The
        arguments are read on the host before anything runs; nothing else is until the paths are cut (``return_path``).

        -> {"token_start_frames", "token_end_frames" [N, n] int32: the first encoder frame of token k + 1 and its last
        frame + 1, -1 beyond lengths[i]; "token_start_times", "token_end_times" [N, n] fp32 seconds = frames *
        FRAME_SECONDS (-1 beyond lengths[i]); "path_cost" [N] fp32 (0 for an empty row)}; ``return_path`` adds "paths" (a
        list of N int32 [len, 2] tensors of (token - 1, frame) pairs) and "cost" [N, max length, T] fp32 (0 where a row
        has no token or frame).  Everything stays on the device."""
        cfg = self.config
        features = self._check_features(features)
        B, dev, V = features.shape[0], self.device, cfg.vocab_size
        seq = torch.as_tensor(sequences).to(device=dev)
        if seq.dtype != torch.int32 or seq.dim() != 2:
            raise ValueError("sequences must be int32 [N, 1 + n]")
        host = lambda x: None if x is None else [int(v) for v in torch.as_tensor(x).reshape(-1).tolist()]  # noqa: E731
        a = check_align_args(cfg, tuple(seq.shape), host(lengths), host(num_frames), alignment_heads, medfilt_width)
        N, n, lens, width = a["N"], a["n"], a["lengths"], a["medfilt_width"]
        if N % B:
            raise ValueError("the number of sequences must be a multiple of the feature batch")
        R = N // B
        if not bool((seq[:, 0] == cfg.decoder_start_token_id).all()):
            raise ValueError("sequences must start with decoder_start_token_id")
        inf = self._infer_prepare(B, features.shape[2], R)
        T = inf["T"]
        nf = a["num_frames"]
        if nf is None:
            nf = [T] * N
        elif len(nf) == B and R > 1:
            nf = [v for v in nf for _ in range(R)]
        if len(nf) != N or max(nf) > T:
            raise ValueError(f"num_frames must be [N] or [B] with entries in ({width // 2}, {T}]")
        i32 = dict(dtype=torch.int32, device=dev)
        n_eff = max(lens) if lens else 0
        starts, ends = torch.full((N, n), -1, **i32), torch.full((N, n), -1, **i32)
        total = torch.zeros(N, device=dev)
        result = {"token_start_frames": starts, "token_end_frames": ends, "path_cost": total}
        order = sorted(range(N), key=lambda r: lens[r])  # (stable: rows of one length keep their order)
        cost = path = path_len = None
        if n_eff > 0:
            lens_t = torch.tensor(lens, device=dev)
            scored = torch.arange(1, n_eff + 1, device=dev)[None, :] <= lens_t[:, None]
            toks = seq[:, 1:1 + n_eff]
            if int(toks[scored].min()) < 0 or int(toks[scored].max()) >= V:
                raise ValueError(f"aligned tokens must be in [0, {V})")
            feed = torch.where(scored, toks, cfg.pad_token_id).to(torch.int32)
            order_t = torch.tensor(order, device=dev)
            rows_d = torch.tensor([lens[r] for r in order], **i32)
            cols_d = torch.tensor([nf[r] for r in order], **i32)
            weights = {l: torch.tensor(w, dtype=torch.float32, device=dev) for l, w in a["head_weights"].items()}
            cost = torch.zeros(N, n_eff, T, device=dev)  # (in the order of ``order``)
            with self._inference(inf):
                ws = self.ws
                enc_out = self._encode_infer(features, inf)
                self._cross_kv_infer(enc_out)
                if cfg.decoder_layers and R > 1:  # (as beam search)
                    _repeat_rows_per_item(ws["kvc_all"].view(N, T, -1), B, R)
                kv_all = ws["kvc_all"][:N * T]
                lo = 0
                while lo < N:
                    L = lens[order[lo]]
                    hi = lo
                    while hi < N and lens[order[hi]] == L:
                        hi += 1
                    if L > 0:
                        g, S = hi - lo, 1 + L
                        idx = order_t[lo:hi]
                        lab = ws["labels"][:g * S].view(g, S)
                        lab[:, :L].copy_(feed[idx, :L])
                        lab[:, L:].fill_(cfg.pad_token_id)  # (the shifted-out column: never read)
                        whole = g == N and order == list(range(N))
                        kvc = None if whole else kv_all.view(N, T, -1).index_select(0, idx).view(g * T, -1)
                        fold = _AlignFold(weights, rows_d[lo:hi], cols_d[lo:hi], cost[lo:hi, :L], width, bool(normalize))
                        self._decode_infer(lab, g, S, T, fold, kvc=kvc)
                    lo = hi
                st, en, tot = torch.full((N, n_eff), -1, **i32), torch.full((N, n_eff), -1, **i32), torch.zeros(N, device=dev)
                if return_path:
                    path = torch.zeros(N, n_eff + T - 1, 2, **i32)
                    path_len = torch.zeros(N, **i32)
                dtw_ws = torch.empty(ops.dtw_workspace_elems(N, n_eff, T), **i32)
                ops.dtw(cost, rows_d, cols_d, st, en, tot, dtw_ws, path, path_len)
                inv = torch.empty_like(order_t)
                inv[order_t] = torch.arange(N, device=dev)
                starts[:, :n_eff] = st.index_select(0, inv)
                ends[:, :n_eff] = en.index_select(0, inv)
                total.copy_(tot.index_select(0, inv))
        for k in ("start", "end"):
            fr = result[f"token_{k}_frames"]
            result[f"token_{k}_times"] = torch.where(fr >= 0, fr.float() * FRAME_SECONDS, -1.0)
        if return_path:
            if n_eff > 0:
                plen = path_len.index_select(0, inv).tolist()  # the one host read
                psrc = path.index_select(0, inv)
                result["paths"] = [psrc[r, :plen[r]] for r in range(N)]
                result["cost"] = cost.index_select(0, inv)
            else:
                result["paths"] = [torch.zeros(0, 2, **i32) for _ in range(N)]
                result["cost"] = torch.zeros(N, 0, T, device=dev)
        return result


ATTENTION_KINDS = ("encoder", "decoder", "cross")

# seconds per encoder frame: the log-mel hop (160 samples at 16 kHz) times the stride 2 of the stem's second convolution
FRAME_SECONDS = 160 / 16000 * 2


class _AlignFold:
    """The capture ``align`` hands to the decoder blocks: it asks for the cross-attention weights of the layers that hold a
    selected head only, folds each into the cost at once (tmi_align_cost; the first selected layer overwrites, the later
    ones accumulate: layer order) and keeps nothing."""
    dtype = torch.float32

    def __init__(self, weights, rows, cols, cost, width, normalize):
        self.weights, self.rows, self.cols, self.cost = weights, rows, cols, cost
        self.width, self.normalize = width, normalize
        self.layer, self.folded = -1, 0

    def wants(self, kind: str) -> bool:
        if kind != "cross":
            return False
        self.layer += 1  # (the decoder asks once per layer, in layer order)
        return self.layer in self.weights

    def attention(self, kind: str, probs):
        ops.align_cost(probs[:, :, 1:, :], self.rows, self.cols, self.weights[self.layer], self.cost, self.width,
                       self.normalize, accumulate=self.folded > 0)
        self.folded += 1

    def layer_input(self, side, x2d, B, T, d):
        pass


def check_timestamp_length(cfg: WhisperConfig, max_length=None) -> int:
    """``generate(return_token_timestamps=True)``'s max_length: aligning the last token needs one more decoder position
    than choosing it, so at most max_target_positions - 1 (the default)."""
    top = cfg.max_target_positions - 1
    max_length = top if max_length is None else int(max_length)
    if max_length < 0 or max_length > top:
        raise ValueError(f"with token timestamps max_length must be in [0, {top}]")
    return max_length


def check_align_args(cfg: WhisperConfig, seq_shape, lengths=None, num_frames=None, alignment_heads=None, medfilt_width=7):
    """Host validation of ``align`` (no GPU needed).  ``seq_shape`` (N, 1 + n); ``lengths`` None (n everywhere) or N
    integers in [0, n] with 1 + lengths <= max_target_positions; ``num_frames`` None or integers in
    (medfilt_width // 2, n_ctx] (``align`` checks their count and the clip's own T); ``alignment_heads`` None - every head of
    the layers >= decoder_layers // 2 - or (layer, head) pairs, no duplicates, in range; ``medfilt_width`` odd in 1..9.
    -> {"N", "n", "lengths" (list), "num_frames" (list or None), "medfilt_width", "heads" (sorted pairs), "head_weights"
    {layer: [weight of head 0, ...]} with 1 / len(heads) at the selected heads and 0 elsewhere}."""
    if len(seq_shape) != 2 or seq_shape[0] < 1 or seq_shape[1] < 1:
        raise ValueError("sequences must be [N, 1 + n] with N >= 1")
    N, n = int(seq_shape[0]), int(seq_shape[1]) - 1
    if isinstance(medfilt_width, bool) or int(medfilt_width) != medfilt_width or not 1 <= int(medfilt_width) <= 9 or int(medfilt_width) % 2 == 0:
        raise ValueError("medfilt_width must be an odd integer in 1..9")
    width = int(medfilt_width)
    lens = [n] * N if lengths is None else [int(v) for v in lengths]
    if len(lens) != N or any(v < 0 or v > n for v in lens):
        raise ValueError("lengths must be [N] with entries in [0, n]")
    if lens and 1 + max(lens) > cfg.max_target_positions:
        raise ValueError(f"aligning a token needs its decoder position: 1 + lengths must be <= {cfg.max_target_positions}")
    nf = None
    if num_frames is not None:
        nf = [int(v) for v in num_frames]
        if not nf or any(v <= width // 2 or v > cfg.n_ctx for v in nf):
            raise ValueError(f"num_frames must be in ({width // 2}, {cfg.n_ctx}]")
    Ld, Hd = cfg.decoder_layers, cfg.decoder_attention_heads
    if alignment_heads is None:
        heads = [(l, h) for l in range(Ld // 2, Ld) for h in range(Hd)]
    else:
        try:
            heads = [(int(l), int(h)) for l, h in alignment_heads]
        except (TypeError, ValueError):
            raise ValueError("alignment_heads must be None or (layer, head) pairs") from None
        if len(set(heads)) != len(heads):
            raise ValueError("alignment_heads holds a pair twice")
        for l, h in heads:
            if not (0 <= l < Ld and 0 <= h < Hd):
                raise ValueError(f"alignment_heads: ({l}, {h}) is outside {Ld} layers x {Hd} heads")
    if not heads:
        raise ValueError("no alignment head: alignment_heads is empty or the model has no decoder layer")
    if Hd > 32:
        raise ValueError("tmi_align_cost takes at most 32 heads per layer")
    heads = sorted(heads)
    weights = {}
    for l, h in heads:
        weights.setdefault(l, [0.0] * Hd)[h] = 1.0 / len(heads)
    return {"N": N, "n": n, "lengths": lens, "num_frames": nf, "medfilt_width": width, "heads": heads, "head_weights": weights}


def check_output_attentions(cfg: WhisperConfig, output_attentions) -> Tuple[str, ...]:
    """Host validation of ``forward_infer``'s ``output_attentions`` (no GPU needed): False / None -> (), True -> every
    kind, else an iterable of names out of ("encoder", "decoder", "cross") -> those, in that fixed order."""
    if output_attentions is None or output_attentions is False:
        return ()
    if output_attentions is True:
        return ATTENTION_KINDS
    if isinstance(output_attentions, (str, bytes)):
        raise ValueError('output_attentions must be True, False or a subset of ("encoder", "decoder", "cross"), e.g. ("cross",)')
    try:
        asked = list(output_attentions)
    except TypeError:
        raise ValueError('output_attentions must be True, False or a subset of ("encoder", "decoder", "cross")') from None
    for n in asked:
        if n not in ATTENTION_KINDS:
            raise ValueError(f'output_attentions: unknown kind {n!r}; choose from ("encoder", "decoder", "cross")')
    return tuple(k for k in ATTENTION_KINDS if k in asked)


class _Capture:
    """What an inference call collects on its way through the layers: the attention weights of the kinds asked for and,
    when asked for, the input of every layer.  The layer blocks take one as an optional argument; training passes none."""

    def __init__(self, kinds, hidden: bool, dtype):
        self.kinds, self.dtype = tuple(kinds), dtype
        self.att = {k: [] for k in self.kinds}
        self.hidden = {"encoder": [], "decoder": []} if hidden else None

    def wants(self, kind: str) -> bool:
        return kind in self.att

    def attention(self, kind: str, probs):
        self.att[kind].append(probs)

    def layer_input(self, side: str, x2d, B: int, T: int, d: int):
        if self.hidden is not None:
            self.hidden[side].append(x2d[:B * T].view(B, T, d).clone())

    def results(self) -> dict:
        out = {f"{k}_attentions": tuple(v) for k, v in self.att.items()}
        if self.hidden is not None:
            out.update({f"{k}_hidden_states": tuple(v) for k, v in self.hidden.items()})
        return out


def check_evaluate_args(cfg: WhisperConfig, labels_shape, mask_shape=None, mask_sum=None, mask_min=None):
    """The arguments of ``evaluate`` -> (B, S): labels [B, S] with B >= 1 and 2 <= S <= max_target_positions (S = 1 leaves
    no scored row), a decoder_attention_mask of the same shape or None.  ``mask_sum`` / ``mask_min``: the sum and the
    smallest entry of the weights mask[:, :-1] where the caller has them - the reference divides by that sum (W:598), so it
    must be > 0, and a negative weight has no meaning."""
    if len(labels_shape) != 2:
        raise ValueError("labels must be [B, S]")
    B, S = int(labels_shape[0]), int(labels_shape[1])
    if B < 1:
        raise ValueError("empty batch")
    if not 2 <= S <= cfg.max_target_positions:
        raise ValueError(f"the target length must be in [2, {cfg.max_target_positions}]")
    if mask_shape is not None and tuple(int(x) for x in mask_shape) != (B, S):
        raise ValueError("decoder_attention_mask must have the shape of labels")
    if mask_min is not None and not float(mask_min) >= 0.0:
        raise ValueError("decoder_attention_mask must not be negative")
    if mask_sum is not None and not (float(mask_sum) > 0.0 and math.isfinite(float(mask_sum))):
        raise ValueError("decoder_attention_mask[:, :-1] must have a positive, finite sum (W:598 divides by it)")
    return B, S


def check_evaluate_generate_args(cfg: WhisperConfig, labels_shape, labels_dtype, label_lengths=None, generate_kwargs=None,
                                 n_ref_tokens=None, return_alignment=False) -> int:
    """The arguments of ``evaluate_generate``, checked on the host -> P, the prompt's length (0 without ``prompt_ids``).
    labels int32 [B, S] with B >= 1 and 1 <= S <= 4096 (tmi_edit_distance's columns); ``label_lengths`` (a host array or
    None) [B] integers in [0, S]; ``generate_kwargs`` without ``return_token_timestamps`` (the alignment pass has nothing
    to compare) and without ``return_dict_in_generate`` (the method sets it).  ``n_ref_tokens``: the number of reference
    tokens where the caller has it - the error rate divides by it, so it must be >= 1.  ``return_alignment``: a bool (a
    path or a count passed by mistake is refused, not taken for True)."""
    if not isinstance(return_alignment, (bool, np.bool_)):
        raise TypeError("return_alignment must be a bool")
    if len(labels_shape) != 2:
        raise ValueError("labels must be [B, S]")
    B, S = int(labels_shape[0]), int(labels_shape[1])
    if labels_dtype != torch.int32:
        raise TypeError("labels must be int32")
    if B < 1:
        raise ValueError("empty batch")
    if not 1 <= S <= ops.EDIT_MAX_COLS:
        raise ValueError(f"the label length must be in [1, {ops.EDIT_MAX_COLS}]")
    if label_lengths is not None:
        ll = np.asarray(label_lengths)
        if ll.shape != (B,) or ll.dtype.kind not in "iu":
            raise ValueError("label_lengths must be [B] integers")
        if int(ll.min()) < 0 or int(ll.max()) > S:
            raise ValueError(f"label_lengths must be in [0, {S}]")
        if int(ll.sum()) < 1:
            raise ValueError("the labels hold no reference token: the error rate has nothing to divide by")
    kw = generate_kwargs or {}
    if kw.get("return_token_timestamps"):
        raise ValueError("evaluate_generate does not take return_token_timestamps")
    if "return_dict_in_generate" in kw:
        raise ValueError("evaluate_generate sets return_dict_in_generate itself")
    if n_ref_tokens is not None and not float(n_ref_tokens) >= 1.0:
        raise ValueError("the labels hold no reference token: the error rate has nothing to divide by")
    prompt = kw.get("prompt_ids")
    if prompt is None:
        return 0
    shape = tuple(prompt.shape) if hasattr(prompt, "shape") else np.asarray(prompt).shape
    if len(shape) not in (1, 2) or shape[-1] < 1:
        raise ValueError("prompt_ids must be [P] or [B, P], P >= 1")
    return int(shape[-1])


def word_error_rate(hyp_texts, ref_texts, device="cuda:0", return_alignment=False):
    """Word-level error counts of hypothesis strings against reference strings, by the kernel of ``evaluate_generate``:
    every text is split on whitespace (no other normalisation: case and punctuation count), the words of both lists are
    numbered through one dictionary, the rows are padded and ONE tmi_edit_distance call compares pair i.  -> the
    dictionary of ``evaluate_generate`` (R == 1), "token_error_rate" being the word error rate.  ``return_alignment=True``:
    the call is tmi_edit_align instead and the result gains "alignment": per pair the list of (op, hyp_word, ref_word) in
    order, op as in ``ops.EDIT_OPS``, None for the missing side."""
    if not isinstance(return_alignment, (bool, np.bool_)):
        raise TypeError("return_alignment must be a bool")
    hyp_texts, ref_texts = list(hyp_texts), list(ref_texts)
    if len(hyp_texts) != len(ref_texts) or not hyp_texts:
        raise ValueError("word_error_rate takes as many hypotheses as references, at least one")
    ids: Dict[str, int] = {}
    rows = [[[ids.setdefault(w, len(ids)) for w in str(t).split()] for t in texts] for texts in (hyp_texts, ref_texts)]
    if sum(len(r) for r in rows[1]) < 1:
        raise ValueError("the references hold no word: the error rate has nothing to divide by")
    dev_rows = []
    for side in rows:
        width = max(1, max(len(r) for r in side))
        if width > ops.EDIT_MAX_COLS:
            raise ValueError(f"a text has more than {ops.EDIT_MAX_COLS} words")
        pad = np.full((len(side), width), -1, np.int32)
        for i, r in enumerate(side):
            pad[i, :len(r)] = r
        lens = np.asarray([len(r) for r in side], np.int32)
        dev_rows.append((torch.from_numpy(pad).to(device), torch.from_numpy(lens).to(device)))
    (h, hl), (r, rl) = dev_rows
    if not return_alignment:
        return ops.edit_counts(ops.edit_distance(h, r, hl, rl))
    edits, steps, n_steps = ops.edit_align(h, r, hl, rl)
    res = ops.edit_counts(edits)
    words = list(ids)
    res["alignment"] = [[(op, None if a is None else words[a], None if b is None else words[b]) for op, a, b, _, _ in it]
                        for it in ops.edit_alignment_items(steps, n_steps, h, r)]
    return res


def alignment_record(item: int, alignment) -> str:
    """One JSON line for one item's "alignment" of ``evaluate_generate(return_alignment=True)``: {"item", "n_steps",
    "n_errors", "steps": [[op name, hyp_token, ref_token, hyp_position, ref_position], ...]} with null for the missing
    side (``speech_jobs/whisper_eval.py --alignments`` writes these)."""
    steps = [[ops.EDIT_OPS[op], h, r, hp, rp] for (op, h, r), hp, rp in
             zip(alignment["steps"], alignment["hyp_positions"], alignment["ref_positions"])]
    return json.dumps({"item": int(item), "n_steps": len(steps), "n_errors": sum(1 for s in steps if s[0] != ops.EDIT_OPS[0]),
                       "steps": steps})


def prepare_loss_mask(cfg: WhisperConfig, labels_shape, mask, device) -> torch.Tensor:
    """The decoder_attention_mask of the training step as a float32 [B, S] tensor on ``device``, checked on the host only.
    A tensor already on an accelerator: shape and dtype (bool, integer or real) - its values are never read.  A host array
    or CPU tensor: ``check_evaluate_args`` on its shape and its smallest weight (a negative weight has no meaning), then
    one upload.  An all-zero mask is NOT an error here (``forward_backward`` says what it gives)."""
    if isinstance(mask, torch.Tensor) and mask.device.type != "cpu":
        check_evaluate_args(cfg, labels_shape, tuple(mask.shape))
        if not (mask.dtype == torch.bool or mask.dtype.is_floating_point or mask.dtype in _INT_DTYPES):
            raise TypeError("decoder_attention_mask must be bool, integer or real")
        return mask.to(device=device, dtype=torch.float32).contiguous()
    host = mask.numpy() if isinstance(mask, torch.Tensor) else np.asarray(mask)
    if host.dtype.kind not in "biuf":
        raise TypeError("decoder_attention_mask must be bool, integer or real")
    check_evaluate_args(cfg, labels_shape, host.shape)
    w = host[:, :-1].astype(np.float64)
    check_evaluate_args(cfg, labels_shape, host.shape, mask_min=float(w.min()) if np.isfinite(w).all() else float("nan"))
    return torch.from_numpy(np.ascontiguousarray(host, dtype=np.float32)).to(device)


_INT_DTYPES = (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64)


def create_whisper_model(model_type: str = "small", device="cuda:0", precision: str = "bf16", seed: int = 1234,
                         **overrides) -> WhisperForConditionalGeneration:
    """W:852-890."""
    return WhisperForConditionalGeneration(make_config(model_type, **overrides), device=device,
                                           precision=precision, seed=seed)


# ----------------------------------------------------------------------------- greedy decoding host logic
def check_generate_args(cfg: WhisperConfig, max_length=None, num_beams=None, temperature=1.0) -> int:
    """The arguments of ``generate`` (W:636-648) -> max_length.  Raises where the reference would fail later or silently:
    ``num_beams > 1`` (W:696-698 leaves next_tokens unbound), ``max_length`` above max_target_positions (the prefix of the
    last step would outrun the positional table, W:383), a temperature <= 0 (W:678 divides by it)."""
    max_length = cfg.max_target_positions if max_length is None else int(max_length)
    if max_length < 0 or max_length > cfg.max_target_positions:
        raise ValueError(f"max_length must be in [0, {cfg.max_target_positions}]")
    if num_beams is not None and int(num_beams) > 1:
        raise ValueError("beam search is not implemented (the reference leaves it unimplemented too)")
    if temperature is not None and not float(temperature) > 0.0:
        raise ValueError("temperature must be > 0")
    return max_length


def check_beam_args(cfg: WhisperConfig, max_length=None, num_beams=2, temperature=1.0, length_penalty=1.0,
                    num_return_sequences=1) -> int:
    """The arguments of beam search -> max_length: 2 <= num_beams <= 8 (tmi_lm_head_topk keeps 2K <= 16 candidates a
    row), 1 <= num_return_sequences <= num_beams, generate's max_length and temperature bounds, and a finite
    length_penalty whose n ** length_penalty is a finite, nonzero fp32 value for every length n <= max_length (the
    scores are divided by it), so that a bad value fails here and not after the encoder has run."""
    K = int(num_beams)
    if not 2 <= K <= 8:
        raise ValueError("num_beams must be in [2, 8] for beam search (1 or None: greedy)")
    if not 1 <= int(num_return_sequences) <= K:
        raise ValueError("num_return_sequences must be in [1, num_beams]")
    max_length = check_generate_args(cfg, max_length, None, temperature)
    lp = float(length_penalty)
    if not math.isfinite(lp):
        raise ValueError("length_penalty must be finite")
    try:  # (n ** lp is monotone in n: its extremes are at n = 1, which gives 1, and at n = max_length)
        edge = float(max(1, max_length)) ** lp
    except OverflowError:
        edge = math.inf
    if not 0.0 < edge < float(np.finfo(np.float32).max) or np.float32(edge) == 0:
        raise ValueError(f"length_penalty {lp}: max_length ** length_penalty is not a finite, nonzero fp32 value")
    return max_length


CONSTRAINT_MAX_VOCAB = 65536  # tmi_decode_constraints'


def token_bitset(ids, V: int) -> np.ndarray:
    """The ids as a decode-constraint bit set over V columns: int32 words, column n at bit n & 31 of word n >> 5."""
    words = np.zeros((int(V) + 31) // 32, dtype=np.uint32)
    for v in ids:
        words[int(v) >> 5] |= np.uint32(1) << np.uint32(int(v) & 31)
    return words.view(np.int32)


def check_constraint_args(cfg: WhisperConfig, max_length=None, num_beams=None, repetition_penalty=None,
                          no_repeat_ngram_size=None, suppress_tokens=None, begin_suppress_tokens=None, prompt_ids=None,
                          eos_token_id=None, return_token_timestamps=False):
    """``generate``'s decode constraints and prompt, checked on the host before the encoder runs.  -> None when every
    one of them is at its default (penalty None or 1, n-gram size None or 0, no suppressed id, no prompt), else {"penalty",
    "ngram", "suppress", "begin" (sorted id lists), "prompt" (int32 numpy [P] or [B, P], or None), "P", "max_length",
    "active" (False for a prompt alone)}.  Raises ValueError unless: the penalty is finite and > 0; the n-gram size is in
    [0, max_target_positions]; every id is in [0, vocab_size); the prompt is [P] or [B, P] with P >= 1; P + max_length <=
    max_target_positions (one less with token timestamps; max_length None: the largest that fits); vocab_size <= 65536;
    and no row can run out of columns: vocab_size - |suppress + begin_suppress + {eos}| - (P + max_length if n-gram bans
    are on else 0) >= 2 * num_beams in beam search (tmi_lm_head_topk_c's candidates per row), >= 1 otherwise."""
    penalty = 1.0 if repetition_penalty is None else float(repetition_penalty)
    if not (math.isfinite(penalty) and penalty > 0.0):
        raise ValueError("repetition_penalty must be finite and > 0 (None or 1: off)")
    ngram = 0 if no_repeat_ngram_size is None else int(no_repeat_ngram_size)
    if isinstance(no_repeat_ngram_size, bool) or (no_repeat_ngram_size is not None and ngram != no_repeat_ngram_size):
        raise ValueError("no_repeat_ngram_size must be an integer")
    if not 0 <= ngram <= cfg.max_target_positions:
        raise ValueError(f"no_repeat_ngram_size must be in [0, {cfg.max_target_positions}] (None or 0: off)")
    V = cfg.vocab_size

    def id_list(ids, what):
        if ids is None:
            return []
        arr = np.asarray(ids.cpu() if isinstance(ids, torch.Tensor) else ids)
        if arr.size == 0:
            return []
        if arr.ndim != 1 or arr.dtype.kind not in "iu":
            raise ValueError(f"{what} must be a list of integer token ids")
        if arr.min() < 0 or arr.max() >= V:
            raise ValueError(f"{what}: every id must be in [0, {V})")
        return sorted(set(int(v) for v in arr))

    suppress, begin = id_list(suppress_tokens, "suppress_tokens"), id_list(begin_suppress_tokens, "begin_suppress_tokens")
    prompt, P = None, 0
    if prompt_ids is not None:
        prompt = np.asarray(prompt_ids.cpu() if isinstance(prompt_ids, torch.Tensor) else prompt_ids)
        if prompt.ndim not in (1, 2) or prompt.shape[-1] < 1 or prompt.dtype.kind not in "iu":
            raise ValueError("prompt_ids must be integer token ids, [P] or [B, P] with P >= 1")
        if prompt.min() < 0 or prompt.max() >= V:
            raise ValueError(f"prompt_ids: every id must be in [0, {V})")
        prompt, P = np.ascontiguousarray(prompt.astype(np.int32)), int(prompt.shape[-1])
    active = penalty != 1.0 or ngram > 0 or bool(suppress) or bool(begin)
    if not active and prompt is None:
        return None
    top = cfg.max_target_positions - (1 if return_token_timestamps else 0)
    if P > top:
        raise ValueError(f"prompt_ids: {P} tokens leave no decoder position (at most {top})")
    max_length = top - P if max_length is None else int(max_length)
    if max_length < 0 or P + max_length > top:
        raise ValueError(f"with a prompt of {P} tokens max_length must be in [0, {top - P}]")
    if active:
        if V > CONSTRAINT_MAX_VOCAB:
            raise ValueError(f"decode constraints take vocab_size <= {CONSTRAINT_MAX_VOCAB}")
        eos = cfg.eos_token_id if eos_token_id is None else int(eos_token_id)
        fixed = set(suppress) | set(begin) | ({eos} if 0 <= eos < V else set())
        free = V - len(fixed) - (P + max_length if ngram > 0 else 0)
        K = 1 if num_beams is None else int(num_beams)
        need = 2 * K if K > 1 else 1
        if free < need:
            raise ValueError(f"the constraints can leave a row with {free} columns to choose from; {need} are needed "
                             "(vocab_size minus the suppressed ids, EOS and, with n-gram bans, one id per position)")
    return {"penalty": penalty, "ngram": ngram, "suppress": suppress, "begin": begin, "prompt": prompt, "P": P,
            "max_length": max_length, "active": active}


TIMESTAMP_TOKENS = 1501      # <|0.00|> .. <|30.00|>: the top ids of Whisper's vocabulary
TIMESTAMP_MAX_UNITS = 1500   # a 30 s window in timestamp units
TIMESTAMP_UNIT_S = 0.02      # seconds per unit: one encoder frame
TIMESTAMP_UNIT_SAMPLES = 320  # samples per unit at 16 kHz
WINDOW_SAMPLES = 480000      # 30 s at 16 kHz


def check_timestamp_rule_args(cfg: WhisperConfig, segment_timestamps=None, max_initial_timestamp=1.0, timestamp_begin=None,
                              no_timestamps_token_id=None, suppress_tokens=None, min_length=None, eos_token_id=None):
    """``generate``'s timestamp grammar (include/tethys_mi.h, "Timestamp rules"), checked on the host before the encoder
    runs.  -> None when ``segment_timestamps`` is None or False (nothing else is then looked at), else {"tb", "no_ts" (-1:
    none), "max_initial" (timestamp units; -1: no cap)}.  Raises ValueError unless
      - vocab_size <= 65536 (tmi_timestamp_rules');
      - timestamp_begin (None: vocab_size - 1501, which then has to be >= 1) is in [1, vocab_size);
      - no_timestamps_token_id (None: timestamp_begin - 1) is -1 or in [0, timestamp_begin);
      - max_initial_timestamp is None or finite and >= 0 (seconds; rounded to units of 0.02 s);
      - the EOS id in force (eos_token_id, else the config's) is -1 or below timestamp_begin;
    and no row can run out of columns:
      - suppress_tokens holds no timestamp id (rules d and e leave a row the timestamps from the last one on) and, with
        the no-timestamps id, does not cover every id below timestamp_begin (rule c leaves a row exactly those);
      - min_length is None or 0 (it bans EOS, which after a closing timestamp at the window's end is all rule d leaves).
    What remains, by cases: n == 0 leaves the timestamps up to the cap (at least timestamp_begin itself); after text
    (rule f) every below column stays; after an opening timestamp or a pair (c) every below column stays; after a closing
    timestamp (d, e) that timestamp itself stays, and EOS."""
    if not segment_timestamps:
        return None
    V = cfg.vocab_size
    if V > CONSTRAINT_MAX_VOCAB:
        raise ValueError(f"segment_timestamps takes vocab_size <= {CONSTRAINT_MAX_VOCAB}")
    tb = V - TIMESTAMP_TOKENS if timestamp_begin is None else int(timestamp_begin)
    if isinstance(timestamp_begin, bool) or (timestamp_begin is not None and tb != timestamp_begin) or not 1 <= tb < V:
        raise ValueError(f"timestamp_begin must be an integer in [1, {V}) (None: vocab_size - {TIMESTAMP_TOKENS})")
    no_ts = tb - 1 if no_timestamps_token_id is None else int(no_timestamps_token_id)
    if isinstance(no_timestamps_token_id, bool) or not -1 <= no_ts < tb:
        raise ValueError(f"no_timestamps_token_id must be -1 (none) or in [0, timestamp_begin = {tb})")
    if max_initial_timestamp is None:
        max_initial = -1
    else:
        mi = float(max_initial_timestamp)
        if not (math.isfinite(mi) and mi >= 0.0):
            raise ValueError("max_initial_timestamp must be finite and >= 0 seconds (None: no cap)")
        max_initial = min(int(round(mi / TIMESTAMP_UNIT_S)), CONSTRAINT_MAX_VOCAB)
    eos = cfg.eos_token_id if eos_token_id is None else int(eos_token_id)
    if eos >= tb:
        raise ValueError(f"eos_token_id {eos} is a timestamp id (timestamp_begin = {tb})")
    if min_length is not None and int(min_length) != 0:
        raise ValueError("segment_timestamps does not take min_length: after a closing timestamp at the window's end EOS "
                         "is the one column left")
    if suppress_tokens is not None:
        sup = np.asarray(suppress_tokens.cpu() if isinstance(suppress_tokens, torch.Tensor) else suppress_tokens).reshape(-1)
        if sup.size and sup.dtype.kind in "iu":
            if int(sup.max()) >= tb:
                raise ValueError(f"suppress_tokens holds a timestamp id (>= {tb}): the grammar needs every one of them")
            if len(set(int(v) for v in sup if v >= 0) | ({no_ts} if no_ts >= 0 else set())) >= tb:
                raise ValueError("suppress_tokens covers every id below timestamp_begin: no text column is left")
    return {"tb": tb, "no_ts": no_ts, "max_initial": max_initial}


def parse_timestamp_segments(g, tb: int, window_units: int, eos_id=None):
    """The segments of one decoded window -> (segments, advance_units).  ``g``: the generated tokens of a row (behind the
    start token and the prompt), cut here before the first ``eos_id`` (None: nothing to cut); a timestamp is an id >= tb,
    id tb + u standing for u units of 0.02 s; ``window_units``: the window's length in units.
      - Two timestamps in a row close one segment and open the next: the slices of g end behind the first of each such
        pair, and at the end of g as well when g ends in a single timestamp behind text.  A slice is the segment {"start":
        first id - tb, "end": last id - tb, "tokens": its ids below tb}.  g ending in that single timestamp: the window
        is done, advance = window_units; otherwise what follows the last pair is unfinished and is decoded again by the
        next window: advance = the last slice's closing time.
      - No pair: one segment from 0 to d with every id below tb, d = the last timestamp - tb when there is one and it is
        not tb, else window_units; advance = window_units."""
    g = [int(v) for v in g]
    if eos_id is not None and eos_id in g:
        g = g[:g.index(eos_id)]
    n, is_t = len(g), lambda x: x >= tb  # noqa: E731
    single_ending = n >= 2 and not is_t(g[-2]) and is_t(g[-1])
    cons = [i + 1 for i in range(n - 1) if is_t(g[i]) and is_t(g[i + 1])]
    if cons:
        ends = cons + ([n] if single_ending else [])
        segments, lo = [], 0
        for hi in ends:
            sl = g[lo:hi]
            segments.append({"start": sl[0] - tb, "end": sl[-1] - tb, "tokens": [x for x in sl if not is_t(x)]})
            lo = hi
        return segments, (int(window_units) if single_ending else g[ends[-1] - 1] - tb)
    stamps = [x for x in g if is_t(x)]
    d = stamps[-1] - tb if stamps and stamps[-1] != tb else int(window_units)
    return [{"start": 0, "end": d, "tokens": [x for x in g if not is_t(x)]}], int(window_units)


SAMPLE_MAX_TOP_K = 64  # tmi_lm_head_sample's


def check_sample_args(cfg: WhisperConfig, max_length=None, num_beams=None, temperature=1.0, top_k=None, top_p=None,
                      min_length=None) -> int:
    """The arguments of sampled decoding (``generate(do_sample=True)``) -> max_length; the bounds are ``sample_args``'."""
    return sample_args(cfg, max_length, num_beams, temperature, top_k, top_p, min_length)[0]


def sample_args(cfg: WhisperConfig, max_length=None, num_beams=None, temperature=1.0, top_k=None, top_p=None,
                min_length=None):
    """The arguments of sampled decoding, checked -> (max_length, top_k, top_p, min_length) with the defaults filled in.
    num_beams None or 1; temperature > 0; top_k None -> 50 (W:646), 0 = no
    filter, at most 64; top_p None -> 1.0, in (0, 1], and < 1 only with a top_k filter (the nucleus is cut out of the
    top_k candidates; one over the whole vocabulary is not built); min_length None -> 0, in [0, max_length]."""
    if num_beams is not None and int(num_beams) != 1:
        raise ValueError("do_sample takes num_beams None or 1 (beam search does not sample)")
    max_length = check_generate_args(cfg, max_length, None, 1.0)
    if temperature is None or not (float(temperature) > 0.0 and math.isfinite(float(temperature))):
        raise ValueError("temperature must be > 0")
    top_k = 50 if top_k is None else int(top_k)
    if not 0 <= top_k <= SAMPLE_MAX_TOP_K:
        raise ValueError(f"top_k must be in [0, {SAMPLE_MAX_TOP_K}] (0: no filter)")
    top_p = 1.0 if top_p is None else float(top_p)
    if not 0.0 < top_p <= 1.0:
        raise ValueError("top_p must be in (0, 1]")
    if top_p < 1.0 and top_k == 0:
        raise ValueError("top_p < 1 needs a top_k filter (1..64): the nucleus is cut out of the top_k candidates")
    min_length = 0 if min_length is None else int(min_length)
    if not 0 <= min_length <= max_length:
        raise ValueError("min_length must be in [0, max_length]")
    return max_length, top_k, top_p, min_length


def sample_step_seed(seed: int, t: int) -> int:
    """The seed of decoding step t of a sampled ``generate(seed=seed)``."""
    return (int(seed) + t * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF


def greedy_loop(max_length: int, n_rows: int, step, read_eos=None, late: bool = True) -> int:
    """Host side of greedy decoding: the number n of tokens to keep (the result is ids[:, :1 + n]).

    ``step(t)`` queues decoding step t = 1 .. max_length (its token lands in column t); ``read_eos(t)`` waits for step t
    and returns how many of the ``n_rows`` rows emitted EOS there (None: no stop check).  The loop ends after the first
    step at which EVERY row's token is EOS (W:700-707: a row that emitted EOS earlier keeps decoding, only an all-EOS
    step stops), or after ``max_length`` steps.  ``late``: step t + 1 is queued before step t's count is read, so the
    device is never idle during the check; when step t stops the loop, the extra step's column is simply dropped - the
    result is the same as with ``late=False``."""
    pending = None
    for t in range(1, max_length + 1):
        if not late:
            step(t)
            if read_eos is not None and read_eos(t) == n_rows:
                return t
            continue
        step(t)
        if pending is not None and read_eos is not None and read_eos(pending) == n_rows:
            return pending
        pending = t
    if late and pending is not None and read_eos is not None and read_eos(pending) == n_rows:
        return pending
    return max_length


# ----------------------------------------------------------------------------- transcription (W:962-986)
DUMMY_AUDIO_SEED = 0


def read_wav(path: str) -> np.ndarray:
    """16-bit PCM, mono, 16 kHz ``.wav`` -> float32 samples in [-1, 1) (stdlib ``wave``; anything else raises)."""
    import wave
    with wave.open(path, "rb") as f:
        if f.getnchannels() != 1 or f.getsampwidth() != 2 or f.getframerate() != 16000:
            raise ValueError(f"{path}: expected 16-bit PCM mono at 16 kHz, got {f.getnchannels()} channel(s), "
                             f"{8 * f.getsampwidth()} bit, {f.getframerate()} Hz")
        if f.getcomptype() != "NONE":
            raise ValueError(f"{path}: compressed wav files are not supported")
        raw = f.readframes(f.getnframes())
    return (np.frombuffer(raw, dtype="<i2").astype(np.float32) / 32768.0)


def dummy_waveform(seed: int = DUMMY_AUDIO_SEED) -> np.ndarray:
    """W:971: 30 s of N(0, 1) samples at 16 kHz (seeded here; the reference draws it unseeded)."""
    return np.random.RandomState(seed).randn(16000 * 30).astype(np.float32)


def transcribe_audio(model, audio=None, tokenizer=None, max_length=448, num_beams=1, length_penalty=1.0, do_sample=False,
                     temperature=1.0, top_k=None, top_p=None, seed=0, return_timestamps=False, repetition_penalty=None,
                     no_repeat_ngram_size=None, suppress_tokens=None, begin_suppress_tokens=None, prompt_ids=None):
    """W:962-986: waveform -> log-mel (frontend.LogMelFrontend, channels-first: the layout the encoder reads; the reference
    feeds [frames, 80] un-transposed) -> ``model.generate`` -> ``tokenizer.decode(ids)``, or the ids
    (int32 numpy array, start token first) without a tokenizer.  ``audio``: a waveform (1-D tensor or array, 16 kHz), a
    ``.wav`` path, or None for the reference's 30 s dummy clip (seeded).  ``num_beams`` > 1: beam search (the best
    hypothesis), with ``length_penalty``.  ``do_sample``: sampled decoding with ``temperature``, ``top_k``, ``top_p`` and
    ``seed`` (``generate(do_sample=True)``).  ``return_timestamps=True``: -> {"text" (with a tokenizer) or "ids",
    "token_start_times", "token_end_times" (fp32 numpy arrays, seconds, one entry per token after the start token)} from
    ``model.align`` with the clip's own number of encoder frames; ``max_length`` is then capped at
    max_target_positions - 1.  ``repetition_penalty``, ``no_repeat_ngram_size``, ``suppress_tokens``,
    ``begin_suppress_tokens`` and ``prompt_ids`` ([P]) are ``generate``'s; with a prompt the returned ids hold it behind the
    start token and ``max_length`` is capped so that prompt and transcript fit the decoder's positions."""
    from .frontend import LogMelFrontend
    if audio is None:
        wav = dummy_waveform()
    elif isinstance(audio, (str, os.PathLike)):
        wav = read_wav(os.fspath(audio))
    else:
        wav = audio
    wav = torch.as_tensor(wav).to(device=model.device, dtype=torch.float32).reshape(-1).contiguous()
    fe = model.__dict__.get("_frontend")
    if fe is None:
        fe = model._frontend = LogMelFrontend(device=model.device, n_mels=model.config.n_mels)
    feats = fe(wav)
    if return_timestamps:
        max_length = min(int(max_length), model.config.max_target_positions - 1)
    cons = {k: v for k, v in (("repetition_penalty", repetition_penalty), ("no_repeat_ngram_size", no_repeat_ngram_size),
                              ("suppress_tokens", suppress_tokens), ("begin_suppress_tokens", begin_suppress_tokens),
                              ("prompt_ids", prompt_ids)) if v is not None}
    if prompt_ids is not None:
        room = model.config.max_target_positions - (1 if return_timestamps else 0) - int(np.asarray(prompt_ids).shape[-1])
        max_length = max(0, min(int(max_length), room))
    if do_sample:
        ids = model.generate(feats, max_length=max_length, num_beams=num_beams, do_sample=True, temperature=temperature,
                             top_k=top_k, top_p=top_p, seed=seed, return_dict_in_generate=bool(return_timestamps), **cons)
    elif num_beams is not None and int(num_beams) > 1:
        ids = model.generate(feats, max_length=max_length, num_beams=num_beams, length_penalty=length_penalty,
                             return_dict_in_generate=bool(return_timestamps), **cons)
    else:
        ids = model.generate(feats, max_length=max_length, **cons)
    if return_timestamps:
        out = ids if isinstance(ids, dict) else {"sequences": ids}
        seqs = out["sequences"][:1]
        n = int(out["lengths"][0]) if "lengths" in out else seqs.shape[1] - 1
        # the clip's encoder frames: its log-mel frames through the stride-2 stem ("SAME" padding: rounded up)
        frames = (fe.num_frames(wav.numel()) + 1) // 2
        al = model.align(feats, seqs, [n], num_frames=[frames])
        row = seqs[0, :1 + n].cpu().numpy()
        res = {"token_start_times": al["token_start_times"][0, :n].cpu().numpy(),
               "token_end_times": al["token_end_times"][0, :n].cpu().numpy()}
        res["text" if tokenizer is not None else "ids"] = tokenizer.decode(row) if tokenizer is not None else row
        return res
    ids = ids[0].cpu().numpy()
    if tokenizer is not None:
        return tokenizer.decode(ids)
    return ids


def transcribe_long(model, audio=None, tokenizer=None, condition_on_previous_text=True, max_initial_timestamp=1.0,
                    max_length=448, num_beams=1, length_penalty=1.0, do_sample=False, temperature=1.0, top_k=None, top_p=None,
                    seed=0, repetition_penalty=None, no_repeat_ngram_size=None, suppress_tokens=None,
                    begin_suppress_tokens=None, prompt_ids=None, timestamp_begin=None, no_timestamps_token_id=None):
    """Long-form transcription of ONE audio (``transcribe_audio``'s forms of ``audio``; any length): Whisper's own walk
    through the waveform by its timestamp tokens.  A sample position ``seek`` starts at 0; each window is wav[seek : seek +
    480000] (30 s; the last one shorter) through the front end, decoded by ``model.generate(..., segment_timestamps=True)``
    under the timestamp grammar with the window's own length in timestamp units (its encoder frames) as the largest
    timestamp; the row's generated tokens go through ``parse_timestamp_segments``, the segments are offset by the seek, and
    seek advances by advance * 320 samples: to the end of the last closed segment, or over the whole window when it closed
    nothing or ended on a single timestamp.  The walk ends when less than one front-end frame is left.
    ``condition_on_previous_text``: the text tokens of the windows so far - the last max_target_positions // 2 - 1 of
    them - follow the start token as ``prompt_ids`` (the caller's ``prompt_ids`` serve while there are none, and every
    window otherwise).  The decode arguments are ``transcribe_audio``'s; ``max_length`` is capped per window so that prompt
    and transcript fit the decoder's positions.  -> {"segments": [{"start", "end" (seconds from the start of the audio),
    "text" (with a tokenizer) or "ids"}], "ids" (every text token in order, a list), "n_windows"}."""
    from .frontend import LogMelFrontend
    if audio is None:
        wav = dummy_waveform()
    elif isinstance(audio, (str, os.PathLike)):
        wav = read_wav(os.fspath(audio))
    else:
        wav = audio
    wav = torch.as_tensor(wav).to(device=model.device, dtype=torch.float32)
    if wav.dim() != 1:
        raise ValueError("transcribe_long takes one waveform, [samples]")
    cfg = model.config
    fe = model.__dict__.get("_frontend")
    if fe is None:
        fe = model._frontend = LogMelFrontend(device=model.device, n_mels=cfg.n_mels)
    eos = cfg.eos_token_id
    tb = cfg.vocab_size - TIMESTAMP_TOKENS if timestamp_begin is None else int(timestamp_begin)
    keep = cfg.max_target_positions // 2 - 1
    mode = dict(do_sample=True, temperature=temperature, top_k=top_k, top_p=top_p, seed=seed) if do_sample else \
        dict(num_beams=num_beams, length_penalty=length_penalty) if num_beams is not None and int(num_beams) > 1 else {}
    cons = {k: v for k, v in (("repetition_penalty", repetition_penalty), ("no_repeat_ngram_size", no_repeat_ngram_size),
                              ("suppress_tokens", suppress_tokens), ("begin_suppress_tokens", begin_suppress_tokens))
            if v is not None}
    segments, text, seek, n_windows = [], [], 0, 0
    while wav.numel() - seek >= fe.n_fft:
        win = wav[seek:seek + WINDOW_SAMPLES].contiguous()
        feats = fe(win)
        units = min(TIMESTAMP_MAX_UNITS, (fe.num_frames(win.numel()) + 1) // 2)  # the window's encoder frames
        prompt = text[-keep:] if condition_on_previous_text and text and keep > 0 else prompt_ids
        P = 0 if prompt is None else int(np.asarray(prompt).shape[-1])
        out = model.generate(feats, max_length=max(0, min(int(max_length), cfg.max_target_positions - P)),
                             return_dict_in_generate=True, segment_timestamps=True,
                             max_initial_timestamp=max_initial_timestamp, timestamp_begin=timestamp_begin,
                             no_timestamps_token_id=no_timestamps_token_id,
                             **({} if prompt is None else {"prompt_ids": prompt}), **mode, **cons)
        row = out["sequences"][0].cpu().numpy()
        n = int(out["lengths"][0]) if "lengths" in out else len(row) - 1
        segs, advance = parse_timestamp_segments(row[1 + P:1 + n], tb, units, eos)
        assert advance > 0, ("the timestamp grammar gives a positive advance", row.tolist())
        t0 = seek / 16000.0
        for sg in segs:
            item = {"start": t0 + sg["start"] * TIMESTAMP_UNIT_S, "end": t0 + sg["end"] * TIMESTAMP_UNIT_S}
            item["text" if tokenizer is not None else "ids"] = tokenizer.decode(sg["tokens"]) if tokenizer is not None \
                else list(sg["tokens"])
            segments.append(item)
            text.extend(sg["tokens"])
        seek += advance * TIMESTAMP_UNIT_SAMPLES
        n_windows += 1
    return {"segments": segments, "ids": text, "n_windows": n_windows}
