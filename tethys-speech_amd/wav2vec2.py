"""Wav2Vec2 pre-training step on the HIP kernels (host orchestration).

Mirrors the reference's operator API for this path (speech_jobs/wav2vec2_dist.py, "V:"):
``Wav2Vec2Config(model_size)`` (V:24-128), ``create_full_model("pretraining", model_size)``
(V:1157-1182) and a model object whose ``forward_backward(audio, neg_indices)`` does what
``model(features, training=True)`` + the loss assembly + ``tape.gradient`` do at V:1199-1240.
Everything on the device is a C-ABI call from ``ops``; dropout rates are forced to 0 (no
parity definition with TF's RNG).  The negative indices of V:908-937 are an input of the
step (``sample_negative_indices`` draws them with the reference's recipe from a seeded
generator).

Layout notes: the q/k/v kernels of a layer are three separate contiguous [H, H] blocks (the
projection is one batched GEMM), because Keras ``clipnorm`` (V:1274) clips every reference
variable on its own; each conv layer writes its GroupNorm+GELU output straight into the
padded buffer whose overlapping rows are the next Conv1D's im2col matrix; the grouped
positional Conv1D runs as one batched window-GEMM over a group-major repack.
"""
from __future__ import annotations

import contextlib
import math
import os
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import ops
from .blocks import Arena, KernelBlocks, _round_up
from .whisper import same_pad


@dataclass
class Wav2Vec2Config:  # V:24-128 (fields read by the pre-training path)
    hidden_size: int = 768
    num_hidden_layers: int = 12
    num_attention_heads: int = 12
    intermediate_size: int = 3072
    conv_dim: Tuple[int, ...] = (512,) * 7
    conv_stride: Tuple[int, ...] = (5, 2, 2, 2, 2, 2, 2)
    conv_kernel: Tuple[int, ...] = (10, 3, 3, 3, 3, 2, 2)
    num_conv_pos_embeddings: int = 128
    num_conv_pos_embedding_groups: int = 16
    layer_norm_eps: float = 1e-5
    num_codevectors_per_group: int = 320
    num_codevector_groups: int = 2
    codevector_dim: int = 256
    proj_codevector_dim: int = 256
    contrastive_logits_temperature: float = 0.1
    num_negatives: int = 100
    diversity_loss_weight: float = 0.1
    hidden_dropout: float = 0.1       # V:69-71; applied only after enable_dropout (bf16 path), see blocks.py
    activation_dropout: float = 0.1
    attention_dropout: float = 0.1
    vocab_size: int = 32              # V:104; the CTC head's columns (Wav2Vec2ForCTC)
    ctc_blank_id: int = 0
    ctc_loss_reduction: str = "sum"   # V:94-95
    ctc_zero_infinity: bool = False
    classifier_proj_size: int = 256   # V:108-114; the classification head's projection (Wav2Vec2ForSequenceClassification)
    num_labels: int = 2               # V:1015 reads it, V:24-128 never sets it: a default of this build


# dropout site ids (KernelBlocks._site_seed; restated in oracle/dropout.py): V:296, V:779, V:560 (x2), then per
# layer V:359 (attention probabilities), V:431 (attention output), V:393 (FFN intermediate), V:396 (FFN output)
SITE_FE, SITE_FP, SITE_PH, SITE_PQ = 1, 2, 3, 4
SITE_CLS = 5  # V:1046: the classification head's Dropout between its two Dense layers (tmi_cls_head_fwd / _bwd)
SITE_CTC = 6  # V:972: the CTC model's Dropout in front of lm_head (tmi_ctc_head_fwd / _bwd)
SITE_ATTN, SITE_ATTN_OUT, SITE_FFN_MID, SITE_FFN_OUT = 100, 200, 300, 400


def make_config(model_size: str = "small", **overrides) -> Wav2Vec2Config:
    if model_size == "small":
        kw = dict(hidden_size=512, num_hidden_layers=6, num_attention_heads=8, intermediate_size=2048,
                  conv_dim=(256,) * 5, conv_stride=(5, 2, 2, 2, 2), conv_kernel=(10, 3, 3, 3, 2),
                  num_conv_pos_embeddings=64, num_conv_pos_embedding_groups=8,
                  num_codevectors_per_group=160, codevector_dim=128, proj_codevector_dim=128, classifier_proj_size=128)
    elif model_size == "tiny":
        kw = dict(hidden_size=256, num_hidden_layers=4, num_attention_heads=4, intermediate_size=1024,
                  conv_dim=(128,) * 4, conv_stride=(5, 2, 2, 2), conv_kernel=(10, 3, 3, 2),
                  num_conv_pos_embeddings=32, num_conv_pos_embedding_groups=4,
                  num_codevectors_per_group=80, codevector_dim=64, proj_codevector_dim=64, classifier_proj_size=64)
    else:
        kw = {}
    kw.update(overrides)
    return Wav2Vec2Config(**kw)


def sample_negative_indices(rng: np.random.Generator, batch_size: int, T: int, num_negatives: int = 100) -> np.ndarray:
    """V:908-937 -> [B, num_negatives] int32: the K = max(min(N, T-1), 1) positions with the
    smallest uniform-int draws (top_k of the negated draws, lowest index first on ties),
    repeated / truncated to N; the reference tiles them over every time step."""
    K = max(min(num_negatives, T - 1), 1)
    r = rng.integers(0, T, size=(batch_size, T))
    order = np.argsort(r, axis=1, kind="stable")[:, :K]
    if K < num_negatives:
        order = np.tile(order, (1, -(-num_negatives // K)))
    return order[:, :num_negatives].astype(np.int32)


def sample_negative_indices_roll(rng: np.random.Generator, T: int, num_negatives: int = 100) -> np.ndarray:
    """speech_jobs/whisper_single.py:789-839 -> [T, min(num_negatives, T)] int32: row t = roll(perm, t + 1)[:N] with
    perm a shuffle of range(T), shared by every batch row.  (TF's shuffle stream, op seed 42, is not reproducible
    outside TF: the permutation is drawn from ``rng`` and is an input of the step.)"""
    perm = rng.permutation(T).astype(np.int32)
    n = min(num_negatives, T)
    return np.stack([np.roll(perm, t + 1)[:n] for t in range(T)])


def frame_lengths(cfg: Wav2Vec2Config, sample_lengths) -> List[int]:
    """Frames each clip of ``sample_lengths`` samples occupies behind the "same"-padded conv stem: ceil(L / stride) per
    layer (V:283-288 with Keras padding="same")."""
    out = []
    for n in sample_lengths:
        n = int(n)
        if n < 0:
            raise ValueError("sample lengths must be >= 0")
        for s in cfg.conv_stride:
            n = -(-n // s)
        out.append(n)
    return out


def frame_attention_mask(cfg: Wav2Vec2Config, sample_lengths, T_in: int) -> torch.Tensor:
    """The reference's ``attention_mask`` argument for a batch of clips padded to ``T_in`` samples: float32 [B, T] over
    frames, 1 on the first ``frame_lengths`` frames of each clip and 0 behind them (host tensor)."""
    if any(int(n) > T_in for n in sample_lengths):
        raise ValueError("a clip is longer than the padded batch")
    T = frame_lengths(cfg, [T_in])[0]
    fl = torch.tensor(frame_lengths(cfg, sample_lengths), dtype=torch.int64)
    return (torch.arange(T)[None, :] < fl[:, None]).to(torch.float32)


def perplexity_from_counts(counts) -> float:
    """V:653-660 over any number of frames: mean_g exp(-sum_c p log(p + 1e-10)), p = clip(count / n, 1e-10, 1) with n the
    frames counted (the sum of a group's counts), in float64 on the host.  ``counts`` [G, Nc] integers.  The perplexity of
    an evaluation set is this function of the set's total counts - not a mean of per-batch values."""
    c = np.asarray(torch.as_tensor(counts).detach().cpu().numpy() if torch.is_tensor(counts) else counts, dtype=np.float64)
    if c.ndim != 2 or c.size == 0 or (c < 0).any():
        raise ValueError("perplexity_from_counts: counts must be [G, Nc] non-negative integers")
    n = c.sum(axis=1, keepdims=True)
    if not (n > 0).all():
        raise ValueError("perplexity_from_counts: no frame was counted")
    p = np.clip(c / n, 1e-10, 1.0)
    return float(np.exp(-(p * np.log(p + 1e-10)).sum(axis=1)).mean())


def check_evaluate_args(cfg: Wav2Vec2Config, audio, neg_indices, attention_mask=None, forced_codes=None, per_time=False):
    """The host-side checks of ``Wav2Vec2ForPreTraining.evaluate`` (the kernels cannot see values in device memory):
    ``audio`` float32 [B, T_in] with B >= 1; ``neg_indices`` int32 [B, Nn] (``per_time``: [T, Nn]) with Nn >= 1 and every
    entry in [0, T); ``attention_mask`` [B, T] over frames with values 0 or 1 only and at least one valid frame;
    ``forced_codes`` integer, B * T * G entries in [0, Nc).  -> (B, T_in, T, Nn, the mask as float32 on the host or None)."""
    if not torch.is_tensor(audio) or audio.dim() != 2 or audio.dtype != torch.float32 or audio.shape[0] < 1 or audio.shape[1] < 1:
        raise TypeError("audio must be float32 [B, T_in]")
    B, T_in = audio.shape
    T = frame_lengths(cfg, [T_in])[0]
    if not torch.is_tensor(neg_indices) or neg_indices.dtype != torch.int32 or neg_indices.dim() != 2:
        raise TypeError("neg_indices must be int32 [B, Nn] (or [T, Nn] with neg_per_time)")
    if neg_indices.shape[0] != (T if per_time else B):
        raise ValueError("neg_indices must have one row per " + ("time step" if per_time else "batch row"))
    Nn = int(neg_indices.shape[1])
    if Nn < 1:
        raise ValueError("neg_indices must hold at least one negative per row")
    ops.check_negative_indices(neg_indices, T)
    mask = None
    if attention_mask is not None:
        mask = torch.as_tensor(attention_mask).detach().to("cpu")
        if mask.dim() != 2 or tuple(mask.shape) != (B, T):
            raise ValueError(f"attention_mask must be [B, T] over frames = [{B}, {T}] (frame_attention_mask), got {list(mask.shape)}")
        mask = mask.to(torch.float32).contiguous()
        if not bool(((mask == 0) | (mask == 1)).all()):
            raise ValueError("attention_mask must be binary here: a frame is scored or it is not")
        if not float(mask.sum()) > 0.0:
            raise ValueError("attention_mask leaves no valid frame")
    if forced_codes is not None:
        G, Nc = cfg.num_codevector_groups, cfg.num_codevectors_per_group
        if not torch.is_tensor(forced_codes) or forced_codes.dtype not in (torch.int32, torch.int64) or forced_codes.numel() != B * T * G:
            raise ValueError(f"forced_codes must be integer [B, T, G] = [{B}, {T}, {G}]")
        if int(forced_codes.min()) < 0 or int(forced_codes.max()) >= Nc:
            raise ValueError(f"forced_codes must be in [0, {Nc})")
    return B, T_in, T, Nn, mask


class W2VArena(Arena):
    """``head="pretraining"``: the base model, the quantiser and the two projection heads (V:826-865).  ``head="ctc"``: the
    base model's parameters under the same names, then ``lm_head`` (V:940-975) - no quantiser, project_q or project_hid.
    ``head="classification"``: the base model likewise, then ``classifier_proj`` and ``classifier`` (V:1013-1015), the
    contiguous tail of the arena."""

    def __init__(self, cfg: Wav2Vec2Config, device, head: str = "pretraining"):
        if head not in ("pretraining", "ctc", "classification"):
            raise ValueError('head must be "pretraining", "ctc" or "classification"')
        pre = head == "pretraining"
        H, I = cfg.hidden_size, cfg.intermediate_size
        C, G = cfg.conv_dim[-1], cfg.num_conv_pos_embedding_groups
        spec: List[Tuple[str, Tuple[int, ...]]] = []

        def ln(p, n):
            spec.extend([(f"{p}.gamma", (n,)), (f"{p}.beta", (n,))])

        cin = 1
        for i, (c, k) in enumerate(zip(cfg.conv_dim, cfg.conv_kernel)):
            spec.append((f"feature_extractor.conv_layers.{i}.conv.kernel", (k, cin, c)))
            ln(f"feature_extractor.conv_layers.{i}.norm", c)
            cin = c
        spec.append(("feature_extractor.pos_conv_embed.kernel", (cfg.num_conv_pos_embeddings, C // G, C)))
        spec.append(("feature_extractor.pos_conv_embed.bias", (C,)))
        ln("feature_extractor.layer_norm", C)
        spec.extend([("feature_projection.kernel", (C, H)), ("feature_projection.bias", (H,))])
        ln("feature_projection_layer_norm", H)
        gd = cfg.codevector_dim // cfg.num_codevector_groups
        if pre:
            spec.extend([("quantizer.projection.kernel", (H, cfg.codevector_dim)), ("quantizer.projection.bias", (cfg.codevector_dim,)),
                         ("quantizer.codevectors", (cfg.num_codevector_groups, cfg.num_codevectors_per_group, gd))])
            spec.extend([("project_q.dense.kernel", (cfg.codevector_dim, cfg.proj_codevector_dim)),
                         ("project_q.dense.bias", (cfg.proj_codevector_dim,))])
            ln("project_q.layer_norm", cfg.proj_codevector_dim)
        for i in range(cfg.num_hidden_layers):
            p = f"encoder.layers.{i}"
            ln(f"{p}.attention_layer_norm", H)
            spec.extend([(f"{p}.attention.qkv3.kernel", (3, H, H)), (f"{p}.attention.qkv3.bias", (3, H)),
                         (f"{p}.attention.out_proj.kernel", (H, H)), (f"{p}.attention.out_proj.bias", (H,))])
            ln(f"{p}.feed_forward_layer_norm", H)
            spec.extend([(f"{p}.feed_forward.intermediate_dense.kernel", (H, I)), (f"{p}.feed_forward.intermediate_dense.bias", (I,)),
                         (f"{p}.feed_forward.output_dense.kernel", (I, H)), (f"{p}.feed_forward.output_dense.bias", (H,))])
        if pre:
            spec.extend([("project_hid.dense.kernel", (H, cfg.proj_codevector_dim)), ("project_hid.dense.bias", (cfg.proj_codevector_dim,))])
            ln("project_hid.layer_norm", cfg.proj_codevector_dim)
        elif head == "ctc":
            spec.extend([("lm_head.kernel", (H, cfg.vocab_size)), ("lm_head.bias", (cfg.vocab_size,))])
        else:
            P, Cl = cfg.classifier_proj_size, cfg.num_labels
            spec.extend([("classifier_proj.kernel", (H, P)), ("classifier_proj.bias", (P,)),
                         ("classifier.kernel", (P, Cl)), ("classifier.bias", (Cl,))])
        super().__init__(spec, device)


class Wav2Vec2ForPreTraining(KernelBlocks):
    """V:826-937: the pre-training step, and the forward pass alone of the model inside it (V:768-825, ``forward_infer``)."""

    _arena_head = "pretraining"  # which heads follow the base model in the arena (W2VArena)

    def __init__(self, config: Wav2Vec2Config, device="cuda:0", precision: str = "bf16", seed: int = 1234):
        if precision not in ("fp32", "bf16"):
            raise ValueError("precision must be 'fp32' or 'bf16'")
        ops.lib()
        self.config = config
        self.device = torch.device(device)
        self.precision = precision
        self.dtype = torch.float32 if precision == "fp32" else torch.bfloat16
        self.hidden = config.hidden_size
        self.layer_norm_eps = config.layer_norm_eps
        H = config.hidden_size
        if H % config.num_attention_heads:
            raise ValueError("hidden_size must divide by the head count")
        if precision == "bf16" and H // config.num_attention_heads != 64:
            raise ValueError("the fused attention kernel is built for head_dim 64")
        if config.conv_dim[-1] % config.num_conv_pos_embedding_groups:
            raise ValueError("conv_dim must divide by the group count")
        self.arena = W2VArena(config, self.device, self._arena_head)
        self.arena.init_keras_defaults(seed)
        self.ws: Dict[str, torch.Tensor] = {}
        self._ws_sets: Dict[tuple, Dict[str, torch.Tensor]] = {}
        self._ws_key = None
        self.mirror = None
        if precision == "bf16":
            self.mirror = torch.zeros(self.arena.numel, dtype=torch.bfloat16, device=self.device)
        k, Cg = config.num_conv_pos_embeddings, config.conv_dim[-1] // config.num_conv_pos_embedding_groups
        G = config.num_conv_pos_embedding_groups
        self.pos_wf = torch.empty((G, k * Cg, Cg), dtype=self.dtype, device=self.device)
        self.pos_wb = torch.empty_like(self.pos_wf)
        segs = self.arena.variable_segments()
        self.n_var = len(segs)
        so = torch.tensor([s for s, _ in segs] + [segs[-1][1]], dtype=torch.int64)
        # per-variable segments must tile [start, end) without gaps for the offset-array form;
        # alignment padding between tensors belongs to the preceding variable's tail (zeros)
        self.seg_vars = so.to(self.device)
        self.seg_chunks = ops.segment_chunks(so, device=self.device)  # the table Adam-with-clipping walks
        self.seg_all = torch.tensor([0, self.arena.numel], dtype=torch.int64, device=self.device)
        # The LATE slice of the clipped Adam update (train.ADAM_LATE, optim.Adam.apply_gradients_clipped(late_row=...)): the
        # arena from encoder layer L/6 to the end (the layers above it and project_hid, which follows them in the arena and
        # in the forward) - 77 % of the base model, first read a conv stack and L/6 layers into the next step.  Measured
        # (ms/step, two rounds on one box, 128 workgroups): from layer 2 4.66 / 4.58, 4: 4.71 / 4.63, 6: 4.73 / 4.63,
        # 8: 4.69 / 4.67; off: 4.74; 192 workgroups lose 0.05-0.07 everywhere, 64 do not finish in time (+0.09).
        Lh = config.num_hidden_layers
        self._late_first = max(1, int(os.environ.get("TMI_ADAM_LATE_LAYER", Lh // 6))) if Lh >= 3 else None
        if self._late_first is not None and self._late_first >= Lh:
            self._late_first = None
        self._late_row = None
        if self._late_first is not None:
            pre = f"encoder.layers.{self._late_first}."
            off = min(o for n, o in self.arena.offsets.items() if n.startswith(pre))
            rows = [i for i, (lo, _, _) in enumerate(self.seg_chunks.tolist()) if lo >= off]
            if rows and int(self.seg_chunks[rows[0], 0]) == off:
                self._late_row = (rows[0], off)
        self.refresh_shadows()
        # weight / bias gradients on a second stream beside the dgrad chain (blocks.KernelBlocks): 6.03 -> 5.9 ms
        self.enable_wgrad_stream(os.environ.get("TMI_WGRAD_STREAM", "1") != "0")

    def refresh_shadows(self):
        super().refresh_shadows()
        self._pack_pos()

    def _prepare_clip(self):
        if "clip_vars" not in self.ws:
            self._buf("clip_vars", (self.n_var,), torch.float32)
            self._buf("clip_all", (1,), torch.float32)

    def _pack_pos(self):
        cfg = self.config
        G = cfg.num_conv_pos_embedding_groups
        ops.posconv_pack_weights(self.arena.p, self.pos_wf, self.pos_wb, cfg.num_conv_pos_embeddings,
                                 cfg.conv_dim[-1] // G, G, w_off=self.arena.offsets["feature_extractor.pos_conv_embed.kernel"])

    # -- workspaces --------------------------------------------------------------------
    def _geometry(self, T_in: int) -> dict:
        """Geometry of the "same"-padded conv stem and of the grouped positional conv for ``T_in`` samples: per conv layer
        the output length ``lens``, the (left, right) ``pads`` and the padded input length ``Tp`` (layer 0's input is the
        audio itself, C = 1); the frame count ``T``; whether layer 0 runs as the fused filter bank (``fir0``); the
        positional conv's pads ``plp`` / ``prp`` and its padded lengths ``Tpp`` (forward) and ``Tpp2`` (gradient: full
        correlation).  Shared by training and inference."""
        cfg = self.config
        lens, pads, T = [], [], T_in
        for k, s in zip(cfg.conv_kernel, cfg.conv_stride):
            To, pl, pr = same_pad(T, k, s)
            pads.append((pl, pr))
            lens.append(To)
            T = To
        Tp = [([T_in] + lens)[i] + pads[i][0] + pads[i][1] for i in range(len(lens))]
        # conv layer 0 runs as a filter bank fused with its GroupNorm + GELU straight from the audio (tmi_fir_groupnorm_gelu_*)
        # whenever the reference's first-layer geometry holds (kernel 10, stride 5: every size of V:24-128)
        c0, Gn = cfg.conv_dim[0], cfg.num_conv_pos_embedding_groups
        fir0 = (cfg.conv_kernel[0] == 10 and cfg.conv_stride[0] == 5 and c0 % 8 == 0 and 2048 % c0 == 0 and
                (c0 // Gn) % 8 == 0 and os.environ.get("TMI_W2V_FIR", "1") != "0")
        kp = cfg.num_conv_pos_embeddings
        plp, prp = same_pad(T, kp, 1)[1:]
        return {"lens": lens, "pads": pads, "Tp": Tp, "T": T, "fir0": fir0, "plp": plp, "prp": prp, "Tpp": T + kp - 1,
                "Tpp2": T + 2 * (kp - 1)}

    def _prepare(self, B: int, T_in: int):
        if self._select_ws_set((B, T_in)):
            return
        cfg = self.config
        f32 = torch.float32
        L = len(cfg.conv_dim)
        geo = self._geo = self._geometry(T_in)
        # (the shape attributes model.T, model.lens, ...: the backward, tests, tools and bench read them)
        self.lens, self.pads, self.Tp, self.T, self.fir0, self.plp, self.prp, self.Tpp, self.Tpp2 = (
            geo[n] for n in ("lens", "pads", "Tp", "T", "fir0", "plp", "prp", "Tpp", "Tpp2"))
        Gn = cfg.num_conv_pos_embedding_groups
        slack = 2
        z = dict(zero=True)
        c0_ = cfg.conv_dim[0]
        if not self.fir0:
            self._buf("in0", (B, self.Tp[0] + slack + 8, 1), **z)
        else:
            self._buf("fir_wpart", (ops.fir_gn_workspace_floats(B, self.lens[0], c0_),), f32)
        cin = 1
        for i in range(L):
            c = cfg.conv_dim[i]
            if not (i == 0 and self.fir0):
                self._buf(f"u{i}", (B, self.lens[i], c))
            self._buf(f"gn{i}.stats", (B, Gn, 2), f32)
            if i + 1 < L:
                self._buf(f"in{i + 1}", (B, self.Tp[i + 1] + slack, c), **z)
                self._buf(f"din{i + 1}", (B, self.Tp[i + 1] + slack, c), **z)
            cin = c
        C, H = cfg.conv_dim[-1], cfg.hidden_size
        R = B * self.T
        Cg = C // Gn
        self._buf("h_last", (R, C))
        self._buf("xg", (Gn, B * self.Tpp, Cg))
        self._buf("yg", (Gn, B * self.Tpp, Cg))
        self._buf("dyg", (Gn, B * self.Tpp, Cg))
        self._buf("dyg2", (Gn, B * self.Tpp2, Cg))
        self._buf("dxg2", (Gn, B * self.Tpp2, Cg))
        self._buf("hp", (R, C))
        self._buf("feats", (R, C))
        self._buf("fe_ln.mean", (R,), f32); self._buf("fe_ln.rstd", (R,), f32)
        self._buf("fp_pre", (R, H))
        self._buf("fp_ln.mean", (R,), f32); self._buf("fp_ln.rstd", (R,), f32)
        cd, pd = cfg.codevector_dim, cfg.proj_codevector_dim
        self._buf("qin", (R, cd))
        self._buf("quant", (R, cd))
        self._buf("code_idx", (R, cfg.num_codevector_groups), torch.int32)
        self._buf("perplexity", (1,), f32)
        self._buf("pq_pre", (R, pd))
        # (64 zero rows behind the last batch: the backward's dS . pq runs its reduction over the PADDED row length of dS -
        # a whole number of K-tiles - and reads up to 63 rows past a batch's T: the next batch's, or these)
        self.ws["pq"] = self._buf("pq_pad", (R + 64, pd), zero=True)[:R]
        self._buf("pq_ln.mean", (R,), f32); self._buf("pq_ln.rstd", (R,), f32)
        self._buf("ph_pre", (R, pd)); self._buf("ph", (R, pd))
        self._buf("ph_ln.mean", (R,), f32); self._buf("ph_ln.rstd", (R,), f32)
        ff = cfg.intermediate_size
        Lh = cfg.num_hidden_layers
        # the operands of the layers' weight gradients live at a constant layer stride (one allocation per kind): the saved
        # forward activations xn1 / ctx / xn2 / g and the gradients dqkv / dya / dU / dyf each Dense layer receives, so that
        # after the backward loop ONE batched GEMM per kind computes that weight gradient for all layers (_wgrad_batched)
        for n, shp in (("xn1", (R, H)), ("ctx", (R, H)), ("xn2", (R, H)), ("g", (R, ff)),
                       ("dqkv", (R, 3 * H)), ("dya", (R, H)), ("dU", (R, ff)), ("dyf", (R, H))):
            self._buf_layers("enc", Lh, n, shp)
        for i in range(Lh):
            p = f"enc{i}."
            for n, shp in (("x_in", (R, H)), ("qkv", (R, 3 * H)), ("x_mid", (R, H)), ("u", (R, ff))):
                self._buf(p + n, shp)
            for s_ in ("ln1", "ln2"):
                self._buf(p + s_ + ".mean", (R,), f32); self._buf(p + s_ + ".rstd", (R,), f32)
            if self.precision == "bf16":
                self._buf(p + "stats", (B, cfg.num_attention_heads, self.T, 2), f32)
            else:
                self._buf(p + "P", (B, cfg.num_attention_heads, self.T, self.T), f32)
        self._buf("enc_x", (R, H))
        self._buf("S", (B, self.T, self.T), f32)
        self._buf("dS", (B, self.T, (self.T + 63) // 64 * 64))  # bf16 copy of dS, rows padded to whole 64-element K-tiles (zeros)
        self._buf("row_loss", (R,), f32)
        self._buf("closs", (1,), f32)
        self._buf("loss", (1,), f32)
        # backward scratch
        self._buf("dres", (R, H)); self._buf("dtmp", (R, H)); self._buf("dctx", (R, H))
        self._buf("dph", (R, pd)); self._buf("dpq", (R, pd)); self._buf("dpd", (R, pd)); self._buf("dpd_q", (R, pd))
        self._buf("dquant", (R, cd))
        self._buf("dfeats", (R, C)); self._buf("dhp", (R, C)); self._buf("dh_last", (R, C))
        if self.precision == "bf16":
            self._buf("delta", (B, cfg.num_attention_heads, self.T), f32)
        else:
            self._buf("dP", (B, cfg.num_attention_heads, self.T, self.T), f32)
        for i in range(L):  # conv-layer input gradients with a zero row in front (the k = 3 dgrad's tap at t - 1)
            if not (i == 0 and self.fir0):
                self._buf(f"dup{i}", (B, 1 + self.lens[i], cfg.conv_dim[i]), **z)
        nch = max([ops.groupnorm_chunks(t) for t in self.lens] + ([ops.fir_chunks(self.lens[0])] if self.fir0 else []))
        self._buf("gn_part", (B * nch * Gn * 2,), f32)
        self._buf("gn_sums", (B, Gn, 2), f32)
        self._buf("clip_all", (1,), f32)
        self._buf("clip_vars", (self.n_var,), f32)

    # -- forward blocks, shared by the training step, forward_infer and evaluate ------------------------------------------
    # Each takes a map of what differs between its callers: training passes the buffers and statistics it keeps for the
    # backward (``_train_bufs``), inference buffers every layer shares, without the GELU pre-activation ``u`` (None)
    # (``_infer_bufs``).  Buffers that have the same name in both workspace sets (in{i}, u{i}, h_last, xg, yg, hp, feats,
    # fp_pre, qin, quant, code_idx, perplexity, pq_pre, pq, ph_pre, ph) are read from ``self.ws``.  ``sites``: the dropout
    # sites apply (the training step; inference runs without dropout even after enable_dropout).  Map keys: x_out (the
    # feature projection's output, then each layer's), the layer's activations x_in, xn1, qkv, ctx, x_mid, xn2, g, u; the
    # names of the statistics: gn (GroupNorm of conv layer i: formatted with i), fe_ln, fp_ln, pq_ln, ph_ln, ln1, ln2, and
    # of the attention scratch att.

    def _feature_encoder(self, audio, geo, b, sites):
        """V:283-296, V:777-779: conv -> GroupNorm -> GELU per layer (each output lands in the padded buffer that is the
        next conv's im2col matrix), the grouped positional conv as one batched window-GEMM, LayerNorm into ws["feats"],
        the feature projection and its LayerNorm into b["x_out"] [B*T, H]."""
        cfg, ws, a = self.config, self.ws, self.arena
        B, T_in = audio.shape
        L, Gn, C = len(cfg.conv_dim), cfg.num_conv_pos_embedding_groups, cfg.conv_dim[-1]
        lens, pads, T = geo["lens"], geo["pads"], geo["T"]
        if not geo["fir0"]:
            in0 = ws["in0"]
            ops.feat_to_channels_last(audio, in0, B, 1, T_in, pads[0][0], in0.shape[1] - T_in - pads[0][0])
        cin = 1
        for i in range(L):
            c, k, s = cfg.conv_dim[i], cfg.conv_kernel[i], cfg.conv_stride[i]
            pre = f"feature_extractor.conv_layers.{i}.norm"
            stats = ws[b["gn"].format(i)]
            if i + 1 < L:
                y, ysb, yoff = ws[f"in{i + 1}"], ws[f"in{i + 1}"].stride(0), pads[i + 1][0] * c
            else:
                y, ysb, yoff = ws["h_last"], lens[i] * c, 0
            if i == 0 and geo["fir0"]:
                # C_in = 1: a filter bank, fused with GroupNorm + GELU, its output never written (fp32 master taps)
                ops.fir_groupnorm_gelu_fwd(audio, pads[0][0], a.param("feature_extractor.conv_layers.0.conv.kernel"), k, s,
                                           a.param(pre + ".gamma"), a.param(pre + ".beta"), y, ysb, stats,
                                           ws["gn_part"], B, lens[0], c, Gn, 1e-5, y_off=yoff)
            else:
                xin, u = ws[f"in{i}"], ws[f"u{i}"]
                self._gemm_xw(xin, f"feature_extractor.conv_layers.{i}.conv.kernel", u, lens[i], c, k * cin, s * cin,
                              ldc=c, nbatch=B, a_sb=xin.stride(0), c_sb=u.stride(0))
                ops.groupnorm_gelu_fwd(u, u.stride(0), a.param(pre + ".gamma"), a.param(pre + ".beta"), y, ysb,
                                       stats, ws["gn_part"], B, lens[i], c, Gn, 1e-5, y_off=yoff)
            cin = c
        # grouped positional conv (V:271-277, V:291) as one batched window-GEMM
        kp, Cg, Tpp = cfg.num_conv_pos_embeddings, C // Gn, geo["Tpp"]
        ops.group_pack(ws["h_last"], ws["xg"], B, T, C, Gn, Tpp, geo["plp"])
        ops.gemm(ws["xg"], self.pos_wf, ws["yg"], B * Tpp - (kp - 1), Cg, kp * Cg, Cg, 1, Cg, 1, Cg, nbatch=Gn,
                 a_sb=B * Tpp * Cg, b_sb=kp * Cg * Cg, c_sb=B * Tpp * Cg)
        ops.group_unpack(ws["yg"], a.param("feature_extractor.pos_conv_embed.bias"), ws["h_last"], ws["hp"], B, T, C, Gn,
                         Tpp, 0)
        # V:296, V:779: LayerNorm + Dropout in one pass (the quantiser sees the dropped features too, V:784)
        self._ln_fwd(ws["hp"], "feature_extractor.layer_norm", ws["feats"], b["fe_ln"], drop_site=SITE_FE if sites else None)
        self._dense_fwd(ws["feats"], "feature_projection.kernel", ws["fp_pre"])
        self._ln_fwd(ws["fp_pre"], "feature_projection_layer_norm", b["x_out"], b["fp_ln"],
                     drop_site=SITE_FP if sites else None)

    def _quantise(self, hproj, b, forced, sites):
        """V:784, V:557-560: the quantiser on the projected features ``hproj`` [B*T, H] (codes into ws["code_idx"], code
        vectors into ws["quant"]), then project_q and its LayerNorm into ws["pq"].  ``forced``: the caller has put the
        codes into ws["code_idx"] and tmi_vq_assign takes them instead of the argmin.  (The kernels' own perplexity counts
        every row, padding too.)"""
        cfg, ws, a = self.config, self.ws, self.arena
        R, Gq, Nc = hproj.shape[0], cfg.num_codevector_groups, cfg.num_codevectors_per_group
        gd = cfg.codevector_dim // Gq
        self._dense_fwd(hproj, "quantizer.projection.kernel", ws["qin"])
        if forced:
            ops.vq_assign(a.param("quantizer.codevectors"), ws["code_idx"], ws["quant"], ws["perplexity"], R, Gq, Nc, gd)
        else:
            ops.vq_nearest(ws["qin"], a.param("quantizer.codevectors"), ws["code_idx"], ws["quant"], ws["perplexity"], R,
                           Gq, Nc, gd)
        self._dense_fwd(ws["quant"], "project_q.dense.kernel", ws["pq_pre"])
        self._ln_fwd(ws["pq_pre"], "project_q.layer_norm", ws["pq"], b["pq_ln"], drop_site=SITE_PQ if sites else None)  # V:560

    def _enc_layer(self, i, b, B, T, sites, key_bias=None, attentions=None, attentions_dtype=None):
        """V:419-439 (stable layer norm): encoder layer i, b["x_in"] -> b["x_out"].  ``key_bias`` (inference): added to the
        scores of the masked keys; ``attentions``: a list that receives the layer's attention weights [B, Hh, T, T]
        (V:376) in ``attentions_dtype``."""
        cfg, a, H = self.config, self.arena, self.config.hidden_size
        p, Hh = f"encoder.layers.{i}", cfg.num_attention_heads
        R, sscale = B * T, 1.0 / math.sqrt(H // Hh)
        self._ln_fwd(b["x_in"], p + ".attention_layer_norm", b["xn1"], b["ln1"])
        wq, _ = self.W(p + ".attention.qkv3.kernel")  # [3H, H] view of the three blocks
        qkv = b["qkv"]
        ops.gemm(b["xn1"], wq, qkv, R, H, H, H, 1, H, 1, 3 * H, nbatch=3, b_sb=H * H, c_sb=H,
                 bias=a.param(p + ".attention.qkv3.bias"), bias_sb=H)
        self._attn_fwd(b["att"], (qkv, 0), (qkv, H), (qkv, 2 * H), b["ctx"], B, Hh, T, T, 0, score_scale=sscale,
                       site=SITE_ATTN + i if sites else None, key_bias=key_bias)
        if attentions is not None:
            attentions.append(self._attn_probs(b["att"], (qkv, 0), (qkv, H), B, Hh, T, T, 0, score_scale=sscale,
                                               key_bias=key_bias, dtype=attentions_dtype))
        # V:431: x + Dropout(attention output): the mask is a term of the GEMM epilogue
        self._dense_fwd(b["ctx"], p + ".attention.out_proj.kernel", b["x_mid"], resid=b["x_in"], r_ld=H,
                        **(self._drop_epi(SITE_ATTN_OUT + i) if sites else {}))
        self._ln_fwd(b["x_mid"], p + ".feed_forward_layer_norm", b["xn2"], b["ln2"])
        self._dense_fwd(b["xn2"], p + ".feed_forward.intermediate_dense.kernel", b["g"], act=1, aux_out=b["u"],
                        **(self._drop_epi(SITE_FFN_MID + i, p=self._drop_act_p) if sites else {}))  # V:393 on the GELU output
        self._dense_fwd(b["g"], p + ".feed_forward.output_dense.kernel", b["x_out"], resid=b["x_mid"], r_ld=H,
                        **(self._drop_epi(SITE_FFN_OUT + i) if sites else {}))  # V:396

    def _project_hid(self, x, b, sites):
        """V:550-561: the projection head on the encoder output ``x`` [B*T, H] into ws["ph"]."""
        self._dense_fwd(x, "project_hid.dense.kernel", self.ws["ph_pre"])
        self._ln_fwd(self.ws["ph_pre"], "project_hid.layer_norm", self.ws["ph"], b["ph_ln"],
                     drop_site=SITE_PH if sites else None)  # V:560

    def _train_bufs(self, i=None):
        """Training's buffer map: encoder layer i's own workspace entries (kept for the backward), or without ``i`` the map
        of the blocks around the encoder (the projection lands in the first layer's input: the encoder's input IS it)."""
        ws, Lh = self.ws, self.config.num_hidden_layers
        if i is None:
            return {"x_out": ws["enc0.x_in"] if Lh else ws["enc_x"], "gn": "gn{}.stats", "fe_ln": "fe_ln", "fp_ln": "fp_ln",
                    "pq_ln": "pq_ln", "ph_ln": "ph_ln"}
        k = f"enc{i}."
        b = {n: ws[k + n] for n in ("x_in", "xn1", "qkv", "ctx", "x_mid", "xn2", "g", "u")}
        b.update(ln1=k + "ln1", ln2=k + "ln2", att=k + ("stats" if self.precision == "bf16" else "P"),
                 x_out=ws[f"enc{i + 1}.x_in"] if i + 1 < Lh else ws["enc_x"])
        return b

    # -- forward + backward ----------------------------------------------------------------
    def forward_backward(self, audio: torch.Tensor, neg_indices: torch.Tensor, num_replicas: int = 1, forced_codes=None):
        """Pins the launch stream for the duration of the step (KernelBlocks.begin_step), then runs
        ``_forward_backward``.  ``forced_codes`` (int32 [B, T, G], parity runs only): the quantiser takes these code
        choices instead of its own argmin (tmi_vq_assign) - an argument of THIS call, never state of the model."""
        self.begin_step()
        try:
            return self._forward_backward(audio, neg_indices, num_replicas, forced_codes)
        finally:
            self.end_step()
            self._drop_step += 1

    def _forward_backward(self, audio: torch.Tensor, neg_indices: torch.Tensor, num_replicas: int = 1, forced=None):
        """One replica's V:1199-1240: returns the device scalar ``scaled_loss`` =
        (contrastive + 0.1 * (-perplexity)) / num_replicas; gradients of it land in ``arena.g``."""
        cfg = self.config
        B, T_in = audio.shape
        if audio.dtype != torch.float32 or neg_indices.dtype != torch.int32 or neg_indices.dim() != 2:
            raise TypeError("audio must be float32 [B, T] and neg_indices int32 [B, N] (or [T, N] with neg_per_time)")
        self._prepare(B, T_in)
        per_time = bool(getattr(self, "neg_per_time", False))  # whisper_single.py's negatives: one index row per time step
        if neg_indices.shape[0] != (self.T if per_time else B):
            raise ValueError("neg_indices must have one row per " + ("time step" if per_time else "batch row"))
        ws, a = self.ws, self.arena
        L = len(cfg.conv_dim)
        Gn = cfg.num_conv_pos_embedding_groups
        H, C = cfg.hidden_size, cfg.conv_dim[-1]
        T, R = self.T, B * self.T
        Hh = cfg.num_attention_heads
        hd = H // Hh
        sscale = 1.0 / math.sqrt(hd)
        if not getattr(a, "g_clean", False):
            self._wait_late()  # (a pending late Adam slice reads the gradients this fill would overwrite)
            ops.fill_zero(a.g)
        a.g_clean = False

        k = cfg.num_conv_pos_embeddings
        Cg = C // Gn
        Mw = B * self.Tpp - (k - 1)  # rows of the positional conv's window GEMM
        drop = self._drop_p > 0.0
        pa = self._drop_act_p
        Gq, Nc = cfg.num_codevector_groups, cfg.num_codevectors_per_group
        gd = cfg.codevector_dim // Gq
        pd = cfg.proj_codevector_dim

        # ---- forward: the shared blocks on the layers' own buffers, dropout sites on
        b = self._train_bufs()
        self._feature_encoder(audio, self._geo, b, True)
        if forced is not None:  # teacher-forced run: int32 [B*T, G] codes replace the argmin (a torch copy, as it always was)
            ws["code_idx"].copy_(forced.reshape(ws["code_idx"].shape))
        self._quantise(b["x_out"], b, forced is not None, True)  # on the projected features (V:784): no gradient flows back through it
        for i in range(cfg.num_hidden_layers):
            if i == self._late_first:
                self._wait_late()  # the previous step's Adam slice for this layer and everything after it, if left running
            self._enc_layer(i, self._train_bufs(i), B, T, True)
        self._project_hid(ws["enc_x"], b, True)

        # ---- contrastive loss (V:866-899)
        S = ws["S"]
        ops.gemm(ws["ph"], ws["pq"], S, T, T, pd, pd, 1, 1, pd, T, nbatch=B, a_sb=T * pd, b_sb=T * pd, c_sb=T * T)
        Nn = neg_indices.shape[1]
        inv_rep = 1.0 / num_replicas
        ops.contrastive_fwd_bwd(S, neg_indices, ws["row_loss"], B, T, Nn, cfg.contrastive_logits_temperature,
                                inv_rep / R, per_time=per_time)
        ops.sum_scale(ws["row_loss"], ws["closs"], R, 1.0 / R)
        ops.loss_combine(ws["closs"], ws["perplexity"], -cfg.diversity_loss_weight, inv_rep, ws["loss"])

        # ================= backward =================
        if self.precision == "bf16":
            # (T = 99 at 2 s clips: with the natural row stride neither product could use 16-byte loads - 35 + 26 us on the
            # generic kernel's scalar path for 40 MFLOP)
            dS, Tp = ws["dS"], ws["dS"].shape[2]
            ops.cast_bf16(S, T, dS, Tp, B * T, T)
        else:
            dS, Tp = S, T
        # d ph = dS · pq ; d pq = dSᵀ · ph   (per batch)
        # (K = Tp, not T: the pad columns of dS are zeros (tmi_cast_bf16 writes them), so the extra products vanish and the
        # launch takes the LDS-DMA kernels, whose k-contiguous operands come in whole 64-element K-tiles - with K = 99 it was
        # the step's only generic-kernel GEMM, 33 us for 40 MFLOP)
        # NB: rows T .. Tp-1 of a sample's ``pq`` operand are the NEXT sample's first rows (or the buffer's zero
        # tail) multiplied by exact zeros - a cross-sample read that is harmless only while ``pq`` is finite: an Inf / NaN in
        # sample b + 1's pq would turn 0 * Inf into NaN in sample b's dph.  A step whose activations are not finite is lost
        # either way (the loss is NaN), so the coupling costs nothing; it is stated here so that nobody relies on per-sample
        # isolation of this product.
        ops.gemm(dS, ws["pq"], ws["dph"], T, pd, Tp, Tp, 1, pd, 1, pd, nbatch=B, a_sb=T * Tp, b_sb=T * pd, c_sb=T * pd)
        ops.gemm(dS, ws["ph"], ws["dpq"], T, pd, T, 1, Tp, pd, 1, pd, nbatch=B, a_sb=T * Tp, b_sb=T * pd, c_sb=T * pd)
        # (the Dropout behind each head's LayerNorm: its mask is applied to dpq / dph as the LayerNorm backward loads them)
        # project_q branch -> codebook
        # (the quantiser branch ends in the codebook: its dense backward and the codebook scatter feed nothing on the chain
        # and run on the second stream, from a buffer of their own - ws["dpd"] is reused by the other head at once)
        self._ln_bwd(ws["dpq"], ws["pq_pre"], "project_q.layer_norm", ws["dpd_q"], "pq_ln", False, drop_site=SITE_PQ)
        self._dense_bwd(ws["quant"], ws["dpd_q"], "project_q.dense.kernel", ws["dquant"], dgrad_on_side=True)
        gcode = a.grad("quantizer.codevectors")
        self._run_on_side(lambda: ops.vq_bwd(ws["code_idx"], ws["dquant"], gcode, R, Gq, Nc, gd), ws["dquant"])
        # project_hid branch -> encoder output
        self._ln_bwd(ws["dph"], ws["ph_pre"], "project_hid.layer_norm", ws["dpd"], "ph_ln", False, drop_site=SITE_PH)
        dres = ws["dres"]
        self._dense_bwd(ws["enc_x"], ws["dpd"], "project_hid.dense.kernel", dres)

        # The gradient of the residual stream that a LayerNorm backward leaves in ``dres`` is the dy of the Dense layer below
        # it (attention out_proj under the FFN LayerNorm, the previous layer's output_dense under the attention LayerNorm):
        # that layer's bias gradient and its dy - dres, Dropout-masked with dropout - come out of the LayerNorm kernel
        # (tmi_layernorm_bwd_emit) instead of a dropout pass and a column-sum pass over dres.
        # Weight gradients of the encoder are batched over the layers.  Every Dense layer's dy is kept in a per-layer buffer:
        # dqkv / dU are written there by the kernels that produce them, the residual-stream gradients (dyf for output_dense,
        # dya for out_proj) are the second output of the LayerNorm backward above them.
        Lh = cfg.num_hidden_layers

        def emit(bias_name, buf, site):
            return (a.grad(bias_name), ws[buf], site)

        # The batched weight gradients go to the second stream in 4 CHUNKS of layers: a chunk starts as soon as the backward
        # chain has left its layers - that chain is a string of decoder-sized kernels on a mostly idle chip - instead of
        # everything queueing behind layer 0 and running into the conv-stack backward, whose own weight gradients share that
        # stream (measured with those on it, ms/step: 1 chunk 4.74, 2: 4.75, 3: 4.71, 4: 4.70).
        nchunk = max(1, min(Lh, 4))
        cuts = sorted({(Lh * j) // nchunk for j in range(nchunk)})   # chunk j = layers [cuts[j], cuts[j + 1])
        st = {n: ws[f"enc*.{n}"] for n in ("xn1", "ctx", "xn2", "g", "dqkv", "dya", "dU", "dyf")}
        lay = "encoder.layers.{}"

        def encoder_weight_grads(lo, hi):
            self._wgrad_batched(st["g"], st["dyf"], lay + ".feed_forward.output_dense.kernel", Lh, bias=False, lo=lo, hi=hi)
            if hi == Lh:  # (the one bias gradient the LayerNorm backward did not emit: the top layer's dres came from the head)
                ops.bias_grad(st["dyf"][Lh - 1], a.grad(lay.format(Lh - 1) + ".feed_forward.output_dense.bias"))
            self._wgrad_batched(st["xn2"], st["dU"], lay + ".feed_forward.intermediate_dense.kernel", Lh, lo=lo, hi=hi)
            self._wgrad_batched(st["ctx"], st["dya"], lay + ".attention.out_proj.kernel", Lh, bias=False, lo=lo, hi=hi)
            # the q / k / v blocks are three [H, H] kernels side by side in the arena: one launch per block over the layers
            gq0 = a.grad(lay.format(lo) + ".attention.qkv3.kernel")
            lstride = self._layer_stride(lay + ".attention.qkv3.kernel", Lh)
            xn1, dqs = st["xn1"][lo:hi], st["dqkv"][lo:hi]
            for j in range(3):
                ops.gemm(xn1, dqs, gq0, H, H, R, 1, H, 3 * H, 1, H, nbatch=hi - lo, a_sb=R * H, b_sb=R * 3 * H,
                         c_sb=lstride, b_off=j * H, c_off=j * H * H, splitk=0)
            ops.bias_grad_batched(dqs, a.grad(lay.format(lo) + ".attention.qkv3.bias"),
                                  self._layer_stride(lay + ".attention.qkv3.bias", Lh))

        for i in reversed(range(Lh)):
            p, kk = f"encoder.layers.{i}", f"enc{i}."
            dU, dt_, dctx, dqkv = ws[kk + "dU"], ws["dtmp"], ws["dctx"], ws[kk + "dqkv"]
            if i == Lh - 1:
                # the top layer's dres comes from the projection head's dgrad, not from a LayerNorm: its dy (the masked
                # gradient with dropout) is written here
                if drop:
                    self._dropout(dres, ws[kk + "dyf"], SITE_FFN_OUT + i)
                else:
                    self._guard_write(ws[kk + "dyf"])
                    ops.copy(ws[kk + "dyf"], dres)
            # d u = gelu'(u) * mask/keep * d g: both factors are epilogue terms of the dgrad (elementwise factors commute)
            self._dense_bwd(ws[kk + "g"], ws[kk + "dyf"], p + ".feed_forward.output_dense.kernel", dU, aux_in=ws[kk + "u"],
                            dgrad_epi=self._drop_epi(SITE_FFN_MID + i, p=pa), wgrad=False)
            self._dense_bwd(ws[kk + "xn2"], dU, p + ".feed_forward.intermediate_dense.kernel", dt_, wgrad=False)
            self._ln_bwd(dt_, ws[kk + "x_mid"], p + ".feed_forward_layer_norm", dres, kk + "ln2", True,
                         emit=emit(p + ".attention.out_proj.bias", kk + "dya", SITE_ATTN_OUT + i))
            self._dense_bwd(ws[kk + "ctx"], ws[kk + "dya"], p + ".attention.out_proj.kernel", dctx, wgrad=False)
            qkv = ws[kk + "qkv"]
            self._attn_bwd(kk + ("stats" if self.precision == "bf16" else "P"), (qkv, 0), (qkv, H), (qkv, 2 * H),
                           ws[kk + "ctx"], dctx, (dqkv, 0), (dqkv, H), (dqkv, 2 * H), B, Hh, T, T, 0, score_scale=sscale,
                           q_prescaled=False, site=SITE_ATTN + i)
            # the dgrad of the three q / k / v blocks, summed over them in one launch
            wq, _ = self.W(p + ".attention.qkv3.kernel")
            self._guard_write(dt_)
            ops.gemm(dqkv, wq, dt_, R, H, H, 3 * H, 1, 1, H, H, kbatch=3, a_skb=H, b_skb=H * H)
            self._ln_bwd(dt_, ws[kk + "x_in"], p + ".attention_layer_norm", dres, kk + "ln1", True,
                         emit=emit(f"encoder.layers.{i - 1}.feed_forward.output_dense.bias", f"enc{i - 1}.dyf",
                                   SITE_FFN_OUT + i - 1) if i > 0 else None)
            if i in cuts:
                # every dy of layers [i, next cut) is final (this layer's dqkv was the last to be written); the rest of the
                # step runs beside this chunk: the layers below, then the feature-projection / pos-conv / conv-stack backward
                lo, hi = i, ([c for c in cuts if c > i] + [Lh])[0]
                self._run_on_side(lambda lo=lo, hi=hi: encoder_weight_grads(lo, hi), ws[kk + "dqkv"])

        # hproj feeds the encoder only (the quantiser branch is non-differentiable)
        self._ln_bwd(dres, ws["fp_pre"], "feature_projection_layer_norm", ws["dtmp"], "fp_ln", False, drop_site=SITE_FP)
        self._dense_bwd(ws["feats"], ws["dtmp"], "feature_projection.kernel", ws["dfeats"])
        self._ln_bwd(ws["dfeats"], ws["hp"], "feature_extractor.layer_norm", ws["dhp"], "fe_ln", False, drop_site=SITE_FE)
        dhp = ws["dhp"]
        # hp = h_last + posconv(h_last) + bias
        ops.bias_grad(dhp, a.grad("feature_extractor.pos_conv_embed.bias"))
        ops.group_pack(dhp, ws["dyg"], B, T, C, Gn, self.Tpp, 0)
        gwp = a.grad("feature_extractor.pos_conv_embed.kernel")
        # (weight gradients of the positional conv and of the conv stack feed nothing on the chain: second stream.  Their
        # operands - the packed / padded forward inputs and the per-layer dy buffers - are not rewritten before the join)
        self._run_on_side(lambda: ops.gemm(ws["xg"], ws["dyg"], gwp, k * Cg, Cg, Mw, 1, Cg, Cg, 1, C, nbatch=Gn,
                                           a_sb=B * self.Tpp * Cg, b_sb=B * self.Tpp * Cg, c_sb=Cg, splitk=0), ws["dyg"])
        ops.group_pack(dhp, ws["dyg2"], B, T, C, Gn, self.Tpp2, k - 1)
        Mw2 = B * self.Tpp2 - (k - 1)
        ops.gemm(ws["dyg2"], self.pos_wb, ws["dxg2"], Mw2, Cg, k * Cg, Cg, 1, Cg, 1, Cg, nbatch=Gn,
                 a_sb=B * self.Tpp2 * Cg, b_sb=k * Cg * Cg, c_sb=B * self.Tpp2 * Cg)
        ops.group_unpack(ws["dxg2"], None, dhp, ws["dh_last"], B, T, C, Gn, self.Tpp2, self.plp)

        # ---- conv stack backward
        for i in reversed(range(L)):
            c, kc, s = cfg.conv_dim[i], cfg.conv_kernel[i], cfg.conv_stride[i]
            cin = cfg.conv_dim[i - 1] if i else 1
            Ti = self.lens[i]
            pre = f"feature_extractor.conv_layers.{i}.norm"
            if i + 1 < L:
                dy, dysb, dyoff = ws[f"din{i + 1}"], ws[f"din{i + 1}"].stride(0), self.pads[i + 1][0] * c
            else:
                dy, dysb, dyoff = ws["dh_last"], Ti * c, 0
            if i == 0 and self.fir0:
                wname0 = "feature_extractor.conv_layers.0.conv.kernel"
                ops.fir_groupnorm_gelu_bwd(audio, self.pads[0][0], a.param(wname0), kc, s, dy, dysb, a.param(pre + ".gamma"),
                                           a.param(pre + ".beta"), ws["gn0.stats"], a.grad(wname0), a.grad(pre + ".gamma"),
                                           a.grad(pre + ".beta"), ws["gn_part"], ws["gn_sums"], ws["fir_wpart"], B, Ti, c, Gn,
                                           dy_off=dyoff)
                continue
            u = ws[f"u{i}"]
            dup = ws[f"dup{i}"]  # [B, 1 + Ti, c], row 0 of every batch stays zero (allocated zeroed, never written)
            ops.groupnorm_gelu_bwd(u, u.stride(0), dy, dysb, a.param(pre + ".gamma"), a.param(pre + ".beta"),
                                   ws[f"gn{i}.stats"], dup, dup.stride(0), a.grad(pre + ".gamma"), a.grad(pre + ".beta"),
                                   ws["gn_part"], ws["gn_sums"], B, Ti, c, Gn, dy_off=dyoff, dx_off=c)
            wname = f"feature_extractor.conv_layers.{i}.conv.kernel"
            xin = ws[f"in{i}"]
            gw = a.grad(wname).view(kc * cin, c)
            self._run_on_side(lambda xin=xin, dup=dup, gw=gw, kc=kc, cin=cin, c=c, Ti=Ti, s=s:
                              ops.gemm(xin, dup, gw, kc * cin, c, Ti, 1, s * cin, c, 1, c, kbatch=B, a_skb=xin.stride(0),
                                       b_skb=dup.stride(0), b_off=c, splitk=0), dup)
            if i == 0:
                continue
            if s != 2 or kc not in (2, 3):
                raise NotImplementedError("conv dgrad is written for stride 2, kernel 2 or 3 (every reference size)")
            w, ldw = self.W(wname)  # [kc*cin, c]
            din = ws[f"din{i}"]
            # even padded rows u = 2j: taps kk = 0 (t = j) and, for k = 3, kk = 2 (t = j - 1)
            ops.gemm(dup, w, din, Ti, cin, c, c, 1, 1, ldw, 2 * cin, nbatch=B, a_sb=dup.stride(0), c_sb=din.stride(0),
                     kbatch=2 if kc == 3 else 1, a_skb=-c, b_skb=2 * cin * ldw, a_off=c)
            # odd padded rows u = 2j + 1: tap kk = 1
            ops.gemm(dup, w, din, Ti, cin, c, c, 1, 1, ldw, 2 * cin, nbatch=B, a_sb=dup.stride(0), c_sb=din.stride(0),
                     a_off=c, b_off=cin * ldw, c_off=cin)
        self._join_side()
        return ws["loss"]

    def __call__(self, inputs, neg_indices=None, attention_mask=None, output_hidden_states=False, pool=None, training=None,
                 output_attentions=False, attentions_dtype=None):
        """V:768-825.  ``training=True`` with ``neg_indices`` is the pre-training step (-> ``{"loss": ...}``); ``training=False``
        - the default when no ``neg_indices`` are given - is the forward pass alone, see ``forward_infer``."""
        if training is None:
            training = neg_indices is not None
        if training:
            if neg_indices is None:
                raise ValueError("the training path takes neg_indices")
            if attention_mask is not None or output_hidden_states or pool is not None or output_attentions or attentions_dtype is not None:
                raise ValueError("attention_mask, output_hidden_states, output_attentions, attentions_dtype and pool belong to the "
                                 "inference call (training=False)")
            return {"loss": self.forward_backward(inputs, neg_indices)}
        if neg_indices is not None:
            raise ValueError("neg_indices belong to the training call")
        return self.forward_infer(inputs, attention_mask=attention_mask, output_hidden_states=output_hidden_states, pool=pool,
                                  output_attentions=output_attentions, attentions_dtype=attentions_dtype)

    # -- inference (forward only): V:768-825 with training=False --------------------------------------------------------
    # Its own workspace set (``_inf``), never one of ``_ws_sets``: no saved pre-activations, no gradient buffers, every
    # encoder layer works in the same buffers.  It is ``self.ws`` only for the duration of a call (the blocks read
    # ``self.ws``); the geometry lives in the set, not in the attributes ``_prepare`` keeps for the step.  Nothing of the
    # training state (``_ws_key``, ``_ws_sets``, ``_drop_step``, ``arena.g`` / ``g_clean``, recorded plans, the optimizer) is
    # read or written, and no dropout site is passed: dropout is off even after ``enable_dropout``.

    def _infer_prepare(self, B: int, T_in: int) -> dict:
        inf = self.__dict__.get("_inf")
        if inf is not None and inf["key"] == (B, T_in):
            return inf
        self._inf = None  # (the previous set is released first)
        cfg = self.config
        f32 = torch.float32
        L, Gn = len(cfg.conv_dim), cfg.num_conv_pos_embedding_groups
        inf = dict(self._geometry(T_in), key=(B, T_in))
        lens, Tp, T, fir0 = inf["lens"], inf["Tp"], inf["T"], inf["fir0"]
        saved, self.ws = self.ws, {}
        try:
            slack = 2
            if not fir0:
                self._buf("in0", (B, Tp[0] + slack + 8, 1), zero=True)
            for i in range(L):
                c = cfg.conv_dim[i]
                if not (i == 0 and fir0):
                    self._buf(f"u{i}", (B, lens[i], c))
                if i + 1 < L:
                    self._buf(f"in{i + 1}", (B, Tp[i + 1] + slack, c), zero=True)  # (the pad rows stay zero: only rows of the clip are written)
            self._buf("gn.stats", (B, Gn, 2), f32)
            nch = max([ops.groupnorm_chunks(t) for t in lens] + ([ops.fir_chunks(lens[0])] if fir0 else []))
            self._buf("gn_part", (B * nch * Gn * 2,), f32)
            C, H, ff, Hh = cfg.conv_dim[-1], cfg.hidden_size, cfg.intermediate_size, cfg.num_attention_heads
            R, Cg = B * T, C // Gn
            for n, w in (("h_last", C), ("hp", C), ("feats", C), ("fp_pre", H), ("x", H), ("x_mid", H), ("xn", H), ("ctx", H),
                         ("qkv", 3 * H), ("g", ff)):
                self._buf(n, (R, w))
            self._buf("xg", (Gn, B * inf["Tpp"], Cg))
            self._buf("yg", (Gn, B * inf["Tpp"], Cg))
            self._buf("ln.mean", (R,), f32)
            self._buf("ln.rstd", (R,), f32)
            self._buf("att", (B, Hh, T, 2) if self.precision == "bf16" else (B, Hh, T, T), f32)
            inf["ws"] = self.ws
        finally:
            self.ws = saved
        self._inf = inf
        return inf

    def _check_mask(self, attention_mask, B, T):
        """[B, T] over frames, values in [0, 1], float or bool -> fp32 on the host."""
        m = torch.as_tensor(attention_mask).detach().to("cpu")
        if m.dim() != 2 or tuple(m.shape) != (B, T):
            raise ValueError(f"attention_mask must be [B, T] over frames = [{B}, {T}] (frame_attention_mask), got {list(m.shape)}")
        m = m.to(torch.float32)
        if not bool(((m >= 0) & (m <= 1)).all()):
            raise ValueError("attention_mask values must lie in [0, 1]")
        return m.contiguous()

    def _infer_bufs(self):
        """Inference's buffer map: every layer works in the same shared buffers, one LayerNorm-statistics buffer and one
        GroupNorm-statistics buffer serve every call, no GELU pre-activation, each layer's output overwrites its input."""
        ws = self.ws
        return {"x_in": ws["x"], "xn1": ws["xn"], "qkv": ws["qkv"], "ctx": ws["ctx"], "x_mid": ws["x_mid"], "xn2": ws["xn"],
                "g": ws["g"], "u": None, "x_out": ws["x"], "gn": "gn.stats", "att": "att",
                **{n: "ln" for n in ("fe_ln", "fp_ln", "pq_ln", "ph_ln", "ln1", "ln2")}}

    def _infer_body(self, audio, inf, key_bias, output_hidden_states=False, on_projection=None, attentions=None,
                    attentions_dtype=None):
        """The forward pass of ``forward_infer`` and ``evaluate`` on the inference workspace (``self.ws`` is ``inf["ws"]``):
        conv stem, positional conv, LayerNorm, feature projection, encoder layers with ``key_bias`` added to the scores of
        the masked keys.  -> (the last hidden state [B*T, H], a view of the workspace; the inputs of the layers when asked
        for).  ``on_projection(x)`` runs between the feature projection and the first layer.  ``attentions``: a list that
        receives every layer's attention weights [B, Hh, T, T] (V:376) in ``attentions_dtype``."""
        cfg = self.config
        B, T, H = audio.shape[0], inf["T"], cfg.hidden_size
        b = self._infer_bufs()
        x = b["x_in"]
        self._feature_encoder(audio, inf, b, False)
        if on_projection is not None:
            on_projection(x)  # (evaluate's quantiser branch, V:784: it reads the projection before the encoder overwrites it)
        hidden = []
        for i in range(cfg.num_hidden_layers):  # (each layer's output overwrites its input)
            if output_hidden_states:
                hidden.append(x.view(B, T, H).clone())
            self._enc_layer(i, b, B, T, False, key_bias, attentions, attentions_dtype)
        return x, hidden

    @torch.no_grad()
    def forward_infer(self, inputs, attention_mask=None, output_hidden_states=False, pool=None, output_attentions=False,
                      attentions_dtype=None):
        """The reference's ``Wav2Vec2Model.call(..., training=False)`` (V:768-825): conv stem, grouped positional conv,
        LayerNorm, feature projection with its LayerNorm, encoder layers; no quantiser, no projection heads, no loss, no
        dropout.  ``inputs`` float32 [B, T_in].  Returns a dict with ``last_hidden_state`` [B, T, H], ``extract_features``
        [B, T, C], with ``output_hidden_states`` ``hidden_states`` (the input of every layer and the output of the last:
        num_hidden_layers + 1 tensors, V:488-537) and with ``pool="mean"`` ``pooled_output`` fp32 [B, H], the masked mean
        over time of V:1031-1042 (the plain mean without a mask; a clip whose mask is all zero pools to zeros).  With
        ``output_attentions`` ``attentions``: one tensor [B, Hh, T, T] per layer (V:333-376, V:481-546), the softmax weights
        before dropout - with an ``attention_mask`` the masked ones - in ``attentions_dtype`` (None: the compute dtype;
        torch.float32 is allowed on the bf16 model).

        ``attention_mask`` [B, T] over FRAMES (``frame_attention_mask``), values in [0, 1], is the reference's argument as
        is: the host turns it into (1 - mask) * -10000 once, and every layer's attention adds that to the scores of the
        masked keys (V:352-355).  Only attention keys are masked, as in the reference: the stem's GroupNorm statistics and
        the positional conv see the padding, so a padded clip does NOT reproduce the same clip run alone - in the reference
        or here.  ``None`` runs the unmasked kernels of the training step."""
        cfg = self.config
        if pool not in (None, "mean"):
            raise ValueError('pool must be None or "mean"')
        if attentions_dtype not in (None, torch.float32, torch.bfloat16):
            raise ValueError("attentions_dtype must be None, torch.float32 or torch.bfloat16")
        if not torch.is_tensor(inputs) or inputs.dim() != 2 or inputs.dtype != torch.float32 or inputs.shape[0] < 1:
            raise TypeError("inputs must be float32 [B, T_in]")
        B, T_in = inputs.shape
        T = frame_lengths(cfg, [T_in])[0]
        mask = None if attention_mask is None else self._check_mask(attention_mask, B, T)
        audio = inputs.to(self.device).contiguous()
        inf = self._infer_prepare(B, T_in)
        with self._inference(inf):
            ws = self.ws
            H, C = cfg.hidden_size, cfg.conv_dim[-1]
            key_bias = mask_dev = None
            if mask is not None:
                mask_dev = mask.to(self.device)
                key_bias = ((1.0 - mask) * -10000.0).to(self.device)  # V:352-355, on the host, once per call
            attentions = [] if output_attentions else None
            x, hidden = self._infer_body(audio, inf, key_bias, output_hidden_states or self._head_reads_layers(),
                                         attentions=attentions, attentions_dtype=attentions_dtype)
            last = x.view(B, T, H).clone()
            result = {"last_hidden_state": last, "extract_features": ws["feats"].view(B, T, C).clone()}
            if output_hidden_states:
                result["hidden_states"] = tuple(hidden) + (last,)
            if output_attentions:
                result["attentions"] = tuple(attentions)
            if pool == "mean":
                pooled = torch.empty(B, H, dtype=torch.float32, device=self.device)
                ops.masked_mean_pool(x, mask_dev, pooled, B, T, H)
                result["pooled_output"] = pooled
            inf["layer_inputs"] = hidden
            try:
                self._infer_head(x, inf, result)
            finally:
                del inf["layer_inputs"]
        return result

    def _head_reads_layers(self) -> bool:
        """Whether ``_infer_head`` reads the inputs of the layers (``inf["layer_inputs"]``) beside the last hidden state:
        Wav2Vec2ForCTC with a layer mix attached.  The base model's does not."""
        return False

    def _infer_head(self, x, inf, result):
        """What a model with a head of its own adds to ``forward_infer``'s outputs from the last hidden state ``x`` [B*T, H],
        still inside the inference workspace (Wav2Vec2ForCTC: logits and log_probs).  The base model adds nothing."""


    # -- evaluation (forward only): the held-out contrastive loss, its accuracy and the code usage ------------------------
    def _eval_buffers(self, inf):
        """The buffers ``evaluate`` needs beyond ``forward_infer``'s, added to the inference set on the first call."""
        if "row_loss" in inf["ws"]:
            return
        cfg = self.config
        B = inf["key"][0]
        R = B * inf["T"]
        cd, pd = cfg.codevector_dim, cfg.proj_codevector_dim
        saved, self.ws = self.ws, inf["ws"]
        try:
            for n, w in (("qin", cd), ("quant", cd), ("pq_pre", pd), ("pq", pd), ("ph_pre", pd), ("ph", pd)):
                self._buf(n, (R, w))
            self._buf("code_idx", (R, cfg.num_codevector_groups), torch.int32)
            self._buf("perplexity", (1,), torch.float32)
            self._buf("row_loss", (R,), torch.float32)
            self._buf("row_correct", (R,), torch.int32)
            self._buf("code_counts", (cfg.num_codevector_groups, cfg.num_codevectors_per_group), torch.int64)
        finally:
            self.ws = saved

    @torch.no_grad()
    def evaluate(self, audio, neg_indices, attention_mask=None, forced_codes=None, return_rows=False):
        """Held-out pre-training metrics of one batch, forward only (V:768-825 with training=False, the quantiser of V:784,
        the heads of V:550-561 and the loss of V:866-899; the combination of V:1220): on the inference workspace, dropout
        off, nothing of the training state read or written (see ``forward_infer``).

        ``audio`` float32 [B, T_in]; ``neg_indices`` int32 [B, Nn], or [T, Nn] when ``neg_per_time`` is set, as in
        ``forward_backward``; ``attention_mask`` [B, T] over frames (``frame_attention_mask``), binary: it masks the
        attention keys as in ``forward_infer``, a masked frame is not scored as a query, and a negative that names a masked
        frame is dropped from its row's softmax (tmi_contrastive_score); ``forced_codes`` int [B, T, G] replace the
        quantiser's argmin (tmi_vq_assign).  Returns Python numbers, float64 on the host: ``loss_sum``, ``n_correct``,
        ``n_frames`` (sums over the valid frames), ``code_counts`` (int64 [G, Nc] CPU tensor: this call's counts over the
        valid frames), ``contrastive_loss`` = loss_sum / n_frames, ``accuracy``, ``perplexity``
        (``perplexity_from_counts(code_counts)``) and ``loss`` = contrastive_loss - diversity_loss_weight * perplexity.
        With ``return_rows`` also the device tensors ``row_loss`` fp32 / ``row_correct`` int32 [B, T], ``code_indices``
        int32 [B, T, G], ``projected_states`` and ``projected_quantized_features`` [B, T, pd]."""
        cfg = self.config
        per_time = bool(getattr(self, "neg_per_time", False))
        B, T_in, T, Nn, mask = check_evaluate_args(cfg, audio, neg_indices, attention_mask, forced_codes, per_time)
        audio = audio.to(self.device).contiguous()
        neg = neg_indices.to(self.device).contiguous()
        forced = None if forced_codes is None else forced_codes.to(self.device, torch.int32).reshape(B * T, -1).contiguous()
        inf = self._infer_prepare(B, T_in)
        self._eval_buffers(inf)
        with self._inference(inf):
            ws, b = self.ws, self._infer_bufs()
            R = B * T
            Gq, Nc, pd = cfg.num_codevector_groups, cfg.num_codevectors_per_group, cfg.proj_codevector_dim
            key_bias = mask_dev = None
            if mask is not None:
                mask_dev = mask.to(self.device)
                key_bias = ((1.0 - mask) * -10000.0).to(self.device)

            def quantise(hproj):  # V:784: the quantiser sees the projected features; then project_q (V:557-559)
                if forced is not None:
                    ops.copy(ws["code_idx"], forced)
                self._quantise(hproj, b, forced is not None, False)  # (its perplexity is ignored: the counts below replace it)

            x, _ = self._infer_body(audio, inf, key_bias, on_projection=quantise)
            self._project_hid(x, b, False)
            ops.contrastive_score(ws["ph"], ws["pq"], neg, ws["row_loss"], ws["row_correct"], B, T, pd, Nn,
                                  cfg.contrastive_logits_temperature, mask=mask_dev, per_time=per_time, validate=False)
            ops.fill_zero(ws["code_counts"])
            ops.vq_count(ws["code_idx"], mask_dev, ws["code_counts"], R, Gq, Nc)
            # the sums in float64 on the host (rows of masked frames hold 0 / 0)
            loss_sum = float(ws["row_loss"].cpu().double().sum())
            n_correct = float(ws["row_correct"].cpu().double().sum())
            counts = ws["code_counts"].cpu().clone()
            n_frames = float(R if mask is None else mask.double().sum())
            result = {"loss_sum": loss_sum, "n_correct": n_correct, "n_frames": n_frames, "code_counts": counts,
                      "contrastive_loss": loss_sum / n_frames, "accuracy": n_correct / n_frames,
                      "perplexity": perplexity_from_counts(counts)}
            result["loss"] = result["contrastive_loss"] - cfg.diversity_loss_weight * result["perplexity"]
            if return_rows:
                result.update(row_loss=ws["row_loss"].view(B, T).clone(), row_correct=ws["row_correct"].view(B, T).clone(),
                              code_indices=ws["code_idx"].view(B, T, Gq).clone(),
                              projected_states=ws["ph"].view(B, T, pd).clone(),
                              projected_quantized_features=ws["pq"].view(B, T, pd).clone())
        return result


# ---------------------------------------------------------------------------------------------------------------------
# CTC (V:940-1001): the head, greedy decoding, the loss and forced alignment, and training of the HEAD alone on cached
# features of the frozen encoder.  The head trains, the encoder does not: encoder fine-tuning is not built.
CTC_MAX_LABELS = 511   # tmi_ctc_forward: one thread per extended state, 2 L + 1 <= 1023
CTC_MAX_FRAMES = 4096  # tmi_ctc_viterbi: the moves of a walk-back piece are staged in LDS
CTC_MAX_BEAMS = 16     # tmi_ctc_beam: one wave per beam
SAMPLE_RATE = 16000


def frame_seconds(cfg: Wav2Vec2Config) -> float:
    """Seconds per encoder frame: the product of the conv strides over the sample rate (20 ms for every reference size)."""
    return float(np.prod(cfg.conv_stride)) / SAMPLE_RATE


def check_ctc_args(cfg: Wav2Vec2Config, inputs_shape, labels=None, label_lengths=None, attention_mask=None):
    """Host validation of ``Wav2Vec2ForCTC.decode`` / ``evaluate`` / ``align`` / ``posteriors`` (no GPU needed; the kernels
    cannot see values in device memory).  ``inputs_shape`` (B, T_in); ``labels`` None or integer [B, L_max] with every entry inside its row's
    ``label_lengths`` in [0, vocab_size) and not the blank, L_max <= 511; ``label_lengths`` None (L_max everywhere) or B
    integers in [0, L_max]; ``attention_mask`` None or [B, T] over frames (``frame_attention_mask``), values 0 or 1 only,
    every row ones first and zeros behind them, at least one frame per row.
    -> (B, T, frame_lens int32 [B] - the mask's row sums, or T -, the mask as float32 on the host or None, labels int32
    [B, max(L_max, 1)] or None, label_lengths int32 [B] or None)."""
    if len(inputs_shape) != 2 or int(inputs_shape[0]) < 1 or int(inputs_shape[1]) < 1:
        raise ValueError("inputs must be [B, T_in]")
    B, T_in = int(inputs_shape[0]), int(inputs_shape[1])
    V, blank = cfg.vocab_size, cfg.ctc_blank_id
    if not 2 <= V <= 64:
        raise ValueError("the CTC head takes 2 <= vocab_size <= 64 (tmi_ctc_logsoftmax: one lane per column)")
    if not 0 <= blank < V:
        raise ValueError("ctc_blank_id must be in [0, vocab_size)")
    T = frame_lengths(cfg, [T_in])[0]
    mask, frame_lens = None, np.full(B, T, dtype=np.int32)
    if attention_mask is not None:
        mask = torch.as_tensor(attention_mask).detach().to("cpu")
        if mask.dim() != 2 or tuple(mask.shape) != (B, T):
            raise ValueError(f"attention_mask must be [B, T] over frames = [{B}, {T}] (frame_attention_mask), got {list(mask.shape)}")
        mask = mask.to(torch.float32).contiguous()
        if not bool(((mask == 0) | (mask == 1)).all()):
            raise ValueError("attention_mask must be binary here: a frame belongs to the clip or it does not")
        frame_lens = mask.sum(dim=1).to(torch.int32).numpy()
        if not bool((mask == (torch.arange(T)[None, :] < torch.from_numpy(frame_lens)[:, None]).to(torch.float32)).all()):
            raise ValueError("attention_mask must be a prefix per row: ones on the clip's frames, zeros behind them")
        if int(frame_lens.min()) < 1:
            raise ValueError("attention_mask leaves a row without a frame")
    lab, lens = _check_ctc_labels(cfg, B, labels, label_lengths)
    return B, T, frame_lens, mask, lab, lens


def _check_ctc_labels(cfg: Wav2Vec2Config, B: int, labels, label_lengths):
    """The label rules of ``check_ctc_args`` for ``B`` items -> (labels int32 [B, max(L_max, 1)], lengths int32 [B]), or
    (None, None) without labels."""
    V, blank = cfg.vocab_size, cfg.ctc_blank_id
    lab = lens = None
    if labels is None:
        if label_lengths is not None:
            raise ValueError("label_lengths come with labels")
    else:
        lab = torch.as_tensor(labels).detach().to("cpu")
        if lab.dim() != 2 or lab.shape[0] != B or lab.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"labels must be integer [B, L_max] = [{B}, L_max]")
        L_max = int(lab.shape[1])
        if L_max > CTC_MAX_LABELS:
            raise ValueError(f"at most {CTC_MAX_LABELS} labels per item (tmi_ctc_forward: one thread per extended state)")
        if label_lengths is None:
            lens = np.full(B, L_max, dtype=np.int32)
        else:
            lens = np.asarray(torch.as_tensor(label_lengths).detach().to("cpu").numpy()).astype(np.int64).reshape(-1)
            if lens.shape[0] != B or (lens < 0).any() or (lens > L_max).any():
                raise ValueError(f"label_lengths must be B = {B} integers in [0, L_max = {L_max}]")
            lens = lens.astype(np.int32)
        lab = lab.to(torch.int32).numpy()
        inside = np.arange(L_max)[None, :] < lens[:, None]
        if ((lab < 0) | (lab >= V))[inside].any():
            raise ValueError(f"labels must be in [0, {V}) inside their length")
        if (lab == blank)[inside].any():
            raise ValueError(f"labels must not hold the blank ({blank}) inside their length")
        if L_max == 0:
            lab = np.zeros((B, 1), dtype=np.int32)  # (the kernels take L_max >= 1; every length is 0)
        lab = np.ascontiguousarray(lab)
    return lab, lens


CTC_HEAD_MAX_ITEMS = 65535    # tmi_ctc_head_fwd / _bwd: items per call
CTC_HEAD_MAX_ROWS = 1 << 22   # items x frames per call
CTC_HEAD_MAX_HIDDEN = 4096    # H, a multiple of 8


def check_ctc_head_args(cfg: Wav2Vec2Config, hidden_shape, hidden_dtype, frame_lengths, labels, label_lengths=None):
    """Host validation of the cached-feature calls of ``Wav2Vec2ForCTC`` (``head_step`` through ``fit_ctc_head``,
    ``evaluate_features``; no GPU needed).  ``hidden_shape`` (N, T_max, H) with H the model's hidden size, a multiple of 8
    and <= 4096, 1 <= T_max <= 4096; ``hidden_dtype`` torch.float32 or torch.bfloat16; ``frame_lengths`` N integers in
    [1, T_max]; ``labels`` / ``label_lengths`` under the rules of ``check_ctc_args``; 2 <= vocab_size <= 64.  N itself is not
    limited: the calls cut it into pieces of at most 65535 items and 2^22 frames (``ctc_head_batch_limit``).
    -> (N, T_max, frame_lens int32 [N], labels int32 [N, max(L_max, 1)], label_lengths int32 [N]) on the host."""
    if len(hidden_shape) != 3 or any(int(s) < 1 for s in hidden_shape):
        raise ValueError("hidden must be [N, T_max, H]")
    N, T_max, H = (int(s) for s in hidden_shape)
    if H != cfg.hidden_size or H % 8 or not 8 <= H <= CTC_HEAD_MAX_HIDDEN:
        raise ValueError(f"hidden must be [N, T_max, hidden_size = {cfg.hidden_size}], a multiple of 8 in [8, {CTC_HEAD_MAX_HIDDEN}]")
    if T_max > CTC_MAX_FRAMES:
        raise ValueError(f"at most {CTC_MAX_FRAMES} frames per item (tmi_ctc_posteriors), got {T_max}")
    if hidden_dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("hidden must be float32 or bfloat16")
    if not 2 <= cfg.vocab_size <= 64:
        raise ValueError("the CTC head takes 2 <= vocab_size <= 64 (tmi_ctc_logsoftmax: one lane per column)")
    if not 0 <= cfg.ctc_blank_id < cfg.vocab_size:
        raise ValueError("ctc_blank_id must be in [0, vocab_size)")
    fl = np.asarray(torch.as_tensor(frame_lengths).detach().to("cpu").numpy())
    if fl.dtype.kind not in "iu" or fl.reshape(-1).shape[0] != N or fl.ndim != 1:
        raise ValueError(f"frame_lengths must be N = {N} integers")
    if (fl < 1).any() or (fl > T_max).any():
        raise ValueError(f"frame_lengths must lie in [1, T_max = {T_max}]")
    if labels is None:
        raise ValueError("labels are required")
    lab, lens = _check_ctc_labels(cfg, N, labels, label_lengths)
    return N, T_max, fl.astype(np.int32), lab, lens


LAYER_MIX_MAX_LAYERS = 64   # tmi_layer_mix_fwd / _bwd: K


class LayerMix:
    """The learned mixing logits of a weighted sum over K layers of hidden states (``use_weighted_layer_sum``, the
    frozen-encoder protocol of SUPERB / s3prl) and their Adam state: fp32 ``logits`` (zeros: uniform weights), ``grad`` and
    the moments ``m``, ``v``, K entries each.  It lives OUTSIDE the model's arena - the arena's layout and the files of
    ``train.save_weights`` are what they were - and is updated by ``head_step`` with ``ops.adam_step`` on its own four
    buffers under the optimizer's hyper-parameters and iteration count (``learning_rate``: its own rate; None: the
    optimizer's).  The allocations are padded to a multiple of 4 entries, the 16-byte granularity of tmi_adam_step; the pad
    stays zero and the mixing kernels read K entries only."""

    def __init__(self, num_layers, device="cuda:0", learning_rate=None):
        K = int(num_layers)
        if not 1 <= K <= LAYER_MIX_MAX_LAYERS:
            raise ValueError(f"1 <= num_layers <= {LAYER_MIX_MAX_LAYERS}, got {num_layers}")
        self.num_layers, self.device = K, torch.device(device)
        self.learning_rate = None if learning_rate is None else float(learning_rate)
        self._n = -(-K // 4) * 4
        self._p, self._g, self._m, self._v = (torch.zeros(self._n, dtype=torch.float32, device=self.device) for _ in range(4))

    logits = property(lambda self: self._p[:self.num_layers])
    grad = property(lambda self: self._g[:self.num_layers])
    m = property(lambda self: self._m[:self.num_layers])
    v = property(lambda self: self._v[:self.num_layers])

    def weights(self):
        """softmax(logits), fp32 [K] on the mix's device (what tmi_layer_mix_fwd forms, to its rounding)."""
        return torch.softmax(self.logits.double(), 0).float()

    def state_dict(self):
        return {k: getattr(self, k).detach().cpu().clone() for k in ("logits", "m", "v")}

    def load_state_dict(self, state):
        """``logits`` [K] is required; ``m`` and ``v`` are zeroed when absent (a mix saved as its logits alone)."""
        if "logits" not in state:
            raise ValueError("a LayerMix state holds logits")
        for k, buf in (("logits", self._p), ("m", self._m), ("v", self._v)):
            if k in state:
                t = torch.as_tensor(np.asarray(state[k], dtype=np.float32) if not torch.is_tensor(state[k]) else state[k])
                if tuple(t.shape) != (self.num_layers,):
                    raise ValueError(f"{k} must hold num_layers = {self.num_layers} entries, got {list(t.shape)}")
                buf[:self.num_layers].copy_(t.to(torch.float32))
            else:
                buf.zero_()
        self._g.zero_()

    def adam_step(self, optimizer):
        """Adam over the K logits from ``grad`` with ``optimizer``'s hyper-parameters and its CURRENT iteration count."""
        lr = optimizer.learning_rate if self.learning_rate is None else self.learning_rate
        ops.adam_step(self._p, self._g, self._m, self._v, self._n, lr, optimizer.beta_1, optimizer.beta_2, optimizer.epsilon,
                      optimizer.iterations, optimizer.eps_mode, optimizer.weight_decay, 1.0)


def check_layer_mix_args(cfg: Wav2Vec2Config, layers_shape, layers_dtype, mix):
    """Host validation of a stacked-layers argument of the CTC probe (no GPU needed): ``layers_shape`` (K, N, T_max, H) with
    K = ``mix.num_layers`` in [1, 64], H the model's hidden size (a multiple of 8, <= 4096), 1 <= T_max <= 4096;
    ``layers_dtype`` torch.float32 or torch.bfloat16; ``mix`` a ``LayerMix``.  -> (K, N, T_max)."""
    if not isinstance(mix, LayerMix):
        raise TypeError("layer_mix must be a wav2vec2.LayerMix")
    if len(layers_shape) != 4 or any(int(s) < 1 for s in layers_shape):
        raise ValueError("with a layer mix hidden must be the stacked layers [K, N, T_max, H] (encode_features(layers=\"all\"))")
    K, N, T_max, H = (int(s) for s in layers_shape)
    if K != mix.num_layers or not 1 <= K <= LAYER_MIX_MAX_LAYERS:
        raise ValueError(f"hidden stacks {K} layers, the mix weighs {mix.num_layers} (1 .. {LAYER_MIX_MAX_LAYERS})")
    if H != cfg.hidden_size or H % 8 or not 8 <= H <= CTC_HEAD_MAX_HIDDEN:
        raise ValueError(f"hidden must be [K, N, T_max, hidden_size = {cfg.hidden_size}], a multiple of 8 in [8, {CTC_HEAD_MAX_HIDDEN}]")
    if T_max > CTC_MAX_FRAMES:
        raise ValueError(f"at most {CTC_MAX_FRAMES} frames per item (tmi_ctc_posteriors), got {T_max}")
    if layers_dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("hidden must be float32 or bfloat16")
    return K, N, T_max


SITE_SPEC = 7  # V:1073-1119: the SpecAugment span masks on the probes' cached features (tmi_spec_masks)
SPEC_MAX_LENGTH = 64   # tmi_spec_masks: columns one start can mask


@dataclass
class SpecAugment:
    """The span masks of ``apply_time_mask`` / ``apply_feature_mask`` (V:1073-1119) for ``head_step`` / ``fit_ctc_head``:
    every frame (column) of an item starts a span of ``mask_time_length`` frames (``mask_feature_length`` columns) with
    probability ``mask_time_prob`` (``mask_feature_prob``); a probability of 0 turns that mask off.  The defaults are the
    reference's time mask (and HF's ``mask_time_prob`` / ``mask_time_length``)."""
    mask_time_prob: float = 0.05
    mask_time_length: int = 10
    mask_feature_prob: float = 0.0
    mask_feature_length: int = 10


def spec_site_seed(seed: int, step: int) -> int:
    """The seed tmi_spec_masks takes in step ``step`` of a run seeded with ``seed`` (site SITE_SPEC)."""
    return (int(seed) + int(step) * 0x9E3779B97F4A7C15 + SITE_SPEC * 0xD1B54A32D192ED03) & 0xFFFFFFFFFFFFFFFF


def check_spec_augment_args(spec, T, H):
    """Host validation of a ``SpecAugment`` for items of ``T`` frames and ``H`` columns (no GPU needed): both probabilities
    in [0, 1) - and below 1 - 2^-17, where the 16-bit threshold would round to 65536 -, both lengths integers in [1, 64],
    1 <= T <= 4096, H a multiple of 8 in [8, 4096].  -> (time on, feature on)."""
    if not isinstance(spec, SpecAugment):
        raise TypeError("spec_augment must be a wav2vec2.SpecAugment")
    T, H = int(T), int(H)
    if not 1 <= T <= CTC_MAX_FRAMES:
        raise ValueError(f"1 <= T <= {CTC_MAX_FRAMES} frames per item, got {T}")
    if H % 8 or not 8 <= H <= CTC_HEAD_MAX_HIDDEN:
        raise ValueError(f"H must be a multiple of 8 in [8, {CTC_HEAD_MAX_HIDDEN}], got {H}")
    for name in ("mask_time", "mask_feature"):
        prob, length = getattr(spec, name + "_prob"), getattr(spec, name + "_length")
        if isinstance(prob, bool) or not isinstance(prob, (int, float, np.floating, np.integer)) or not 0.0 <= float(prob) < 1.0 \
                or int(np.float32(prob) * np.float32(65536.0) + np.float32(0.5)) > 65535:
            raise ValueError(f"{name}_prob must be in [0, 1), got {prob!r}")
        if isinstance(length, bool) or not isinstance(length, (int, np.integer)) or not 1 <= int(length) <= SPEC_MAX_LENGTH:
            raise ValueError(f"1 <= {name}_length <= {SPEC_MAX_LENGTH} (an integer), got {length!r}")
    return float(spec.mask_time_prob) > 0.0, float(spec.mask_feature_prob) > 0.0


def _spec_mask_buffers(N, T, H, time_on, feat_on, device):
    i32 = dict(dtype=torch.int32, device=device)
    return (torch.zeros((N, ops.spec_masks_words(T)), **i32) if time_on else None,
            torch.zeros((N, ops.spec_masks_words(H)), **i32) if feat_on else None, torch.zeros((N, 2), **i32))


def spec_augment_masks(spec, N, T, H, seed=0, step=0, device="cuda:0"):
    """The masks ``head_step(spec_augment=spec, seed=seed, step=step)`` applies to a step of ``N`` items (by position), ``T``
    frames and ``H`` columns, from one tmi_spec_masks launch -> (``time_bits`` int32 [N, ceil(T / 32)], ``feature_bits`` int32
    [N, ceil(H / 32)], ``counts`` int32 [N, 2]: the set bits per item).  A mask whose probability is 0 is None, its count 0."""
    time_on, feat_on = check_spec_augment_args(spec, T, H)
    N = int(N)
    if not 1 <= N <= ctc_head_batch_limit(T):
        raise ValueError(f"1 <= N <= {ctc_head_batch_limit(T)} items of {T} frames")
    tb, fb, counts = _spec_mask_buffers(N, int(T), int(H), time_on, feat_on, torch.device(device))
    if time_on or feat_on:
        ops.spec_masks(N, T, H, tb, fb, counts, spec.mask_time_prob, spec.mask_time_length, spec.mask_feature_prob,
                       spec.mask_feature_length, spec_site_seed(seed, step))
    return tb, fb, counts


def unpack_mask_bits(bits, cols):
    """``bits`` int32 [N, >= ceil(cols / 32)] as tmi_spec_masks writes them -> bool [N, cols] on the same device."""
    cols = int(cols)
    words = (cols + 31) // 32
    if not torch.is_tensor(bits) or bits.dtype != torch.int32 or bits.dim() != 2 or bits.shape[1] < words:
        raise ValueError(f"bits must be int32 [N, >= {words}]")
    w = bits[:, :words].to(torch.int64).unsqueeze(-1) >> torch.arange(32, device=bits.device)
    return (w & 1).bool().reshape(bits.shape[0], words * 32)[:, :cols]


def _apply_span_mask(hidden_states, mask_prob, mask_length, seed, step, time):
    x = hidden_states
    if not torch.is_tensor(x) or x.dim() != 3 or x.dtype not in (torch.float32, torch.bfloat16) or not x.is_cuda:
        raise TypeError("hidden_states must be a float32 or bfloat16 device tensor [B, T, H]")
    B, T, H = (int(s) for s in x.shape)
    spec = SpecAugment(mask_prob if time else 0.0, mask_length if time else 1, 0.0 if time else mask_prob, 1 if time else mask_length)
    check_spec_augment_args(spec, T, H)
    if not 1 <= B <= ctc_head_batch_limit(T):
        raise ValueError(f"1 <= B <= {ctc_head_batch_limit(T)} items of {T} frames")
    if x.stride(2) != 1 or x.stride(1) < H or x.stride(0) < T * x.stride(1):
        x = x.contiguous()
    bits = torch.zeros((B, ops.spec_masks_words(T if time else H)), dtype=torch.int32, device=x.device)
    with torch.cuda.device(x.device):
        ops.spec_masks(B, T, H, bits if time else None, None if time else bits, None, mask_prob, mask_length, mask_prob, mask_length,
                       spec_site_seed(seed, step))
        out = torch.empty((B, T, H), dtype=x.dtype, device=x.device)
        ops.span_mask_apply(x, out, bits if time else None, None if time else bits)
    mask = unpack_mask_bits(bits, T if time else H).to(torch.float32)
    return out, mask.unsqueeze(-1) if time else mask.unsqueeze(1)


def apply_time_mask(hidden_states, mask_prob=0.05, mask_length=10, seed=0, step=0):
    """V:1073-1094 on the device: every frame of every item starts, with probability ``mask_prob``, a span of ``mask_length``
    frames that is set to zero (tmi_spec_masks' time mask under (``seed``, ``step``) in place of TF's global stream, then
    tmi_span_mask_apply).  ``hidden_states`` bf16 / fp32 [B, T, H], H a multiple of 8 -> (``masked_hidden_states`` in the
    input's dtype, ``expanded_mask`` fp32 [B, T, 1], 1 where masked)."""
    return _apply_span_mask(hidden_states, mask_prob, mask_length, seed, step, True)


def apply_feature_mask(hidden_states, mask_prob=0.05, mask_length=10, seed=0, step=0):
    """V:1098-1119 on the device: the same over the columns of every item (the feature mask) -> (``masked_hidden_states``,
    ``expanded_mask`` fp32 [B, 1, H])."""
    return _apply_span_mask(hidden_states, mask_prob, mask_length, seed, step, False)


def ctc_head_batch_limit(T_max: int) -> int:
    """The most items one tmi_ctc_head call takes at ``T_max`` frames: 65535, and 2^22 frames in all."""
    return max(1, min(CTC_HEAD_MAX_ITEMS, CTC_HEAD_MAX_ROWS // int(T_max)))


def check_ctc_beam_args(cfg: Wav2Vec2Config, num_beams=None, num_return_sequences=1):
    """Host validation of the beam arguments of ``Wav2Vec2ForCTC.decode`` / ``evaluate`` (no GPU needed): ``num_beams`` None
    or an integer in [1, 16] (None and 1: greedy decoding), ``num_return_sequences`` an integer with
    1 <= num_return_sequences <= num_beams.  -> (K, R) as integers, K = 1 for the greedy path."""
    def integer(v):
        return isinstance(v, (int, np.integer)) and not isinstance(v, bool)
    if not 2 <= cfg.vocab_size <= 64 or not 0 <= cfg.ctc_blank_id < cfg.vocab_size:
        raise ValueError("the CTC head takes 2 <= vocab_size <= 64 and ctc_blank_id in [0, vocab_size)")
    K = 1 if num_beams is None else num_beams
    if not integer(K) or not 1 <= K <= CTC_MAX_BEAMS:
        raise ValueError(f"num_beams must be None or an integer in [1, {CTC_MAX_BEAMS}] (tmi_ctc_beam: one wave per beam)")
    if not integer(num_return_sequences) or not 1 <= num_return_sequences <= K:
        raise ValueError("num_return_sequences must be an integer with 1 <= num_return_sequences <= num_beams")
    return int(K), int(num_return_sequences)


def check_ctc_confusion_args(cfg: Wav2Vec2Config, confusion=False, edit_ops=False) -> bool:
    """Host validation of ``Wav2Vec2ForCTC.evaluate``'s ``confusion`` (no GPU needed): a bool; True only together with
    ``edit_ops=True`` - the table is folded from the alignment of the kernel path, the host loop has none.  -> the flag."""
    if not isinstance(confusion, (bool, np.bool_)):
        raise TypeError("confusion must be a bool (the CLI's path is not the flag)")
    if confusion and not edit_ops:
        raise ValueError("confusion=True needs edit_ops=True (the table comes from tmi_edit_align's steps)")
    return bool(confusion)


CTC_LM_MAX_ORDER = 4          # tmi_ctc_beam_lm: a dense table of V^order entries ...
CTC_LM_MAX_ENTRIES = 1 << 24  # ... of at most this many


def check_ctc_lm_args(cfg: Wav2Vec2Config, lm, lm_alpha=0.5, lm_beta=0.0, num_beams=None):
    """Host validation of the language-model arguments of ``Wav2Vec2ForCTC.decode`` / ``evaluate`` (no GPU needed; the
    kernel cannot check the table's values).  ``lm`` None (then nothing else is looked at), or a float tensor or array of
    shape [V] * order, or flat with V^order entries, 1 <= order <= 4 and V^order <= 2^24: ``lm[..., c]`` is log P(c | the
    previous order - 1 tokens), most recent last, ``ctc_blank_id`` in a context slot before the sequence's start (tmi_ctc_beam_lm in
    include/tethys_mi.h).  Entries finite or -inf (a forbidden transition), never NaN or +inf; ``lm_alpha`` >= 0 and
    ``lm_beta`` finite numbers; a table comes with ``num_beams`` >= 2 - the greedy path has no ranking to fuse it into.
    -> None, or (the table as a contiguous float32 CPU tensor [V^order], order, alpha, beta)."""
    if lm is None:
        return None
    K, _ = check_ctc_beam_args(cfg, num_beams)
    if K < 2:
        raise ValueError("lm comes with num_beams >= 2: greedy decoding has no ranking to fuse a language model into")
    V = cfg.vocab_size
    table = torch.as_tensor(lm).detach().to("cpu")
    if not table.dtype.is_floating_point:
        raise ValueError("lm must be a float tensor or array")
    n = table.numel()
    if table.dim() == 1:
        order = next((o for o in range(1, CTC_LM_MAX_ORDER + 1) if V ** o == n), None)
    else:
        order = table.dim() if all(int(s) == V for s in table.shape) else None
    if order is None or not 1 <= order <= CTC_LM_MAX_ORDER or V ** order > CTC_LM_MAX_ENTRIES:
        raise ValueError(f"lm must have shape [V] * order or V^order entries flat, V = {V}, 1 <= order <= {CTC_LM_MAX_ORDER}, "
                         f"V^order <= 2^24; got {list(table.shape)}")
    table = table.to(torch.float32).contiguous().view(-1)
    if bool(torch.isnan(table).any()) or bool((table == math.inf).any()):
        raise ValueError("lm entries must be finite or -inf (a forbidden transition), never NaN or +inf")
    for name, v in (("lm_alpha", lm_alpha), ("lm_beta", lm_beta)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not abs(float(v)) <= float(np.finfo(np.float32).max):
            raise ValueError(f"{name} must be a finite number (in float32)")
    if float(lm_alpha) < 0:
        raise ValueError("lm_alpha must be >= 0")
    return table, order, float(lm_alpha), float(lm_beta)


def ngram_lm_table(sequences, lengths, order, vocab_size, blank, add_k=1.0):
    """A dense n-gram table for ``decode(lm=...)`` from label sequences: ``sequences`` integer [N, L_max] (or a list of
    rows), ``lengths`` N integers.  Every token of every sequence counts once in the row of its ``order - 1`` predecessors,
    slots before the sequence's start holding ``blank``; counts in float64, then add-k smoothing over the non-blank
    columns: P(c | ctx) = (n(ctx, c) + add_k) / (n(ctx) + add_k (V - 1)), so every row sums to 1 over them (a row
    without counts is uniform; with add_k = 0 an unseen transition is -inf, and so is a whole row that was never seen).
    Column ``blank`` holds -inf.  -> float32 numpy [V] * order of log-probabilities."""
    V, order = int(vocab_size), int(order)
    if not 2 <= V <= 64 or not 0 <= blank < V or not 1 <= order <= CTC_LM_MAX_ORDER or V ** order > CTC_LM_MAX_ENTRIES:
        raise ValueError("ngram_lm_table: 2 <= vocab_size <= 64, blank inside it, 1 <= order <= 4, V^order <= 2^24")
    if not add_k >= 0 or not math.isfinite(add_k):
        raise ValueError("ngram_lm_table: add_k must be finite and >= 0")
    lengths = [int(n) for n in lengths]
    if len(lengths) != len(sequences):
        raise ValueError("ngram_lm_table: one length per sequence")
    mod = V ** (order - 1)
    counts = np.zeros((mod, V), dtype=np.float64)
    for row, n in zip(sequences, lengths):
        row = [int(t) for t in list(row)[:n]]
        if len(row) != n or n < 0 or any(not 0 <= t < V or t == blank for t in row):
            raise ValueError("ngram_lm_table: tokens must be in [0, vocab_size) and not the blank inside their length")
        ctx = blank * sum(V ** i for i in range(order - 1))
        for t in row:
            counts[ctx, t] += 1.0
            ctx = (ctx * V + t) % mod
    cols = np.arange(V) != blank
    num = counts + add_k
    den = counts[:, cols].sum(axis=1, keepdims=True) + add_k * (V - 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        table = np.where(den > 0, np.log(num) - np.log(den), -np.inf)
    table[:, blank] = -np.inf
    return table.astype(np.float32).reshape((V,) * order)


def edit_distance(hyp: np.ndarray, ref: np.ndarray) -> int:
    """Levenshtein distance of two integer sequences, one row of the table per hypothesis token, each row in numpy:
    d[j] = min(up + 1, diagonal + (h != r_j), d[j-1] + 1), the last term as a running minimum of d[j] - j."""
    hyp, ref = np.asarray(hyp), np.asarray(ref)
    n = len(ref)
    idx = np.arange(n + 1)
    d = idx.copy()
    for i, h in enumerate(hyp, 1):
        cand = np.empty(n + 1, dtype=np.int64)
        cand[0] = i
        cand[1:] = np.minimum(d[1:] + 1, d[:-1] + (ref != h))
        d = np.minimum.accumulate(cand - idx) + idx
    return int(d[n])


class Wav2Vec2ForCTC(Wav2Vec2ForPreTraining):
    """V:940-1001 at inference: the base model (stem, positional conv, projection, encoder - the blocks and the inference
    workspace of ``Wav2Vec2ForPreTraining``) and a Dense head (V:972-975) over ``vocab_size`` symbols, with greedy CTC
    decoding, the CTC loss and forced alignment on the kernels of csrc/ctc.hip, and the forward-backward posteriors of
    csrc/ctc_post.hip.  Every inference method runs under
    ``torch.no_grad()`` on the inference workspace with dropout off, and reads or writes nothing of the training state.
    The head trains, the encoder does not: ``encode_features`` caches the frozen encoder's output, ``head_step`` /
    ``fit_ctc_head`` train ``lm_head`` on it (csrc/ctc_head.hip around tmi_ctc_posteriors) and touch nothing of the arena
    outside the head's slice, ``evaluate_features`` scores it.  With a ``LayerMix`` the probe reads a learned
    softmax-weighted sum of all layers (csrc/layer_mix.hip; ``encode_features(layers="all")``, ``layer_mix=`` on the three
    calls, ``set_layer_mix`` for inference).  ``spec_augment=`` (a ``SpecAugment``) on ``head_step`` / ``fit_ctc_head`` zeroes
    spans of frames and of columns of the features inside the head kernels (csrc/spec_augment.hip draws the masks as bits);
    no inference or evaluation call masks.  The whole-model training entry points raise.  Not built: encoder fine-tuning,
    a LayerNorm per layer before the mix, label smoothing."""

    _arena_head = "ctc"

    def __init__(self, config: Wav2Vec2Config, device="cuda:0", precision: str = "bf16", seed: int = 1234):
        if not 2 <= config.vocab_size <= 64:
            raise ValueError("the CTC head takes 2 <= vocab_size <= 64 (tmi_ctc_logsoftmax: one lane per column)")
        if not 0 <= config.ctc_blank_id < config.vocab_size:
            raise ValueError("ctc_blank_id must be in [0, vocab_size)")
        if config.ctc_loss_reduction not in ("sum", "mean"):
            raise ValueError('ctc_loss_reduction must be "sum" or "mean"')
        super().__init__(config, device=device, precision=precision, seed=seed)
        a = self.arena
        self.head_lo, self.head_hi = a.offsets["lm_head.kernel"], a.numel  # the head: the arena's contiguous tail
        self._head_sets: Dict[tuple, Dict[str, torch.Tensor]] = {}
        self._layer_mix: Optional[LayerMix] = None

    def forward_backward(self, *a, **k):
        raise NotImplementedError("CTC fine-tuning is not built")

    def set_layer_mix(self, mix):
        """Attach (or, with None, detach) a ``LayerMix`` over the num_hidden_layers + 1 hidden states.  While one is attached
        the head of every inference call - ``model(inputs)``, ``decode`` (greedy, beam, LM), ``evaluate``, ``align``,
        ``posteriors`` - reads tmi_layer_mix_fwd of the layers' inputs and the last layer's output, then tmi_ctc_head_fwd
        without dropout from the fp32 master weights (as ``evaluate_features`` does), so they follow a probe trained with
        ``head_step(layer_mix=...)``.  ``last_hidden_state`` stays the encoder's.  With None the head is the GEMM it was."""
        if mix is not None:
            if not isinstance(mix, LayerMix):
                raise TypeError("set_layer_mix takes a wav2vec2.LayerMix or None")
            if mix.num_layers != self.config.num_hidden_layers + 1:
                raise ValueError(f"the mix must weigh num_hidden_layers + 1 = {self.config.num_hidden_layers + 1} layers, "
                                 f"got {mix.num_layers}")
            if mix.device != self.device:
                raise ValueError("the mix must live on the model's device")
        self._layer_mix = mix

    def _head_reads_layers(self) -> bool:
        return self._layer_mix is not None

    def __call__(self, inputs, attention_mask=None, training=False, **kw):
        """``model(inputs, attention_mask=None, training=False)`` is ``forward_infer``."""
        if training:
            raise NotImplementedError("CTC fine-tuning is not built")
        return self.forward_infer(inputs, attention_mask=attention_mask, **kw)

    # -- the head ----------------------------------------------------------------------------------------------------
    def _ctc_buffers(self, inf):
        """The head's buffers, added to the inference set on the first call."""
        if "ctc_logits" in inf["ws"]:
            return
        B, V = inf["key"][0], self.config.vocab_size
        R = B * inf["T"]
        saved, self.ws = self.ws, inf["ws"]
        try:
            self._buf("ctc_logits", (R, V), torch.float32)
            self._buf("ctc_logp", (R, V), torch.float32)
            self._buf("ctc_argmax", (R,), torch.int32)
        finally:
            self.ws = saved

    def _ctc_head(self, x, inf, layer_inputs=None):
        """V:972-975: logits = x . lm_head + bias as ONE tmi_gemm into fp32 (bf16 operands on the bf16 model: the logits are
        never rounded to bf16), then tmi_ctc_logsoftmax.  -> (logits, log_probs fp32 [B*T, V], argmax int32 [B*T])."""
        self._ctc_buffers(inf)
        ws = inf["ws"]
        if self._layer_mix is not None:
            return self._ctc_head_mixed(x, inf, layer_inputs)
        self._dense_fwd(x, "lm_head.kernel", ws["ctc_logits"])
        ops.ctc_logsoftmax(ws["ctc_logits"], self.config.vocab_size, ws["ctc_logp"], ws["ctc_argmax"])
        return ws["ctc_logits"], ws["ctc_logp"], ws["ctc_argmax"]

    def _ctc_head_mixed(self, x, inf, layer_inputs):
        """The head behind the attached layer mix: tmi_layer_mix_fwd over ``layer_inputs`` (the input of every layer, as
        ``_infer_body`` collects them) and ``x``, then ONE tmi_ctc_head_fwd without dropout from the fp32 master weights,
        which writes logits, log-probs and argmax.  Every frame is computed, as the GEMM path computes every frame."""
        ws, cfg = inf["ws"], self.config
        B, T, H, V = inf["key"][0], inf["T"], cfg.hidden_size, cfg.vocab_size
        if layer_inputs is None or len(layer_inputs) != cfg.num_hidden_layers:
            raise RuntimeError("the attached layer mix needs the inputs of all layers (_infer_body(output_hidden_states=True))")
        if "ctc_mixed" not in ws:
            saved, self.ws = self.ws, ws
            try:
                self._buf("ctc_mixed", (B, T, H), torch.float32)
            finally:
                self.ws = saved
            ws["ctc_all_frames"] = torch.full((B,), T, dtype=torch.int32, device=self.device)
        a = self.arena
        ops.layer_mix_fwd(list(layer_inputs) + [x.view(B, T, H)], self._layer_mix.logits, ws["ctc_all_frames"], ws["ctc_mixed"])
        ops.ctc_head_fwd(ws["ctc_mixed"], a.param("lm_head.kernel"), a.param("lm_head.bias"), ws["ctc_all_frames"],
                         ws["ctc_logp"].view(B, T, V), logits=ws["ctc_logits"].view(B, T, V), argmax=ws["ctc_argmax"])
        return ws["ctc_logits"], ws["ctc_logp"], ws["ctc_argmax"]

    def _infer_head(self, x, inf, result):
        B, T, V = inf["key"][0], inf["T"], self.config.vocab_size
        logits, logp, _ = self._ctc_head(x, inf, inf.get("layer_inputs"))
        result["logits"] = logits.view(B, T, V).clone()
        result["log_probs"] = logp.view(B, T, V).clone()

    @contextlib.contextmanager
    def _ctc_pass(self, inputs, labels=None, label_lengths=None, attention_mask=None):
        """The forward pass and the head of one batch, inside the inference workspace: yields what decode / evaluate /
        align share."""
        if not torch.is_tensor(inputs) or inputs.dim() != 2 or inputs.dtype != torch.float32:
            raise TypeError("inputs must be float32 [B, T_in]")
        cfg = self.config
        B, T, frame_lens, mask, lab, lens = check_ctc_args(cfg, tuple(inputs.shape), labels, label_lengths, attention_mask)
        audio = inputs.to(self.device).contiguous()
        inf = self._infer_prepare(B, inputs.shape[1])
        with self._inference(inf):
            key_bias = None if mask is None else ((1.0 - mask) * -10000.0).to(self.device)  # V:352-355, as forward_infer
            x, layer_inputs = self._infer_body(audio, inf, key_bias, self._layer_mix is not None)
            _, logp, amax = self._ctc_head(x, inf, layer_inputs)
            i32 = dict(dtype=torch.int32, device=self.device)
            yield {"B": B, "T": T, "V": cfg.vocab_size, "logp": logp.view(B, T, cfg.vocab_size), "argmax": amax.view(B, T),
                   "frame_lens": torch.from_numpy(frame_lens).to(self.device), "frame_lens_host": frame_lens,
                   "labels": None if lab is None else torch.from_numpy(lab).to(self.device), "labels_host": lab,
                   "label_lens": None if lens is None else torch.from_numpy(lens).to(self.device), "label_lens_host": lens,
                   "L_max": 0 if labels is None else int(torch.as_tensor(labels).shape[1]), "i32": i32, "f32": dict(dtype=torch.float32, device=self.device)}

    def _greedy(self, c):
        B, T = c["B"], c["T"]
        out = {n: torch.full((B, T), -1, **c["i32"]) for n in ("tokens", "start", "end")}
        out["len"] = torch.zeros(B, **c["i32"])
        out["best"] = torch.zeros(B, **c["f32"])
        ops.ctc_greedy(c["argmax"], c["logp"], c["frame_lens"], self.config.ctc_blank_id, out["tokens"], out["len"],
                       out["start"], out["end"], out["best"])
        return out

    def _times(self, frames):
        return torch.where(frames >= 0, frames.to(torch.float64) * frame_seconds(self.config), -1.0)

    def _beam(self, c, K, lm=None):
        """tmi_ctc_beam on the pass's log-probs -> tokens [B, K, T] (-1 past a length), len [B, K], scores [B, K], n [B].
        ``lm`` (what ``check_ctc_lm_args`` returned): tmi_ctc_beam_lm instead, the table moved to the device here, once per
        call; ``scores`` is then the fused score, and ``ctc`` / ``lm`` [B, K] are its two terms."""
        B, T = c["B"], c["T"]
        out = {"tokens": torch.full((B, K, T), -1, **c["i32"]), "len": torch.zeros((B, K), **c["i32"]),
               "scores": torch.full((B, K), -math.inf, **c["f32"]), "n": torch.zeros(B, **c["i32"])}
        wsp = torch.empty(ops.ctc_beam_workspace_elems(B, K, T), **c["i32"])
        if lm is None:
            ops.ctc_beam(c["logp"], c["frame_lens"], self.config.ctc_blank_id, K, out["tokens"], out["len"], out["scores"],
                         out["n"], wsp)
            return out
        table, order, alpha, beta = lm
        out["ctc"], out["lm"] = torch.full((B, K), -math.inf, **c["f32"]), torch.zeros((B, K), **c["f32"])
        ops.ctc_beam_lm(c["logp"], c["frame_lens"], self.config.ctc_blank_id, K, table.to(self.device), order, alpha, beta,
                        out["tokens"], out["len"], out["scores"], out["ctc"], out["lm"], out["n"], wsp)
        return out

    def _check_beam_frames(self, inputs, what):
        if torch.is_tensor(inputs) and inputs.dim() == 2 and inputs.shape[1] >= 1:
            T = frame_lengths(self.config, [int(inputs.shape[1])])[0]
            if T > CTC_MAX_FRAMES:
                raise ValueError(f"{what} with num_beams takes at most {CTC_MAX_FRAMES} frames, got {T}")

    @torch.no_grad()
    def decode(self, inputs, attention_mask=None, num_beams=None, num_return_sequences=1, return_timestamps=False,
               lm=None, lm_alpha=0.5, lm_beta=0.0):
        """Greedy CTC decoding: per frame the most probable symbol, runs of equal symbols collapsed, blanks dropped
        (tmi_ctc_greedy).  -> ``sequences`` int32 [B, max length] padded with -1, ``lengths`` int32 [B],
        ``token_start_frames`` / ``token_end_frames`` int32 (the first frame of a token's run and its last plus 1; -1 in the
        padding), ``token_start_times`` / ``token_end_times`` float64 seconds (frames x ``frame_seconds``; -1 in the padding),
        ``best_path_logprob`` fp32 [B]: the sum of the chosen symbols' log-probabilities over the clip's frames.

        ``num_beams`` in [2, 16]: CTC prefix beam search (tmi_ctc_beam in include/tethys_mi.h) - the label sequences whose
        paths together carry the most probability, not the best path.  With R = ``num_return_sequences`` <= num_beams
        -> ``sequences`` int32 [B, R, max length] padded with -1, ``lengths`` int32 [B, R], ``sequences_scores`` fp32 [B, R]
        (the log-probability the search kept for the sequence, descending; -inf past ``n_beams``), ``n_beams`` int32 [B] (the
        ranks the search filled, of num_beams); R == 1 drops the rank dimension.  ``return_timestamps`` adds
        ``token_start_frames`` / ``token_end_frames`` int32 [B, max best length] and the times of the BEST sequence of each
        item: its forced alignment (tmi_ctc_viterbi on the same log-probs, the labels never leave the device).  At most
        4096 frames; timestamps take a best sequence of at most 511 tokens.  ``num_beams`` None or 1 is the greedy path.

        ``lm`` (with ``num_beams`` >= 2; see ``check_ctc_lm_args``, ``ngram_lm_table`` builds one): an n-gram table of
        log-probabilities fused into the ranking WHILE the search runs (tmi_ctc_beam_lm in include/tethys_mi.h), which
        rescoring an n-best list cannot do - a prefix the model prefers is pruned by then.  A beam ranks by its CTC
        log-probability + ``lm_alpha`` x the table's log-probabilities of its tokens + ``lm_beta`` x its length; -inf
        entries forbid a transition.  ``sequences_scores`` is then this fused score and the result adds ``ctc_scores`` and
        ``lm_scores``, its two terms, shaped like it; timestamps are those of the fused search's best sequence.  Not built:
        an end-of-sequence term, word-level models, lexicons beyond -inf entries, backoff structures.  ``lm`` None is the
        search without a model: the same kernel and launches as before."""
        K, R = check_ctc_beam_args(self.config, num_beams, num_return_sequences)
        lm = check_ctc_lm_args(self.config, lm, lm_alpha, lm_beta, num_beams)
        if K > 1:
            return self._decode_beam(inputs, attention_mask, K, R, return_timestamps, lm)
        with self._ctc_pass(inputs, attention_mask=attention_mask) as c:
            g = self._greedy(c)
            n = max(int(g["len"].max()), 0)  # (the one host read: the width of the result)
            st, en = g["start"][:, :n].clone(), g["end"][:, :n].clone()
            return {"sequences": g["tokens"][:, :n].clone(), "lengths": g["len"], "token_start_frames": st,
                    "token_end_frames": en, "token_start_times": self._times(st), "token_end_times": self._times(en),
                    "best_path_logprob": g["best"]}

    def _decode_beam(self, inputs, attention_mask, K, R, return_timestamps, lm=None):
        self._check_beam_frames(inputs, "decode")
        with self._ctc_pass(inputs, attention_mask=attention_mask) as c:
            B, T = c["B"], c["T"]
            bm = self._beam(c, K, lm)
            n = max(int(bm["len"][:, :R].max()), 0)  # (the one host read: the width of the result)
            seqs, lens, scores = bm["tokens"][:, :R, :n].clone(), bm["len"][:, :R].clone(), bm["scores"][:, :R].clone()
            if R == 1:
                seqs, lens, scores = seqs[:, 0], lens[:, 0], scores[:, 0]
            result = {"sequences": seqs, "lengths": lens, "sequences_scores": scores, "n_beams": bm["n"]}
            if lm is not None:
                for name, key in (("ctc_scores", "ctc"), ("lm_scores", "lm")):
                    part = bm[key][:, :R].clone()
                    result[name] = part[:, 0] if R == 1 else part
            if return_timestamps:
                nb = max(int(bm["len"][:, 0].max()), 0)
                if nb > CTC_MAX_LABELS:
                    raise ValueError(f"timestamps take a best sequence of at most {CTC_MAX_LABELS} tokens (tmi_ctc_viterbi), got {nb}")
                L = max(nb, 1)
                lab = bm["tokens"][:, 0, :L].clamp_min(0).contiguous()  # (past a length: never read)
                ll = bm["len"][:, 0].contiguous()
                st, en = torch.full((B, L), -1, **c["i32"]), torch.full((B, L), -1, **c["i32"])
                total, bad = torch.zeros(B, **c["f32"]), torch.zeros(B, **c["i32"])
                wsp = torch.empty(ops.ctc_workspace_elems(B, L, T), **c["i32"])
                ops.ctc_viterbi(c["logp"], lab, ll, c["frame_lens"], self.config.ctc_blank_id, st, en, total, bad, wsp)
                st, en = st[:, :nb], en[:, :nb]
                result.update(token_start_frames=st, token_end_frames=en, token_start_times=self._times(st),
                              token_end_times=self._times(en))
            return result

    @torch.no_grad()
    def evaluate(self, inputs, labels, label_lengths=None, attention_mask=None, return_items=False, num_beams=None,
                 lm=None, lm_alpha=0.5, lm_beta=0.0, edit_ops=False, confusion=False):
        """The CTC loss of one batch and the error rate of its greedy transcript, forward only.  ``labels`` integer
        [B, L_max] with ``label_lengths`` [B] (see ``check_ctc_args``).  Returns Python numbers, float64 on the host, so
        that shards add up: ``nll_sum`` over the feasible items, ``n_items``, ``n_infeasible`` (items with fewer frames than
        their labels need: nll = +inf); ``loss`` by ``ctc_loss_reduction`` as torch's ctc_loss - "sum": the sum of the
        items' nll, "mean": the mean of nll / max(L, 1) - in which an infeasible item counts +inf, or 0 with
        ``ctc_zero_infinity``; ``n_edits`` / ``n_ref_tokens`` / ``token_error_rate``: the Levenshtein distance of the greedy
        transcript to the labels, summed over the items, over the number of labels.  ``return_items`` adds the device
        tensors ``nll`` fp32 [B] (+inf where infeasible, whatever ``ctc_zero_infinity``), ``infeasible`` int32 [B],
        ``sequences`` / ``lengths`` of the greedy transcript.  ``num_beams`` in [2, 16]: ``n_edits`` / ``token_error_rate`` are
        those of the best sequence of the prefix beam search (``decode(num_beams=...)``) instead of the greedy transcript,
        and ``return_items`` adds its ``beam_sequences`` / ``beam_lengths``; everything else is as without it.  ``lm`` /
        ``lm_alpha`` / ``lm_beta`` (with ``num_beams`` >= 2) as in ``decode``: the best sequence is the fused search's.

        ``edit_ops=True``: the error counts come from ONE tmi_edit_distance launch (include/tethys_mi.h states the rule)
        on the device tensors the pass holds - the greedy tokens and lengths, or the beams' - so the B * T transcript
        tokens are not copied to the host, and the result gains ``n_sub`` / ``n_del`` / ``n_ins`` (which add up to
        ``n_edits``) and ``n_hyp_tokens``.  With ``num_beams`` it also gains ``n_oracle_edits`` / ``oracle_error_rate``: the
        per-item minimum of the distance over the ranks the search filled (``n_beams``), the error rate a perfect
        rescoring of the n-best list would reach.  At most 4096 frames.  False: the function as it was, the same path
        and the same keys.

        ``confusion=True`` (with ``edit_ops=True``): the launch is tmi_edit_align instead, with the same counts, and
        tmi_edit_confusion folds its steps on the device; the result gains ``confusion``, an int64 tensor [V + 1, V + 1] on
        the device - row = the label, column = the transcript's token, index V = none (deletions in column V, insertions
        in row V) - of every item's transcript, with ``num_beams`` of its best beam only.  The transcript tokens still do
        not go to the host.  Tables of batches add."""
        cfg = self.config
        confusion = check_ctc_confusion_args(cfg, confusion, edit_ops)
        K, _ = check_ctc_beam_args(cfg, num_beams)
        lm = check_ctc_lm_args(cfg, lm, lm_alpha, lm_beta, num_beams)
        if K > 1:
            self._check_beam_frames(inputs, "evaluate")
        with self._ctc_pass(inputs, labels, label_lengths, attention_mask) as c:
            B = c["B"]
            nll, bad = torch.zeros(B, **c["f32"]), torch.zeros(B, **c["i32"])
            ops.ctc_forward(c["logp"], c["labels"], c["label_lens"], c["frame_lens"], cfg.ctc_blank_id, nll, bad, False)
            g = self._greedy(c)
            # one copy of what the host needs: the tokens and lengths of the transcript, nll and the flags (with edit_ops
            # the tokens stay on the device)
            T = c["T"]
            o = 0 if edit_ops else B * T
            host = torch.cat(([] if edit_ops else [g["tokens"].reshape(-1)]) + [g["len"], bad, nll.view(torch.int32)]).cpu()
            tok = None if edit_ops else host[:o].view(B, T).numpy()
            hl, hbad = host[o:o + B].numpy(), host[o + B:o + 2 * B].numpy()
            hnll = host[o + 2 * B:].view(torch.float32).double().numpy()
            ok = hbad == 0
            lens, lab = c["label_lens_host"], c["labels_host"]
            nll_sum = float(hnll[ok].sum())
            item = np.where(ok, hnll, 0.0 if cfg.ctc_zero_infinity else np.inf)
            if cfg.ctc_loss_reduction == "mean":
                loss = float((item / np.maximum(lens, 1)).mean())
            else:
                loss = float(item.sum())
            result = {"nll_sum": nll_sum, "n_items": float(B), "n_infeasible": float((~ok).sum()), "loss": loss}
            if K > 1:
                bm = self._beam(c, K, lm)
            if edit_ops:
                hyp, hyp_lens = (bm["tokens"].view(B * K, T), bm["len"].view(-1)) if K > 1 else (g["tokens"], g["len"])
                if confusion:
                    edits, steps, n_steps = ops.edit_align(hyp, c["labels"], hyp_lens, c["label_lens"], R=K)
                    table = ops.edit_confusion(steps, n_steps, hyp, c["labels"], cfg.vocab_size, R=K, first_only=True)
                    result["confusion"] = table[:-1].view(cfg.vocab_size + 1, cfg.vocab_size + 1).long()
                else:
                    edits = ops.edit_distance(hyp, c["labels"], hyp_lens, c["label_lens"], R=K)
                if K > 1:
                    ranks = torch.arange(K, device=self.device)[None, :] < bm["n"][:, None]
                    counts = ops.edit_counts(edits, K, valid=ranks)
                else:
                    counts = ops.edit_counts(edits)
                keys = ("n_edits", "n_ref_tokens", "token_error_rate", "n_sub", "n_del", "n_ins", "n_hyp_tokens")
                result.update({k: counts[k] for k in keys + (("n_oracle_edits", "oracle_error_rate") if K > 1 else ())})
                hyp_len = bm["len"][:, 0] if K > 1 else None
            else:
                hyp_tok, hyp_len = tok, hl
                if K > 1:
                    bhost = torch.cat([bm["tokens"][:, 0].reshape(-1), bm["len"][:, 0]]).cpu()
                    hyp_tok, hyp_len = bhost[:B * T].view(B, T).numpy(), bhost[B * T:].numpy()
                n_edits = sum(edit_distance(hyp_tok[b, :hyp_len[b]], lab[b, :lens[b]]) for b in range(B))
                n_ref = int(lens.sum())
                result.update({"n_edits": float(n_edits), "n_ref_tokens": float(n_ref),
                               "token_error_rate": n_edits / n_ref if n_ref else float("nan")})
            if return_items:
                n = max(int(hl.max()), 0)
                result.update(nll=nll, infeasible=bad, sequences=g["tokens"][:, :n].clone(), lengths=g["len"])
                if K > 1:
                    nbm = max(int(hyp_len.max()), 0)
                    result.update(beam_sequences=bm["tokens"][:, 0, :nbm].clone(), beam_lengths=bm["len"][:, 0].clone())
        return result

    @torch.no_grad()
    def align(self, inputs, labels, label_lengths=None, attention_mask=None, return_states=False):
        """Forced alignment: the most probable CTC path that spells ``labels`` (tmi_ctc_viterbi; the tie rule is in
        include/tethys_mi.h).  -> ``token_start_frames`` / ``token_end_frames`` int32 [B, L_max] (the first frame a token's
        state holds and the last plus 1; -1 past ``label_lengths`` and for an item without a path), ``token_start_times`` /
        ``token_end_times`` float64 seconds, ``path_logprob`` fp32 [B] (-inf without a path), ``infeasible`` int32 [B];
        ``return_states`` adds ``states`` int32 [B, T]: the extended state (2 i + 1: token i, even: a blank) of every frame,
        -1 past the clip's frames.  At most 4096 frames."""
        with self._ctc_pass(inputs, labels, label_lengths, attention_mask) as c:
            B, T, L = c["B"], c["T"], c["labels"].shape[1]
            if T > CTC_MAX_FRAMES:
                raise ValueError(f"align takes at most {CTC_MAX_FRAMES} frames (tmi_ctc_viterbi), got {T}")
            st, en = torch.full((B, L), -1, **c["i32"]), torch.full((B, L), -1, **c["i32"])
            total, bad = torch.zeros(B, **c["f32"]), torch.zeros(B, **c["i32"])
            states = torch.full((B, T), -1, **c["i32"]) if return_states else None
            wsp = torch.empty(ops.ctc_workspace_elems(B, L, T), **c["i32"])
            ops.ctc_viterbi(c["logp"], c["labels"], c["label_lens"], c["frame_lens"], self.config.ctc_blank_id, st, en, total,
                            bad, wsp, states)
            st, en = st[:, :c["L_max"]], en[:, :c["L_max"]]  # (L_max == 0: the kernels were given one unused column)
            result = {"token_start_frames": st, "token_end_frames": en, "token_start_times": self._times(st),
                      "token_end_times": self._times(en), "path_logprob": total, "infeasible": bad}
            if return_states:
                result["states"] = states
        return result

    @torch.no_grad()
    def posteriors(self, inputs, labels, label_lengths=None, attention_mask=None, return_logit_grad=False,
                   return_states=False):
        """The CTC forward-backward pass over ALL paths that spell ``labels`` (tmi_ctc_posteriors in include/tethys_mi.h),
        where ``align`` returns the single best one.  -> ``nll`` fp32 [B] (+inf where infeasible, whatever
        ``ctc_zero_infinity``, as ``evaluate(return_items=True)``), ``infeasible`` int32 [B], ``symbol_posteriors`` fp32
        [B, T, V] (the probability that frame t emits symbol c; zeros past a clip's frames), ``token_expected_frames`` fp32
        [B, L_max] (the expected number of frames of each token; -1 past ``label_lengths``, 0 for an item without a path),
        ``token_center_frames`` fp32 [B, L_max] (the posterior mean frame of each token; -1 in the padding and for items
        without a path), ``token_center_times`` float64 seconds (centre x ``frame_seconds``, the convention of the start
        times; -1 likewise).  ``return_logit_grad`` adds ``logit_grad`` fp32 [B, T, V]: the gradient of the sum of the
        items' nll with respect to ``logits`` (softmax - posterior; zero past a clip and for infeasible items) - a result
        for inspection, nothing of the training state is read or written.  ``return_states`` adds ``state_posteriors`` fp32
        [B, T, 2 L_max + 1] over the extended states (zeros past a clip's frames and an item's states).  At most 4096
        frames."""
        if torch.is_tensor(inputs) and inputs.dim() == 2 and inputs.shape[1] >= 1:   # (before the pass: nothing runs)
            T = frame_lengths(self.config, [int(inputs.shape[1])])[0]
            if T > CTC_MAX_FRAMES:
                raise ValueError(f"posteriors takes at most {CTC_MAX_FRAMES} frames (tmi_ctc_posteriors), got {T}")
        with self._ctc_pass(inputs, labels, label_lengths, attention_mask) as c:
            B, T, V, L = c["B"], c["T"], c["V"], c["labels"].shape[1]
            nll, bad = torch.zeros(B, **c["f32"]), torch.zeros(B, **c["i32"])
            gamma = torch.zeros((B, T, 2 * L + 1), **c["f32"])   # (what the kernel leaves unwritten is pre-filled)
            occ = torch.zeros((B, T, V), **c["f32"])
            grad = torch.zeros((B, T, V), **c["f32"]) if return_logit_grad else None
            frames, center = torch.full((B, L), -1.0, **c["f32"]), torch.full((B, L), -1.0, **c["f32"])
            ops.ctc_posteriors(c["logp"], c["labels"], c["label_lens"], c["frame_lens"], self.config.ctc_blank_id, nll, bad,
                               gamma, occ, frames, center, grad, False)
            frames, center = frames[:, :c["L_max"]], center[:, :c["L_max"]]  # (L_max == 0: one unused column, as align)
            result = {"nll": nll, "infeasible": bad, "symbol_posteriors": occ, "token_expected_frames": frames,
                      "token_center_frames": center, "token_center_times": self._times(center)}
            if return_logit_grad:
                result["logit_grad"] = grad
            if return_states:
                result["state_posteriors"] = gamma[:, :, :2 * c["L_max"] + 1]
        return result

    # -- the head on cached features of the frozen encoder (the CTC probe) -------------------------------------------
    @torch.no_grad()
    def encode_features(self, inputs, attention_mask=None, layers=None):
        """The frozen encoder's output for ``head_step`` / ``fit_ctc_head`` / ``evaluate_features``: ``hidden`` [B, T, H] in
        the model's dtype, bit for bit ``forward_infer``'s ``last_hidden_state`` (the head is not run), and
        ``frame_lengths`` int32 [B] on the device (the row sums of ``attention_mask``, a binary prefix mask over frames as
        ``check_ctc_args`` takes it; T without one).  Cache it: the encoder does not change while the head is trained.
        ``layers="all"`` adds ``hidden_layers`` [K, B, T, H], K = num_hidden_layers + 1, in the model's dtype: slice k is bit
        for bit ``forward_infer(output_hidden_states=True)["hidden_states"][k]`` (the input of layer k; the last slice is
        ``hidden``) - what the calls take with a ``LayerMix``."""
        if layers not in (None, "all"):
            raise ValueError('layers must be None or "all"')
        if not torch.is_tensor(inputs) or inputs.dim() != 2 or inputs.dtype != torch.float32:
            raise TypeError("inputs must be float32 [B, T_in]")
        B, T, frame_lens, mask, _, _ = check_ctc_args(self.config, tuple(inputs.shape), None, None, attention_mask)
        audio = inputs.to(self.device).contiguous()
        inf = self._infer_prepare(B, inputs.shape[1])
        with self._inference(inf):
            key_bias = None if mask is None else ((1.0 - mask) * -10000.0).to(self.device)  # V:352-355, as forward_infer
            x, layer_inputs = self._infer_body(audio, inf, key_bias, layers == "all")
            hidden = x.view(B, T, self.config.hidden_size).clone()
        result = {"hidden": hidden, "frame_lengths": torch.from_numpy(frame_lens).to(self.device)}
        if layers == "all":
            result["hidden_layers"] = torch.stack(layer_inputs + [hidden])
        return result

    def _check_hidden(self, hidden, layer_mix=None):
        H = self.config.hidden_size
        if layer_mix is not None:
            if not torch.is_tensor(hidden) or hidden.dtype != self.dtype or hidden.dim() != 4 or hidden.stride(3) != 1:
                raise TypeError(f"with a layer mix hidden must be {self.dtype} [K, N, T, {H}] with unit column stride "
                                f"(encode_features(layers=\"all\"))")
            check_layer_mix_args(self.config, tuple(hidden.shape), hidden.dtype, layer_mix)
            if layer_mix.device != self.device:
                raise ValueError("the mix must live on the model's device")
            return hidden if hidden.device == self.device else hidden.to(self.device)
        if not torch.is_tensor(hidden) or hidden.dtype != self.dtype or hidden.dim() != 3 or hidden.shape[2] != H or \
                hidden.shape[0] < 1 or hidden.shape[1] < 1 or hidden.stride(2) != 1:
            raise TypeError(f"hidden must be {self.dtype} [N, T, {H}] with unit column stride (encode_features)")
        if hidden.shape[1] > CTC_MAX_FRAMES:
            raise ValueError(f"at most {CTC_MAX_FRAMES} frames per item (tmi_ctc_posteriors), got {hidden.shape[1]}")
        return hidden if hidden.device == self.device else hidden.to(self.device)

    def _ctc_head_buffers(self, kind, N, T, L):
        """The buffers of one cached-feature call, kept per (kind, N, T_max, L_max); at most 8 sets live."""
        key = (kind, N, T, L)
        ws = self._head_sets.get(key)
        if ws is None:
            V, H = self.config.vocab_size, self.config.hidden_size
            f32, i32 = dict(dtype=torch.float32, device=self.device), dict(dtype=torch.int32, device=self.device)
            # (what the kernels leave unwritten - frames past a clip - is zero from here on)
            ws = {"logp": torch.zeros((N, T, V), **f32), "nll": torch.zeros(N, **f32), "bad": torch.zeros(N, **i32)}
            if kind == "step":
                ws.update(grad=torch.zeros((N, T, V), **f32), occ=torch.zeros((N, T, V), **f32),
                          gamma=torch.zeros((N, T, 2 * L + 1), **f32), tok_frames=torch.zeros((N, L), **f32),
                          tok_center=torch.zeros((N, L), **f32),
                          bwd_ws=torch.empty(ops.ctc_head_workspace_elems(N, T, H, V), **f32))
            else:
                ws.update(argmax=torch.zeros((N, T), **i32), tokens=torch.zeros((N, T), **i32), start=torch.zeros((N, T), **i32),
                          end=torch.zeros((N, T), **i32), len=torch.zeros(N, **i32), best=torch.zeros(N, **f32))
            self._head_sets[key] = ws
            while len(self._head_sets) > 8:
                self._head_sets.pop(next(k for k in self._head_sets if k != key))
        return ws

    def _layer_mix_buffers(self, ws, kind, N, T, K):
        """What a call with a layer mix adds to its buffer set: the fp32 ``mixed`` [N, T, H] (zeros past a clip's frames) and,
        for a step, the weights and tmi_layer_mix_bwd's workspace."""
        V, H = self.config.vocab_size, self.config.hidden_size
        f32 = dict(dtype=torch.float32, device=self.device)
        if "mixed" not in ws:
            ws["mixed"] = torch.zeros((N, T, H), **f32)
        if kind == "step" and ws.get("mix_K") != K:
            ws.update(mix_K=K, mix_w=torch.zeros(K, **f32), mix_ws=torch.empty(ops.layer_mix_workspace_elems(N, T, H, V, K), **f32))
        return ws

    def _check_step_args(self, hidden, frame_lengths, labels, label_lengths, row_index, layer_mix=None):
        hidden = self._check_hidden(hidden, layer_mix)
        items = hidden if layer_mix is None else hidden[0]
        N = int(items.shape[0] if row_index is None else row_index.numel())
        T = int(items.shape[1])
        if not 1 <= N <= ctc_head_batch_limit(T):
            raise ValueError(f"one call takes 1 <= N <= {ctc_head_batch_limit(T)} items of {T} frames (65535 items, 2^22 frames)")
        for t, shape, w in ((frame_lengths, (N,), "frame_lengths"), (label_lengths, (N,), "label_lengths"), (row_index, (N,), "row_index")):
            if t is None and w == "row_index":
                continue
            if not torch.is_tensor(t) or t.dtype != torch.int32 or tuple(t.shape) != shape or t.device != self.device or \
                    not t.is_contiguous():
                raise TypeError(f"{w} must be a contiguous int32 tensor [N = {N}] on the model's device (by position in the call)")
        if not torch.is_tensor(labels) or labels.dtype != torch.int32 or labels.dim() != 2 or labels.shape[0] != N or \
                not 1 <= labels.shape[1] <= CTC_MAX_LABELS or labels.device != self.device or not labels.is_contiguous():
            raise TypeError(f"labels must be a contiguous int32 tensor [N = {N}, 1 <= L_max <= {CTC_MAX_LABELS}] on the model's device")
        return hidden, N, T, int(labels.shape[1])

    def _spec_masks(self, spec, ws, N, T, seed, step, counts=None):
        """The step's span masks, drawn into the buffer set by ONE tmi_spec_masks launch -> (time_bits, feat_bits), None
        where that mask is off.  ``counts`` int32 [N, 2]: where the set bits per item go (default: the set's own)."""
        H = self.config.hidden_size
        time_on, feat_on = check_spec_augment_args(spec, T, H)
        if "spec_counts" not in ws:
            i32 = dict(dtype=torch.int32, device=self.device)
            ws.update(spec_tb=torch.zeros((N, ops.spec_masks_words(T)), **i32), spec_fb=torch.zeros((N, ops.spec_masks_words(H)), **i32),
                      spec_counts=torch.zeros((N, 2), **i32))
        tb, fb = ws["spec_tb"] if time_on else None, ws["spec_fb"] if feat_on else None
        if time_on or feat_on:
            ops.spec_masks(N, T, H, tb, fb, ws["spec_counts"] if counts is None else counts, spec.mask_time_prob,
                           spec.mask_time_length, spec.mask_feature_prob, spec.mask_feature_length, spec_site_seed(seed, step))
        return tb, fb

    def _spec_intermediates(self, tb, fb, N, T):
        H = self.config.hidden_size
        off = lambda cols: torch.zeros((N, cols), dtype=torch.bool, device=self.device)
        return dict(time_mask=off(T) if tb is None else unpack_mask_bits(tb, T),
                    feature_mask=off(H) if fb is None else unpack_mask_bits(fb, H))

    def head_step(self, hidden, frame_lengths, labels, label_lengths, optimizer, row_index=None, dropout=None, seed=0, step=0,
                  return_intermediates=False, layer_mix=None, spec_augment=None, _spec_counts=None):
        """One training step of the HEAD (``lm_head``) on cached features ``hidden`` [N_src, T, H] of the frozen encoder
        (``encode_features``), in this order: tmi_ctc_head_fwd with the reference's Dropout (V:972; rate ``dropout``, None:
        ``config.hidden_dropout``) in front of the Dense layer; tmi_ctc_posteriors with zero_infinity on, so an infeasible
        item costs 0 and gives no gradient; tmi_ctc_head_bwd into the head's slice of ``arena.g`` with
        ``config.ctc_loss_reduction``; then ``optimizer``'s Adam (``optim.Adam`` defaults to the Keras epsilon) over that
        slice ONLY.  The encoder's parameters, their moments and the bf16 mirror outside the head are not touched; the
        mirror inside it is refreshed, so ``decode`` / ``evaluate`` see the trained head at once.  ``row_index`` int32
        device tensor [N]: item n of the step is ``hidden[row_index[n]]`` (the minibatch gather costs nothing extra);
        ``frame_lengths`` [N], ``labels`` [N, L_max] and ``label_lengths`` [N], int32 device tensors, are BY POSITION in
        the step.  Their values are not read back here (``check_ctc_head_args`` validates them on the host; the kernels
        clamp lengths and never dereference a symbol outside the row).  The mask of the step is that of dropout site
        SITE_CTC under (``seed``, ``step``), as every site of this project, keyed by the position n * T + t in the step.
        -> ``loss`` (before the update: the sum of the items' nll, or with "mean" the mean of nll / max(L, 1)) and
        ``n_infeasible`` as one-element device tensors, no read-back.  ``return_intermediates`` adds clones of the step's
        ``log_probs`` and ``logit_grad`` fp32 [N, T, V] (zeros past a clip's frames).

        ``layer_mix`` (a ``LayerMix``): ``hidden`` is the stacked layers [K, N_src, T, H] (``encode_features(layers="all")``)
        and the step trains the mix with the head: tmi_layer_mix_fwd gathers and mixes the layers into a cached fp32
        buffer BY POSITION; tmi_ctc_head_fwd (with the dropout, keyed by position as above), tmi_ctc_posteriors and
        tmi_ctc_head_bwd run on that buffer; tmi_layer_mix_bwd writes the gradient of the loss with respect to the mixing
        logits; then Adam over the head's slice, then Adam over the mix (``LayerMix.adam_step``).  Nothing else of the
        arena is written.  ``return_intermediates`` then adds ``layer_weights`` [K] (the softmax the step used),
        ``layer_logit_grad`` [K] and ``mixed`` fp32 [N, T, H].

        ``spec_augment`` (a ``SpecAugment``): the step first draws its span masks with ONE tmi_spec_masks launch (site
        SITE_SPEC under (``seed``, ``step``), keyed by the item's POSITION n in the step; drawn over all T frames whatever
        ``frame_lengths`` says) into bit buffers of the cached buffer set, and the three calls that read the features run in
        their masked forms (tmi_ctc_head_fwd_m, tmi_ctc_head_bwd_m and, with a mix, tmi_layer_mix_bwd_m): a masked frame or
        column of ``hidden`` - of ``mixed`` behind a mix, which masks every layer - is +0 in front of the Dropout.  No masked
        copy of the features is written.  ``return_intermediates`` then adds ``time_mask`` bool [N, T] and ``feature_mask``
        bool [N, H] (``spec_augment_masks`` gives the same bits).  With None every call and launch is the one it was."""
        cfg = self.config
        hidden, N, T, L = self._check_step_args(hidden, frame_lengths, labels, label_lengths, row_index, layer_mix)
        p = float(cfg.hidden_dropout if dropout is None else dropout)
        if not 0.0 <= p < 1.0:
            raise ValueError("dropout must be in [0, 1)")
        ws = self._ctc_head_buffers("step", N, T, L)
        site = (int(seed) + int(step) * 0x9E3779B97F4A7C15 + SITE_CTC * 0xD1B54A32D192ED03) & 0xFFFFFFFFFFFFFFFF
        a = self.arena
        tb = fb = None
        if spec_augment is not None:
            tb, fb = self._spec_masks(spec_augment, ws, N, T, seed, step, _spec_counts)
        if layer_mix is not None:
            out = self._mixed_head_step(hidden, frame_lengths, labels, label_lengths, optimizer, row_index, p, site, ws, N, T, L,
                                        return_intermediates, layer_mix, tb, fb)
            if return_intermediates and spec_augment is not None:
                out.update(self._spec_intermediates(tb, fb, N, T))
            return out
        ops.ctc_head_fwd(hidden, a.param("lm_head.kernel"), a.param("lm_head.bias"), frame_lengths, ws["logp"],
                         row_index=row_index, p=p, seed=site, time_bits=tb, feat_bits=fb)
        ops.ctc_posteriors(ws["logp"], labels, label_lengths, frame_lengths, cfg.ctc_blank_id, ws["nll"], ws["bad"], ws["gamma"],
                           ws["occ"], ws["tok_frames"], ws["tok_center"], ws["grad"], True)
        loss = torch.empty(1, dtype=torch.float32, device=self.device)
        n_bad = torch.empty(1, dtype=torch.int32, device=self.device)
        ops.ctc_head_bwd(hidden, frame_lengths, label_lengths, ws["grad"], ws["nll"], ws["bad"], a.grad("lm_head.kernel"),
                         a.grad("lm_head.bias"), loss, n_bad, ws["bwd_ws"], L, row_index=row_index, p=p, seed=site,
                         reduction=cfg.ctc_loss_reduction, time_bits=tb, feat_bits=fb)
        optimizer.iterations += 1
        optimizer._update(self, self.head_lo, self.head_hi, 1.0, False, 0)
        out = {"loss": loss, "n_infeasible": n_bad}
        if return_intermediates:
            out.update(log_probs=ws["logp"].clone(), logit_grad=ws["grad"].clone())
            if spec_augment is not None:
                out.update(self._spec_intermediates(tb, fb, N, T))
        return out

    def _mixed_head_step(self, layers, frame_lengths, labels, label_lengths, optimizer, row_index, p, site, ws, N, T, L,
                         return_intermediates, mix, tb=None, fb=None):
        """``head_step`` behind a layer mix (its docstring states the order)."""
        cfg, a = self.config, self.arena
        self._layer_mix_buffers(ws, "step", N, T, mix.num_layers)
        W, b = a.param("lm_head.kernel"), a.param("lm_head.bias")
        ops.layer_mix_fwd(layers, mix.logits, frame_lengths, ws["mixed"], row_index=row_index, w_out=ws["mix_w"])
        ops.ctc_head_fwd(ws["mixed"], W, b, frame_lengths, ws["logp"], p=p, seed=site, time_bits=tb, feat_bits=fb)
        ops.ctc_posteriors(ws["logp"], labels, label_lengths, frame_lengths, cfg.ctc_blank_id, ws["nll"], ws["bad"], ws["gamma"],
                           ws["occ"], ws["tok_frames"], ws["tok_center"], ws["grad"], True)
        loss = torch.empty(1, dtype=torch.float32, device=self.device)
        n_bad = torch.empty(1, dtype=torch.int32, device=self.device)
        ops.ctc_head_bwd(ws["mixed"], frame_lengths, label_lengths, ws["grad"], ws["nll"], ws["bad"], a.grad("lm_head.kernel"),
                         a.grad("lm_head.bias"), loss, n_bad, ws["bwd_ws"], L, p=p, seed=site, reduction=cfg.ctc_loss_reduction,
                         time_bits=tb, feat_bits=fb)
        ops.layer_mix_bwd(layers, mix.logits, frame_lengths, label_lengths, ws["grad"], ws["bad"], W, mix.grad, ws["mix_ws"], L,
                          row_index=row_index, p=p, seed=site, reduction=cfg.ctc_loss_reduction, time_bits=tb, feat_bits=fb)
        out = {"loss": loss, "n_infeasible": n_bad}
        if return_intermediates:
            out.update(log_probs=ws["logp"].clone(), logit_grad=ws["grad"].clone(), layer_weights=ws["mix_w"].clone(),
                       layer_logit_grad=mix.grad.clone(), mixed=ws["mixed"].clone())
        optimizer.iterations += 1
        optimizer._update(self, self.head_lo, self.head_hi, 1.0, False, 0)
        mix.adam_step(optimizer)
        return out

    @torch.no_grad()
    def evaluate_features(self, hidden, frame_lengths, labels, label_lengths=None, layer_mix=None):
        """``evaluate(edit_ops=True)`` on cached features ``hidden`` [N, T, H] (``encode_features``): tmi_ctc_head_fwd without
        dropout from the fp32 master weights, then tmi_ctc_forward, tmi_ctc_greedy and tmi_edit_distance, in pieces of at
        most 65535 items and 2^22 frames.  Arguments as ``check_ctc_head_args`` takes them.  -> Python numbers: ``nll_sum``,
        ``n_items``, ``n_infeasible``, ``loss`` (as ``evaluate``: by ``ctc_loss_reduction``, an infeasible item +inf, or 0
        with ``ctc_zero_infinity``), ``n_edits``, ``n_sub``, ``n_del``, ``n_ins``, ``n_ref_tokens``, ``n_hyp_tokens``,
        ``token_error_rate``.  On a bf16 model this differs from ``evaluate(inputs, ...)`` only by the latter's bf16
        rounding of ``lm_head`` (its GEMM reads the bf16 mirror; the head here reads the fp32 master in both precisions);
        on an fp32 model only by the order of the sums.  ``layer_mix``: ``hidden`` is the stacked layers [K, N, T, H] and
        the head reads tmi_layer_mix_fwd of them (the path of ``set_layer_mix``)."""
        cfg = self.config
        hidden = self._check_hidden(hidden, layer_mix)
        items_shape = tuple(hidden.shape) if layer_mix is None else tuple(hidden.shape[1:])
        N, T, fl, lab, lens = check_ctc_head_args(cfg, items_shape, hidden.dtype, frame_lengths, labels, label_lengths)
        L = lab.shape[1]
        a = self.arena
        nll_sum = item_sum = 0.0
        n_bad = 0
        counts = {k: 0.0 for k in ops.EDIT_COUNT_KEYS}
        step = ctc_head_batch_limit(T)
        for s in range(0, N, step):
            n = min(step, N - s)
            ws = self._ctc_head_buffers("eval", n, T, L)
            fl_d, lab_d = torch.from_numpy(fl[s:s + n]).to(self.device), torch.from_numpy(lab[s:s + n]).to(self.device)
            lens_d = torch.from_numpy(lens[s:s + n]).to(self.device)
            feats = hidden[s:s + n]
            if layer_mix is not None:
                feats = self._layer_mix_buffers(ws, "eval", n, T, layer_mix.num_layers)["mixed"]
                ops.layer_mix_fwd(hidden[:, s:s + n], layer_mix.logits, fl_d, feats)
            ops.ctc_head_fwd(feats, a.param("lm_head.kernel"), a.param("lm_head.bias"), fl_d, ws["logp"], argmax=ws["argmax"])
            ops.ctc_forward(ws["logp"], lab_d, lens_d, fl_d, cfg.ctc_blank_id, ws["nll"], ws["bad"], False)
            ops.ctc_greedy(ws["argmax"], ws["logp"], fl_d, cfg.ctc_blank_id, ws["tokens"], ws["len"], ws["start"], ws["end"],
                           ws["best"])
            edits = ops.edit_distance(ws["tokens"], lab_d, ws["len"], lens_d)
            c = ops.edit_counts(edits)
            for k in counts:
                counts[k] += c[k]
            host = torch.cat([ws["bad"], ws["nll"].view(torch.int32)]).cpu()
            hbad, hnll = host[:n].numpy(), host[n:].view(torch.float32).double().numpy()
            ok = hbad == 0
            nll_sum += float(hnll[ok].sum())
            n_bad += int((~ok).sum())
            item = np.where(ok, hnll, 0.0 if cfg.ctc_zero_infinity else np.inf)
            item_sum += float((item / np.maximum(lens[s:s + n], 1)).sum() if cfg.ctc_loss_reduction == "mean" else item.sum())
        counts = ops.finish_edit_counts(counts)
        result = {"nll_sum": nll_sum, "n_items": float(N), "n_infeasible": float(n_bad),
                  "loss": item_sum / N if cfg.ctc_loss_reduction == "mean" else item_sum}
        result.update({k: counts[k] for k in ("n_edits", "n_ref_tokens", "token_error_rate", "n_sub", "n_del", "n_ins", "n_hyp_tokens")})
        return result


def fit_ctc_head(model, hidden, frame_lengths, labels, label_lengths, epochs, batch_size, learning_rate=1e-3, seed=0,
                 eval_set=None, layer_mix=None, mix_learning_rate=None, spec_augment=None):
    """Train ``model``'s CTC head on cached features ``hidden`` [N, T, H] (``model.encode_features``) with
    ``frame_lengths`` [N], ``labels`` [N, L_max] and ``label_lengths`` [N] (``check_ctc_head_args``).  Every epoch draws one
    permutation from a host generator seeded with ``seed``, gathers the labels and the two lengths in that order on the
    host, uploads them and the permutation once, and runs one ``head_step`` per minibatch with a slice of the permutation
    as ``row_index``: ``hidden`` stays where it is.  The last batch may be short.  Adam with ``learning_rate`` and the Keras
    epsilon; the dropout rate is ``config.hidden_dropout``.  -> the history, one dict per epoch: ``epoch``, ``loss`` ("mean":
    the mean of the steps' losses weighted by their items; "sum": their sum; one read-back per epoch), ``n_infeasible``
    (over the epoch's steps) and, with ``eval_set`` = (hidden, frame_lengths, labels, label_lengths), ``eval_loss`` and
    ``eval_token_error_rate`` (``evaluate_features``).  ``layer_mix`` (a ``LayerMix``): ``hidden`` - and ``eval_set``'s - is
    the stacked layers [K, N, T, H], every step trains the mix with the head (``mix_learning_rate``: the mix's own Adam
    rate; None: ``learning_rate``), and every epoch's record gains ``layer_weights``, the K softmax weights after the epoch
    (the logits come back in the epoch's one read-back, with the loss).  ``spec_augment`` (a ``SpecAugment``): every step
    masks its features (``head_step``; the evaluation never does) and every epoch's record gains ``masked_frame_fraction``:
    the time mask's set bits over the epoch's items, divided by items x T (the masks are drawn over all T frames of an item,
    whatever its length); the steps' counts come back in the epoch's one read-back."""
    from . import optim
    feats = model._check_hidden(hidden, layer_mix)
    N, T, fl, lab, lens = check_ctc_head_args(model.config, tuple(feats.shape) if layer_mix is None else tuple(feats.shape[1:]),
                                              feats.dtype, frame_lengths, labels, label_lengths)
    if layer_mix is not None and mix_learning_rate is not None:
        layer_mix.learning_rate = float(mix_learning_rate)
    epochs, batch_size = int(epochs), int(batch_size)
    if epochs < 0 or not 1 <= batch_size <= ctc_head_batch_limit(T):
        raise ValueError(f"epochs >= 0 and 1 <= batch_size <= {ctc_head_batch_limit(T)}")
    if eval_set is not None and len(eval_set) != 4:
        raise ValueError("eval_set is (hidden, frame_lengths, labels, label_lengths)")
    if spec_augment is not None:
        check_spec_augment_args(spec_augment, T, model.config.hidden_size)
    mean = model.config.ctc_loss_reduction == "mean"
    opt = optim.Adam(learning_rate)
    rng = np.random.default_rng(seed)
    history, step = [], 0
    for epoch in range(epochs):
        perm = rng.permutation(N)
        idx = torch.from_numpy(perm.astype(np.int32)).to(model.device)
        fl_d = torch.from_numpy(np.ascontiguousarray(fl[perm])).to(model.device)
        lab_d = torch.from_numpy(np.ascontiguousarray(lab[perm])).to(model.device)
        lens_d = torch.from_numpy(np.ascontiguousarray(lens[perm])).to(model.device)
        losses, bad, rows = [], [], []
        counts = None if spec_augment is None else torch.zeros((N, 2), dtype=torch.int32, device=model.device)
        for s in range(0, N, batch_size):
            e = min(N, s + batch_size)
            if spec_augment is None:
                r = model.head_step(feats, fl_d[s:e], lab_d[s:e], lens_d[s:e], opt, row_index=idx[s:e], seed=seed, step=step,
                                    layer_mix=layer_mix)
            else:
                r = model.head_step(feats, fl_d[s:e], lab_d[s:e], lens_d[s:e], opt, row_index=idx[s:e], seed=seed, step=step,
                                    layer_mix=layer_mix, spec_augment=spec_augment, _spec_counts=counts[s:e])
            losses.append(r["loss"])
            bad.append(r["n_infeasible"])
            rows.append(e - s)
            step += 1
        w = torch.tensor(rows if mean else [1.0] * len(rows), dtype=torch.float64, device=model.device)
        total = (torch.cat(losses).double() * w).sum() / (w.sum() if mean else 1.0)
        back = [total.view(1), torch.cat(bad).sum().double().view(1)]
        if spec_augment is not None:
            back.append(counts[:, 0].sum().double().view(1))
        if layer_mix is not None:
            back.append(layer_mix.logits.double())
        host = torch.cat(back).cpu().tolist()
        rec = {"epoch": epoch, "loss": float(host[0]), "n_infeasible": int(host[1])}
        if spec_augment is not None:
            rec["masked_frame_fraction"] = float(host.pop(2)) / float(N * T)
        if layer_mix is not None:
            z = np.asarray(host[2:], dtype=np.float64)
            e = np.exp(z - z.max())
            rec["layer_weights"] = (e / e.sum()).tolist()
        if eval_set is not None:
            ev = model.evaluate_features(*eval_set, layer_mix=layer_mix)
            rec.update(eval_loss=ev["loss"], eval_token_error_rate=ev["token_error_rate"])
        history.append(rec)
    return history


# ---------------------------------------------------------------------------------------------------------------------
# Sequence classification (V:1004-1067): masked-mean pooling, Dense + tanh, Dropout, Dense.  Inference and evaluation on
# padded batches, and training of the HEAD alone on pooled features of the frozen encoder (a linear probe).  Encoder
# fine-tuning is not built.
CLS_MAX_ROWS = 65535    # tmi_cls_head_fwd / _bwd: rows per call
CLS_MAX_HIDDEN = 4096   # H, a multiple of 4
CLS_MAX_PROJ = 1024     # classifier_proj_size, even
CLS_MAX_LABELS = 1024   # num_labels


def check_classification_args(cfg: Wav2Vec2Config, inputs_shape, labels=None, attention_mask=None, top_k=(1,)):
    """Host validation of ``Wav2Vec2ForSequenceClassification``'s calls (no GPU needed; the kernels cannot see values in
    device memory).  ``inputs_shape`` (B, T_in) of the audio - or (N, H) of pooled features, ``T_in`` then unused by the
    caller; 1 <= B <= 65535; the config inside the head kernels' limits (hidden_size a multiple of 4 and <= 4096,
    classifier_proj_size even and <= 1024, 1 <= num_labels <= 1024); ``labels`` None or B integers (tensor, array or list) -
    when they are on the host every one in [-1, num_labels), -1 meaning "unlabelled"; ``attention_mask`` None or [B, T]
    over frames (``frame_attention_mask``); ``top_k`` integers in [1, num_labels], no duplicates.
    -> (B, T, labels as a contiguous int32 tensor on the device they came from or None, top_k as a tuple)."""
    def integer(v):
        return isinstance(v, (int, np.integer)) and not isinstance(v, bool)
    H, P, C = cfg.hidden_size, cfg.classifier_proj_size, cfg.num_labels
    if not (integer(C) and 1 <= C <= CLS_MAX_LABELS):
        raise ValueError(f"num_labels must be an integer in [1, {CLS_MAX_LABELS}] (tmi_cls_head_fwd)")
    if not (integer(P) and 2 <= P <= CLS_MAX_PROJ and P % 2 == 0):
        raise ValueError(f"classifier_proj_size must be even and in [2, {CLS_MAX_PROJ}] (the dropout generator draws per column pair)")
    if not (4 <= H <= CLS_MAX_HIDDEN and H % 4 == 0):
        raise ValueError(f"hidden_size must be a multiple of 4 and <= {CLS_MAX_HIDDEN} (tmi_cls_head_fwd)")
    if len(inputs_shape) != 2 or int(inputs_shape[0]) < 1 or int(inputs_shape[1]) < 1:
        raise ValueError("inputs must be [B, T_in]")
    B, T_in = int(inputs_shape[0]), int(inputs_shape[1])
    if B > CLS_MAX_ROWS:
        raise ValueError(f"at most {CLS_MAX_ROWS} rows per call (tmi_cls_head_fwd)")
    T = frame_lengths(cfg, [T_in])[0]
    if attention_mask is not None:
        m = torch.as_tensor(attention_mask)
        if m.dim() != 2 or tuple(m.shape) != (B, T):
            raise ValueError(f"attention_mask must be [B, T] over frames = [{B}, {T}] (frame_attention_mask), got {list(m.shape)}")
    lab = None
    if labels is not None:
        lab = labels if torch.is_tensor(labels) else torch.as_tensor(np.asarray(labels))
        if lab.dtype not in (torch.int32, torch.int64) or lab.dim() != 1 or lab.shape[0] != B:
            raise ValueError(f"labels must be B = {B} integers (int32 or int64)")
        if lab.device.type == "cpu" and B and (int(lab.min()) < -1 or int(lab.max()) >= C):
            raise ValueError(f"labels must be in [-1, {C}): a class, or -1 for an unlabelled item")
        lab = lab.detach().to(torch.int32).contiguous()
    ks = tuple(top_k) if isinstance(top_k, (tuple, list)) else (top_k,)
    if not ks or any(not integer(k) or not 1 <= k <= C for k in ks) or len(set(ks)) != len(ks):
        raise ValueError(f"top_k must be distinct integers in [1, num_labels = {C}]")
    return B, T, lab, tuple(int(k) for k in ks)


class Wav2Vec2ForSequenceClassification(Wav2Vec2ForPreTraining):
    """V:1004-1067: the base model (the blocks and the inference workspace of ``Wav2Vec2ForPreTraining``), the masked mean
    over time (tmi_masked_mean_pool) and the head classifier_proj (Dense + tanh) -> Dropout -> classifier (Dense) on the
    kernels of csrc/cls_head.hip.  The head runs in fp32 from the arena's master weights in both precisions: the pooled
    vector is fp32 already.  Inference and ``evaluate`` run under ``torch.no_grad()`` on the inference workspace with
    dropout off; ``head_step`` / ``fit_head`` train the HEAD on pooled features of the frozen encoder and touch nothing of
    the arena outside the head's slice.  Encoder fine-tuning is not built: the training entry points raise.  Not built
    either: ``use_weighted_layer_sum``, class weights, the x-vector model."""

    _arena_head = "classification"

    def __init__(self, config: Wav2Vec2Config, device="cuda:0", precision: str = "bf16", seed: int = 1234):
        check_classification_args(config, (1, 1))
        super().__init__(config, device=device, precision=precision, seed=seed)
        a = self.arena
        self.head_lo, self.head_hi = a.offsets["classifier_proj.kernel"], a.numel  # the head: the arena's contiguous tail
        self._head_call = None
        self._head_sets: Dict[int, Dict[str, torch.Tensor]] = {}

    def forward_backward(self, *a, **k):
        raise NotImplementedError("encoder fine-tuning is not built")

    def __call__(self, inputs, attention_mask=None, labels=None, output_hidden_states=False, output_attentions=False,
                 training=False, **kw):
        """``model(inputs, attention_mask=None, labels=None, ...)`` is ``forward_infer``; ``training=True`` raises (the head
        alone is trained, on pooled features: ``head_step``)."""
        if training:
            raise NotImplementedError("encoder fine-tuning is not built")
        return self.forward_infer(inputs, attention_mask=attention_mask, labels=labels, output_hidden_states=output_hidden_states,
                                  output_attentions=output_attentions, **kw)

    # -- the head ----------------------------------------------------------------------------------------------------
    def _head_params(self):
        a = self.arena
        return (a.param("classifier_proj.kernel"), a.param("classifier_proj.bias"), a.param("classifier.kernel"),
                a.param("classifier.bias"))

    def _head_buffers(self, N, store=None):
        """The head's outputs for ``N`` rows: in the inference workspace (``store`` None) or in a set of their own."""
        cfg = self.config
        if store is None:
            saved = None
            ws = self.ws
        else:
            saved, self.ws = self.ws, store
            ws = store
        try:
            if "cls_logits" not in ws or ws["cls_logits"].shape[0] != N:
                f32, i32 = torch.float32, torch.int32
                self._buf("cls_logits", (N, cfg.num_labels), f32)
                self._buf("cls_logp", (N, cfg.num_labels), f32)
                self._buf("cls_pred", (N,), i32)
                self._buf("cls_nll", (N,), f32)
                self._buf("cls_rank", (N,), i32)
        finally:
            if saved is not None:
                self.ws = saved
        return ws

    def _head_fwd(self, pooled, N, ws, labels=None, confusion=None, row_index=None, p=0.0, seed=0, z=None):
        Wp, bp, Wc, bc = self._head_params()
        ops.cls_head_fwd(pooled, Wp, bp, Wc, bc, ws["cls_logits"], ws["cls_pred"], N=N, row_index=row_index, labels=labels,
                         p=p, seed=seed, z=z, log_probs=ws["cls_logp"], nll=ws["cls_nll"], label_rank=ws["cls_rank"],
                         confusion=confusion)

    def _infer_head(self, x, inf, result):
        call = self._head_call
        if call is None or call.get("skip"):
            return
        B = inf["key"][0]
        ws = self._head_buffers(B)
        labels = call.get("labels")
        self._head_fwd(result["pooled_output"], B, ws, labels=labels, confusion=call.get("confusion"))
        result["logits"] = ws["cls_logits"].clone()
        result["log_probs"] = ws["cls_logp"].clone()
        result["predictions"] = ws["cls_pred"].clone()
        if labels is not None:
            result["nll"] = ws["cls_nll"].clone()
            result["label_rank"] = ws["cls_rank"].clone()

    @torch.no_grad()
    def forward_infer(self, inputs, attention_mask=None, labels=None, output_hidden_states=False, output_attentions=False,
                      attentions_dtype=None, pool="mean", _confusion=None):
        """V:1017-1067 with training=False: the base model's outputs (``Wav2Vec2ForPreTraining.forward_infer``, always with
        ``pool="mean"``: ``pooled_output`` fp32 [B, H] is bit for bit what that call gives) plus ``logits`` fp32 [B, C],
        ``log_probs`` fp32 [B, C], ``predictions`` int32 [B] (the argmax, the lowest index on ties).  ``attention_mask`` is
        the frame mask of ``frame_attention_mask``.  With ``labels`` (B integers in [0, C), or -1: unlabelled) also ``nll``
        fp32 [B] and ``label_rank`` int32 [B] per item, and ``loss``: the mean of the sparse categorical cross-entropy
        over the labelled items, a one-element device tensor (V:1053-1056).  The reference computes the loss only in
        training; here it is computed whenever labels are given.  No dropout."""
        if pool != "mean":
            raise ValueError('the classification model pools with "mean"')
        if not torch.is_tensor(inputs) or inputs.dim() != 2:
            raise TypeError("inputs must be float32 [B, T_in]")
        B, _, lab, _ = check_classification_args(self.config, tuple(inputs.shape), labels, attention_mask)
        lab_dev = None if lab is None else lab.to(self.device)
        self._head_call = {"labels": lab_dev, "confusion": _confusion}
        try:
            result = super().forward_infer(inputs, attention_mask=attention_mask, output_hidden_states=output_hidden_states,
                                           pool="mean", output_attentions=output_attentions, attentions_dtype=attentions_dtype)
        finally:
            self._head_call = None
        if lab_dev is not None:
            n = ((lab_dev >= 0) & (lab_dev < self.config.num_labels)).sum().clamp(min=1).to(torch.float32).view(1)
            loss = torch.empty(1, dtype=torch.float32, device=self.device)
            ops.sum_scale_dev(result["nll"], loss, B, 1.0 / n)  # (unlabelled items hold 0)
            result["loss"] = loss
        return result

    @torch.no_grad()
    def pool_features(self, inputs, attention_mask=None):
        """The frozen encoder's pooled output fp32 [B, H] (``forward_infer``'s ``pooled_output``, the head not run): what
        ``head_step`` / ``fit_head`` train on.  Cache it: the encoder does not change while the head is trained."""
        self._head_call = {"skip": True}
        try:
            return super().forward_infer(inputs, attention_mask=attention_mask, pool="mean")["pooled_output"]
        finally:
            self._head_call = None

    @staticmethod
    def _score_sums(nll, rank, top_k):
        """-> [nll_sum, n_items, n_correct, topk_correct per k] as one float64 device vector (a few torch reductions over
        [B] ahead of the call's one read-back, as ``ops.edit_counts``)."""
        valid = rank >= 0
        parts = [nll.double().sum(), valid.sum().double(), (rank == 0).sum().double()]
        parts += [(valid & (rank < k)).sum().double() for k in top_k]
        return torch.stack(parts)

    @staticmethod
    def _finish_scores(sums, top_k):
        s = [float(v) for v in sums.cpu().tolist()]
        n = s[1]
        out = {"n_items": int(n), "nll_sum": s[0], "loss": s[0] / n if n else 0.0, "n_correct": int(s[2]),
               "accuracy": s[2] / n if n else 0.0, "topk_correct": {k: int(v) for k, v in zip(top_k, s[3:])}}
        out["topk_accuracy"] = {k: (v / n if n else 0.0) for k, v in out["topk_correct"].items()}
        return out

    def _confusion_arg(self, confusion):
        C = self.config.num_labels
        if confusion is None or confusion is False:
            return None
        if confusion is True:
            return torch.zeros((C, C), dtype=torch.int64, device=self.device)
        if not torch.is_tensor(confusion) or confusion.dtype != torch.int64 or tuple(confusion.shape) != (C, C) or \
                confusion.device != self.device or not confusion.is_contiguous():
            raise ValueError(f"confusion must be a bool or the previous int64 [{C}, {C}] table on the model's device")
        return confusion

    @torch.no_grad()
    def evaluate(self, inputs, labels, attention_mask=None, top_k=(1,), return_items=False, confusion=False):
        """Classification metrics of one batch, forward only (``forward_infer``: inference workspace, dropout off).
        ``labels`` B integers in [0, C), or -1 for an unlabelled item: it is scored 0 and counted nowhere.  Returns Python
        numbers from ONE read-back of the sums: ``n_items`` (labelled), ``nll_sum``, ``loss`` = nll_sum / n_items,
        ``n_correct``, ``accuracy``, ``topk_correct`` / ``topk_accuracy`` {k: ...} for every k of ``top_k`` - an item is in
        the top k when its ``label_rank`` (tmi_cls_head_fwd: the classes that beat the label) is < k, so no sort runs.
        ``confusion`` True: also ``confusion``, an int64 [C, C] device table, label by prediction; pass the previous
        call's table instead of True and this batch is ADDED to it on the device.  ``return_items``: the device tensors
        ``nll`` fp32, ``predictions`` and ``label_rank`` int32 [B]."""
        if labels is None:
            raise ValueError("evaluate takes labels")
        if not torch.is_tensor(inputs) or inputs.dim() != 2:
            raise TypeError("inputs must be float32 [B, T_in]")
        _, _, _, ks = check_classification_args(self.config, tuple(inputs.shape), labels, attention_mask, top_k)
        table = self._confusion_arg(confusion)
        r = self.forward_infer(inputs, attention_mask=attention_mask, labels=labels, _confusion=table)
        out = self._finish_scores(self._score_sums(r["nll"], r["label_rank"], ks), ks)
        if table is not None:
            out["confusion"] = table
        if return_items:
            out.update(nll=r["nll"], predictions=r["predictions"], label_rank=r["label_rank"])
        return out

    @torch.no_grad()
    def evaluate_features(self, pooled, labels, top_k=(1,), confusion=False):
        """``evaluate`` on cached pooled features fp32 [N, H] (``pool_features``): the head alone, dropout off, in pieces of
        at most 65535 rows.  Same result keys, without the per-item tensors."""
        pooled = self._check_pooled(pooled)
        N = pooled.shape[0]
        _, _, lab, ks = check_classification_args(self.config, (min(N, CLS_MAX_ROWS), 1), None, None, top_k)
        lab = torch.as_tensor(labels) if not torch.is_tensor(labels) else labels
        if lab.dim() != 1 or lab.shape[0] != N or lab.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"labels must be N = {N} integers")
        lab = lab.to(self.device, torch.int32).contiguous()
        table = self._confusion_arg(confusion)
        total = None
        for s in range(0, N, CLS_MAX_ROWS):
            n = min(CLS_MAX_ROWS, N - s)
            ws = self._head_buffers(n, self._head_sets.setdefault(("eval", n), {}))
            self._head_fwd(pooled[s:s + n], n, ws, labels=lab[s:s + n], confusion=table)
            sums = self._score_sums(ws["cls_nll"], ws["cls_rank"], ks)
            total = sums if total is None else total + sums
        out = self._finish_scores(total, ks)
        if table is not None:
            out["confusion"] = table
        return out

    def _check_pooled(self, pooled):
        H = self.config.hidden_size
        if not torch.is_tensor(pooled) or pooled.dtype != torch.float32 or pooled.dim() != 2 or pooled.shape[1] != H or \
                pooled.shape[0] < 1 or pooled.stride(1) != 1:
            raise TypeError(f"pooled features must be float32 [N, {H}] with unit column stride")
        return pooled if pooled.device == self.device else pooled.to(self.device)

    # -- training of the head on cached features (the linear probe) --------------------------------------------------
    def head_step(self, pooled, labels, optimizer, row_index=None, dropout=None, seed=0, step=0):
        """One training step of the HEAD on pooled features ``pooled`` fp32 [N_src, H] of the frozen encoder: forward with
        Dropout (V:1046; rate ``dropout``, None: ``config.hidden_dropout``), backward into the head's slice of ``arena.g``
        (tmi_cls_head_fwd / _bwd), then ``optimizer``'s Adam (tmi_adam_step; ``optim.Adam`` defaults to the Keras
        epsilon) over that slice ONLY.  The encoder's parameters, their moments and the bf16 mirror outside the head are
        not touched.  ``row_index`` int32 device tensor [N]: row r of the step is ``pooled[row_index[r]]`` (the minibatch
        gather costs nothing extra); ``labels`` int32 device tensor [N] BY POSITION in the step (-1: unlabelled).  The
        mask of the step is that of dropout site SITE_CLS under (``seed``, ``step``), as every site of this project.
        -> the mean loss over the labelled rows before the update, a one-element device tensor (no read-back)."""
        cfg = self.config
        pooled = self._check_pooled(pooled)
        N = int(pooled.shape[0] if row_index is None else row_index.numel())
        if not 1 <= N <= CLS_MAX_ROWS:
            raise ValueError(f"head_step takes 1 <= N <= {CLS_MAX_ROWS} rows")
        if not torch.is_tensor(labels) or labels.dtype != torch.int32 or labels.numel() != N or labels.device != self.device:
            raise TypeError("labels must be an int32 tensor [N] on the model's device (by position in the step)")
        if row_index is not None and (row_index.dtype != torch.int32 or row_index.device != self.device):
            raise TypeError("row_index must be an int32 tensor on the model's device")
        p = float(cfg.hidden_dropout if dropout is None else dropout)
        if not 0.0 <= p < 1.0:
            raise ValueError("dropout must be in [0, 1)")
        P, C = cfg.classifier_proj_size, cfg.num_labels
        ws = self._head_buffers(N, self._head_sets.setdefault(("step", N), {}))
        if "cls_z" not in ws:
            saved, self.ws = self.ws, ws
            try:
                self._buf("cls_z", (N, P), torch.float32)
                self._buf("cls_bwd_ws", (ops.cls_head_workspace_elems(N, cfg.hidden_size, P, C),), torch.float32)
            finally:
                self.ws = saved
        while len(self._head_sets) > 8:
            self._head_sets.pop(next(k for k in self._head_sets if self._head_sets[k] is not ws))
        site = (int(seed) + int(step) * 0x9E3779B97F4A7C15 + SITE_CLS * 0xD1B54A32D192ED03) & 0xFFFFFFFFFFFFFFFF
        a = self.arena
        self._head_fwd(pooled, N, ws, labels=labels, row_index=row_index, p=p, seed=site, z=ws["cls_z"])
        loss = torch.empty(1, dtype=torch.float32, device=self.device)
        ops.cls_head_bwd(pooled, a.param("classifier.kernel"), labels, ws["cls_z"], ws["cls_logp"],
                         a.grad("classifier_proj.kernel"), a.grad("classifier_proj.bias"), a.grad("classifier.kernel"),
                         a.grad("classifier.bias"), loss, ws["cls_bwd_ws"], N=N, row_index=row_index, p=p, seed=site)
        optimizer.iterations += 1
        optimizer._update(self, self.head_lo, self.head_hi, 1.0, False, 0)
        return loss


def fit_head(model, features, labels, epochs, batch_size, learning_rate=1e-3, seed=0, eval_features=None, eval_labels=None):
    """Train ``model``'s head (a linear probe) on cached pooled features ``features`` fp32 [N, H] with ``labels`` [N]
    integers (-1: unlabelled).  Every epoch draws one permutation from a host generator seeded with ``seed``, uploads it
    (and the labels in that order) once, and runs one ``head_step`` per minibatch with a slice of it as ``row_index``; the
    last batch may be short.  Adam with ``learning_rate`` and the Keras epsilon.  -> the history: one dict per epoch with
    ``epoch``, ``loss`` (the mean of the steps' losses weighted by their rows; one read-back per epoch) and, with
    ``eval_features`` / ``eval_labels``, ``eval_loss`` and ``eval_accuracy`` (``evaluate_features``)."""
    from . import optim
    feats = model._check_pooled(features)
    N = feats.shape[0]
    lab = np.asarray(torch.as_tensor(labels).detach().cpu().numpy()).astype(np.int64).reshape(-1)
    C = model.config.num_labels
    if lab.shape[0] != N or (lab < -1).any() or (lab >= C).any():
        raise ValueError(f"labels must be N = {N} integers in [-1, {C})")
    epochs, batch_size = int(epochs), int(batch_size)
    if epochs < 0 or not 1 <= batch_size <= CLS_MAX_ROWS:
        raise ValueError(f"epochs >= 0 and 1 <= batch_size <= {CLS_MAX_ROWS}")
    if (eval_features is None) != (eval_labels is None):
        raise ValueError("eval_features and eval_labels come together")
    opt = optim.Adam(learning_rate)
    rng = np.random.default_rng(seed)
    history, step = [], 0
    for epoch in range(epochs):
        perm = rng.permutation(N)
        idx = torch.from_numpy(perm.astype(np.int32)).to(model.device)
        lab_dev = torch.from_numpy(lab[perm].astype(np.int32)).to(model.device)
        losses, rows = [], []
        for s in range(0, N, batch_size):
            e = min(N, s + batch_size)
            losses.append(model.head_step(feats, lab_dev[s:e], opt, row_index=idx[s:e], seed=seed, step=step))
            rows.append(e - s)
            step += 1
        w = torch.tensor(rows, dtype=torch.float64, device=model.device)
        rec = {"epoch": epoch, "loss": float((torch.cat(losses).double() * w).sum() / w.sum())}
        if eval_features is not None:
            ev = model.evaluate_features(eval_features, eval_labels)
            rec.update(eval_loss=ev["loss"], eval_accuracy=ev["accuracy"])
        history.append(rec)
    return history


def create_classification_model(model_size: str = "small", num_labels: int = 2, device="cuda:0", precision: str = "bf16",
                                seed: int = 1234, **overrides):
    """Wav2Vec2ForSequenceClassification (V:1004-1067) of ``model_size`` with ``num_labels`` classes.  A factory of its own:
    ``create_full_model`` keeps the two types it has (a test pins its refusal of the others)."""
    cfg = make_config(model_size, num_labels=num_labels, **overrides)
    return Wav2Vec2ForSequenceClassification(cfg, device=device, precision=precision, seed=seed)


def load_pretrained_encoder(model, path):
    """Copy into ``model`` (a Wav2Vec2ForCTC or a Wav2Vec2ForSequenceClassification) every reference-keyed tensor of a
    ``train.save_weights`` file of a pre-training model that the model also has: the whole base model.  The head keeps its initialisation, the file's quantiser and
    projection heads are ignored, the bf16 mirror is re-derived.  Raises if a shared name has another shape or the file
    shares nothing.  -> the names copied."""
    ck = torch.load(path, map_location="cpu")
    if not isinstance(ck, dict) or "p" in ck:
        raise ValueError("load_pretrained_encoder takes a save_weights file (reference-keyed tensors)")
    views = model.arena.ref_views(model.arena.p)
    heads = ("lm_head.", "classifier_proj.", "classifier.")  # a head of the model's own: absent from a pre-training file
    shared = [k for k in views if k in ck and not k.startswith(heads)]
    if not shared:
        raise ValueError("the file shares no parameter with the model")
    for k in shared:
        if tuple(ck[k].shape) != tuple(views[k].shape):
            raise ValueError(f"{k}: the file has shape {tuple(ck[k].shape)}, the model {tuple(views[k].shape)}")
    missing = [k for k in views if k not in ck and not k.startswith(heads)]
    if missing:
        raise ValueError(f"the file lacks base-model parameters: {missing[:4]} ...")
    if hasattr(model, "finish_late"):
        model.finish_late()
    for k in shared:
        views[k].copy_(ck[k].to(torch.float32))
    model.refresh_shadows()
    return shared


def create_full_model(model_type: str = "pretraining", model_size: str = "small", device="cuda:0",
                      precision: str = "bf16", seed: int = 1234, **overrides):
    """V:1157-1182: "pretraining" -> Wav2Vec2ForPreTraining (``main`` hard-codes it, V:1416: the type on the hot path),
    "asr" -> Wav2Vec2ForCTC (inference only).  The other two types of the reference are not built."""
    cfg = make_config(model_size, **overrides)
    if model_type == "pretraining":
        return Wav2Vec2ForPreTraining(cfg, device=device, precision=precision, seed=seed)
    if model_type == "asr":
        return Wav2Vec2ForCTC(cfg, device=device, precision=precision, seed=seed)
    raise NotImplementedError('only "pretraining" (Wav2Vec2ForPreTraining) and "asr" (Wav2Vec2ForCTC) are built')
