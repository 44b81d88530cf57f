"""Host-side operator wrappers: torch tensors in, C-ABI calls out.

Each function resolves pointers / element strides from torch tensors (device memory is
PyTorch's caching allocator: plumbing) and launches the HIP kernel on torch's current
stream.  Nothing here computes on the host or falls back to torch ops (``edit_counts`` alone sums the integer table of
``edit_distance`` with torch reductions on the device, ahead of its one read-back, and ``edit_alignment_items`` gathers the
tokens that ``edit_align``'s steps name ahead of its one).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch

from . import _lib
from ._lib import TMI_BF16, TMI_F32, AttnDesc, GemmDesc, check, lib


def dt(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return TMI_F32
    if t.dtype == torch.bfloat16:
        return TMI_BF16
    raise TypeError(f"unsupported dtype {t.dtype}")


_STREAM_OVERRIDE: Optional[int] = None


def stream() -> int:
    """hipStream_t every wrapper launches on: torch's current stream, unless a caller has pinned
    another one with ``set_stream`` (cheaper than switching torch's current stream per launch)."""
    return _STREAM_OVERRIDE if _STREAM_OVERRIDE is not None else torch.cuda.current_stream().cuda_stream


def set_stream(handle: Optional[int]) -> Optional[int]:
    """Pin (or, with None, unpin) the launch stream; returns the previous pin so callers can nest."""
    global _STREAM_OVERRIDE
    prev, _STREAM_OVERRIDE = _STREAM_OVERRIDE, handle
    return prev


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


class OpProfile:
    """bench.py's roofline probe: HIP events (recorded on the launch stream) around every wrapped launch,
    folded per kernel class together with the launch's ALGORITHMIC work (flop for the MFMA classes, bytes
    for the HBM classes).  Events are read out every ``flush_every`` records: with ~500 timing events
    outstanding the runtime stalls the stream for tens of milliseconds on a record."""

    def __init__(self, flush_every=160):
        self.records = []
        self.flush_every = flush_every
        self.acc = {}  # class -> [ms, work, launches]

    def add(self, cls, e0, e1, work):
        self.records.append((cls, e0, e1, work))
        if len(self.records) >= self.flush_every:
            self.flush()

    def flush(self):
        if not self.records:
            return
        torch.cuda.synchronize()
        for cls, a, b, w in self.records:
            t = self.acc.setdefault(cls, [0.0, 0.0, 0])
            t[0] += a.elapsed_time(b)
            t[1] += w
            t[2] += 1
        self.records = []

    def totals(self, cls="gemm"):
        self.flush()
        ms, work, n = self.acc.get(cls, [0.0, 0.0, 0])
        return ms, work, n


GemmProfile = OpProfile  # (earlier name)
PROFILE = None  # set to an OpProfile() to instrument


class _probe:
    """``with _probe(cls, work):`` times the launches inside it when a profile is installed."""
    __slots__ = ("cls", "work", "e0")

    def __init__(self, cls, work):
        self.cls, self.work, self.e0 = cls, work, None

    def __enter__(self):
        if PROFILE is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e0.record()
        return self

    def __exit__(self, *exc):
        if self.e0 is not None and PROFILE is not None:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            PROFILE.add(self.cls, self.e0, e1, self.work)
        return False


_WORKSPACE = {}
GEMM_WORKSPACE_BYTES = 96 << 20  # TMI_GEMM_WORKSPACE_MIN


def gemm_workspace(device):
    """Split-K scratch of tmi_gemm (one fp32 slab per split): one per (device, stream), since calls
    that share it must be ordered on one stream."""
    key = (device.type, device.index, stream())  # one per stream in use
    ws = _WORKSPACE.get(key)
    if ws is None:
        ws = _WORKSPACE[key] = torch.empty(GEMM_WORKSPACE_BYTES, dtype=torch.uint8, device=device)  # contents irrelevant
    return ws


_GEMM_DESCS = {}   # call-site key -> (descriptor, byref): a step repeats the same ~150 launches with the same pointers and shapes


def gemm(A, B, Cm, M, N, K, a_sm, a_sk, b_sk, b_sn, ldc, *, nbatch=1, a_sb=0, b_sb=0, c_sb=0,
         kbatch=1, a_skb=0, b_skb=0, bias=None, bias_sb=0, scale_cols=0, scale=1.0, accumulate=False,
         act=0, aux_out=None, aux_in=None, resid=None, r_ld=0, r_sb=0, splitk=1,
         a_off=0, b_off=0, c_off=0, dropout_p=0.0, dropout_seed=0, nbatch2=1, a_sb2=0, b_sb2=0, c_sb2=0):
    """C = epi(A·B); see tmi_gemm in include/tethys_mi.h.  ``*_off`` are element offsets
    added to the tensors' base pointers (aux_* share c_off).  ``nbatch2`` / ``*_sb2``: an outer batch level.
    The descriptor is a pure function of the arguments (only the dropout seed changes from step to step), so it is built
    once per distinct call and reused: filling 45 ctypes fields cost more host time than the launch itself (round 4)."""
    ws = gemm_workspace(Cm.device) if (splitk == 0 and Cm.is_cuda) else None
    key = (A.data_ptr(), B.data_ptr(), Cm.data_ptr(), M, N, K, a_sm, a_sk, b_sk, b_sn, ldc, nbatch, a_sb, b_sb, c_sb, kbatch, a_skb,
           b_skb, None if bias is None else bias.data_ptr(), bias_sb, scale_cols, scale, accumulate, act,
           None if aux_out is None else aux_out.data_ptr(), None if aux_in is None else aux_in.data_ptr(),
           None if resid is None else resid.data_ptr(), r_ld, r_sb, splitk, a_off, b_off, c_off, dropout_p, nbatch2, a_sb2, b_sb2,
           c_sb2, A.dtype, B.dtype, Cm.dtype, None if ws is None else ws.data_ptr())
    hit = _GEMM_DESCS.get(key)
    if hit is None:
        d = GemmDesc()
        esA, esC = A.element_size(), Cm.element_size()
        d.A = A.data_ptr() + a_off * esA
        d.B = B.data_ptr() + b_off * B.element_size()
        d.C = Cm.data_ptr() + c_off * esC
        d.M, d.N, d.K = M, N, K
        d.a_sm, d.a_sk, d.b_sk, d.b_sn, d.ldc = a_sm, a_sk, b_sk, b_sn, ldc
        d.nbatch, d.a_sb, d.b_sb, d.c_sb = nbatch, a_sb, b_sb, c_sb
        d.kbatch, d.a_skb, d.b_skb = kbatch, a_skb, b_skb
        d.bias = ptr(bias)
        d.bias_sb = bias_sb
        d.scale_cols, d.scale = scale_cols, scale
        d.accumulate = 1 if accumulate else 0
        d.act = act
        d.aux_out = None if aux_out is None else aux_out.data_ptr() + c_off * esC
        d.aux_in = None if aux_in is None else aux_in.data_ptr() + c_off * esC
        d.resid = ptr(resid)
        d.r_ld, d.r_sb = r_ld, r_sb
        d.splitk = splitk
        d.dropout_p = dropout_p
        d.nbatch2, d.a_sb2, d.b_sb2, d.c_sb2 = nbatch2, a_sb2, b_sb2, c_sb2
        if ws is not None:
            d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
        assert A.dtype == B.dtype
        d.in_dtype, d.out_dtype = dt(A), dt(Cm)
        if len(_GEMM_DESCS) > 8192:   # (ragged batches / many models in one process: start over rather than grow without bound)
            _GEMM_DESCS.clear()
        hit = _GEMM_DESCS[key] = (d, C.byref(d))
    d, ref = hit
    if dropout_p > 0.0:
        d.dropout_seed = dropout_seed
    if PROFILE is None:
        check(lib().tmi_gemm(ref, stream()), "tmi_gemm")
        return
    with _probe("gemm", 2.0 * M * N * K * max(1, nbatch) * max(1, kbatch) * max(1, nbatch2)):
        check(lib().tmi_gemm(ref, stream()), "tmi_gemm")


def linear(x2d, w, out, *, w_is_kn=True, **kw):
    """out[M,N] = x2d[M,K] @ W with W given as [K,N] row-major (Keras Dense kernel layout)
    when ``w_is_kn`` else as [N,K] row-major."""
    M, K = x2d.shape
    if w_is_kn:
        N = w.shape[1]
        b_sk, b_sn = w.stride(0), w.stride(1)
    else:
        N = w.shape[0]
        b_sk, b_sn = w.stride(1), w.stride(0)
    gemm(x2d, w, out, M, N, K, x2d.stride(0), x2d.stride(1), b_sk, b_sn, out.stride(0), **kw)


def layernorm_fwd(x2d, gamma, beta, y2d, mean, rstd, eps):
    with _probe("layernorm", 2.0 * x2d.numel() * x2d.element_size()):
        rows, Cn = x2d.shape
        check(lib().tmi_layernorm_fwd(x2d.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y2d.data_ptr(),
                                      mean.data_ptr(), rstd.data_ptr(), rows, Cn, eps, dt(x2d), stream()),
              "tmi_layernorm_fwd")


_LN_WS = {}
# tmi_layernorm_bwd's column sums: fp32 atomics (default) or per-workgroup partial rows in a workspace + a fixed-order
# fold launch (TMI_LN_DETERMINISTIC=1: bit-reproducible dgamma / dbeta / bias sums).  Measured on MI355X, round 3
# (profiles/r03_ln_bwd_forms.txt): the two forms take the same time alone (23-24 us at [12000, 768] bf16) AND beside the
# weight-gradient stream (88-108 us either way: the kernel is starved of CUs by the one-workgroup-per-CU GEMMs, it is
# not serialising on its atomics), and the extra launch per call costs the step 0.07-0.1 ms - so atomics stay the default.
LN_ATOMIC = os.environ.get("TMI_LN_DETERMINISTIC", "0") == "0"


def set_deterministic(on: bool) -> bool:
    """Reproducible reductions for the whole step (returns the previous setting): LayerNorm backward through its workspace +
    fixed-order fold, column sums with one workgroup per column group (tmi_set_deterministic).  Every other kernel of the
    Whisper step is order-independent already, so two runs of the same steps then agree bit for bit; costs ~0.1 ms/step."""
    global LN_ATOMIC
    was = not LN_ATOMIC
    LN_ATOMIC = not on
    lib().tmi_set_deterministic(1 if on else 0)
    return was


def ln_bwd_workspace(device, rows, C, emit):
    """Partial-sum table of tmi_layernorm_bwd (one row of 2-3 * C floats per workgroup): one per (device, stream) like the
    GEMM workspace - the fold launch that reads it follows on the same stream.  An outgrown buffer is parked, never
    returned to the allocator while queued kernels may read it (see attn_workspace)."""
    if LN_ATOMIC:
        return None
    need = int(lib().tmi_layernorm_bwd_workspace_bytes(rows, C, 1 if emit else 0))
    key = (device.type, device.index, stream())
    ws = _LN_WS.get(key)
    if ws is None or ws.numel() * 4 < need:
        if ws is not None:
            _ATTN_WS_RETIRED.append(ws)
        ws = _LN_WS[key] = torch.empty(max(need // 4, 1 << 20), dtype=torch.float32, device=device)
    return ws


def layernorm_dropout_fwd(x2d, gamma, beta, y2d, mean, rstd, eps, dropout_p, dropout_seed):
    """y = Dropout_p(LayerNorm(x)) in one pass (tmi_layernorm_dropout_fwd): the mask of ``dropout`` over the [rows, C] output."""
    with _probe("layernorm", 2.0 * x2d.numel() * x2d.element_size()):
        rows, Cn = x2d.shape
        check(lib().tmi_layernorm_dropout_fwd(x2d.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y2d.data_ptr(), mean.data_ptr(),
                                              rstd.data_ptr(), rows, Cn, eps, dropout_p, dropout_seed, dt(x2d), stream()),
              "tmi_layernorm_dropout_fwd")


def layernorm_dropout_bwd(dy2d, x2d, gamma, mean, rstd, dx2d, dgamma, dbeta, dropout_p, dropout_seed, accumulate_dx=False):
    """layernorm_bwd of a LayerNorm whose output went through Dropout: the same mask (same seed) applied to dy on load."""
    with _probe("layernorm", (4.0 if accumulate_dx else 3.0) * x2d.numel() * x2d.element_size()):
        rows, Cn = x2d.shape
        ws = ln_bwd_workspace(x2d.device, rows, Cn, False)
        check(lib().tmi_layernorm_dropout_bwd(dy2d.data_ptr(), x2d.data_ptr(), gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                              dx2d.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), rows, Cn,
                                              1 if accumulate_dx else 0, dropout_p, dropout_seed, ptr(ws),
                                              0 if ws is None else ws.numel() * 4, dt(x2d), stream()), "tmi_layernorm_dropout_bwd")


def layernorm_bwd(dy2d, x2d, gamma, mean, rstd, dx2d, dgamma, dbeta, accumulate_dx=False):
    """dgamma / dbeta are accumulated into: zero them first (the grad arena is)."""
    with _probe("layernorm", (4.0 if accumulate_dx else 3.0) * x2d.numel() * x2d.element_size()):
        rows, Cn = x2d.shape
        ws = ln_bwd_workspace(x2d.device, rows, Cn, False)
        check(lib().tmi_layernorm_bwd(dy2d.data_ptr(), x2d.data_ptr(), gamma.data_ptr(), mean.data_ptr(),
                                      rstd.data_ptr(), dx2d.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), rows, Cn,
                                      1 if accumulate_dx else 0, ptr(ws), 0 if ws is None else ws.numel() * 4, dt(x2d), stream()),
              "tmi_layernorm_bwd")


def layernorm_bwd_emit(dy2d, x2d, gamma, mean, rstd, dx2d, dgamma, dbeta, colsum, masked=None, dropout_p=0.0, dropout_seed=0,
                       accumulate_dx=False):
    """layernorm_bwd that also accumulates colsum[c] += sum_rows dy' and (with ``masked``) writes dy' = Dropout-mask(dx):
    what the Dense layer below needs of dx (tmi_layernorm_bwd_emit)."""
    es = x2d.element_size()
    work = ((4.0 if accumulate_dx else 3.0) + (1.0 if masked is not None and dropout_p > 0 else 0.0)) * x2d.numel() * es
    with _probe("layernorm", work):
        rows, Cn = x2d.shape
        ws = ln_bwd_workspace(x2d.device, rows, Cn, True)
        check(lib().tmi_layernorm_bwd_emit(dy2d.data_ptr(), x2d.data_ptr(), gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                           dx2d.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), rows, Cn,
                                           1 if accumulate_dx else 0, colsum.data_ptr(), ptr(masked), dropout_p, dropout_seed,
                                           ptr(ws), 0 if ws is None else ws.numel() * 4, dt(x2d), stream()), "tmi_layernorm_bwd_emit")


def bias_grad(dy2d, dbias):
    """dbias[N] += sum over rows of dy2d[rows, N] (atomics: zero dbias first)."""
    with _probe("colsum", 1.0 * dy2d.numel() * dy2d.element_size()):
        rows, N = dy2d.shape
        check(lib().tmi_colsum(dy2d.data_ptr(), dy2d.stride(0), dbias.data_ptr(), rows, N, dt(dy2d), stream()),
              "tmi_colsum")


def bias_grad_batched(dy3d, dbias, out_sb):
    """dy3d [L, rows, N] (constant layer stride) -> dbias + l * out_sb (elements) += column sums of dy3d[l], one launch."""
    with _probe("colsum", 1.0 * dy3d.numel() * dy3d.element_size()):
        L, rows, N = dy3d.shape
        check(lib().tmi_colsum_batched(dy3d.data_ptr(), dy3d.stride(1), dy3d.stride(0), dbias.data_ptr(), out_sb, rows, N, L,
                                       dt(dy3d), stream()), "tmi_colsum_batched")


def gelu_bwd(dy, u, dx):
    check(lib().tmi_gelu_bwd(dy.data_ptr(), u.data_ptr(), dx.data_ptr(), dy.numel(), dt(dy), stream()),
          "tmi_gelu_bwd")


def gelu_bwd_batched(dy, u, dx, n, nbatch, dy_sb, u_sb, dx_sb):
    """nbatch spans of n elements, batch strides in elements (tensors give the base pointers)."""
    check(lib().tmi_gelu_bwd_batched(dy.data_ptr(), u.data_ptr(), dx.data_ptr(), n, nbatch, dy_sb, u_sb, dx_sb, dt(dy),
                                     stream()), "tmi_gelu_bwd")


def softmax_fwd(s, rows, Tq, Tk, mask_mode):
    check(lib().tmi_softmax_fwd(s.data_ptr(), rows, Tq, Tk, mask_mode, stream()), "tmi_softmax_fwd")


def softmax_bias_fwd(s, rows, Tq, Tk, H, key_bias):
    """tmi_softmax_fwd with the additive key term ``key_bias`` fp32 [B, Tk] (row r belongs to batch r // (H * Tq))."""
    if key_bias.dtype != torch.float32 or key_bias.dim() != 2 or key_bias.shape[1] != Tk or key_bias.stride(1) != 1:
        raise ValueError("key_bias must be float32 [B, Tk] with contiguous rows")
    check(lib().tmi_softmax_bias_fwd(s.data_ptr(), rows, Tq, Tk, H, key_bias.data_ptr(), key_bias.stride(0), stream()),
          "tmi_softmax_bias_fwd")


def softmax_bwd(p, dp, rows, Tk):
    check(lib().tmi_softmax_bwd(p.data_ptr(), dp.data_ptr(), rows, Tk, stream()), "tmi_softmax_bwd")


_ATTN_WS = {}
_ATTN_WS_RETIRED = []


def attn_workspace(device, B, H, Tq):
    """Key-split scratch of tmi_attn_fwd / tmi_attn_bwd (cross-attention: one query tile against a long key side): one per
    (device, stream) like the GEMM workspace, grown to the largest (B, H, Tq) seen.  None when the shape never splits."""
    need = int(lib().tmi_attn_workspace_bytes(B, H, Tq))
    if need == 0:
        return None
    key = (device.type, device.index, stream())
    ws = _ATTN_WS.get(key)
    if ws is None or ws.numel() < need:
        # Kernels are launched on the ops-pinned stream, which is not torch's current stream, so the caching allocator
        # cannot know that a dropped buffer may still be read by queued key-split / combine kernels: a buffer that is
        # outgrown is parked (never handed back while the process lives; growth happens a handful of times per model)
        if ws is not None:
            _ATTN_WS_RETIRED.append(ws)
        ws = _ATTN_WS[key] = torch.empty(need, dtype=torch.uint8, device=device)
    return ws


def _attn_desc(q, k, v, o, stats, B, H, Tq, Tk, mask_mode, score_scale=1.0):
    """q,k,v,o: (tensor, element_offset, batch_stride, token_stride)."""
    d = AttnDesc()
    if mask_mode == 0 and Tq <= 128 and Tk >= 512:
        ws = attn_workspace(stats.device, B, H, Tq)
        if ws is not None:
            d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
    for name, (t, off, sb, st) in (("q", q), ("k", k), ("v", v), ("o", o)):
        setattr(d, name, t.data_ptr() + off * t.element_size())
        setattr(d, f"{name}_sb", sb)
        setattr(d, f"{name}_st", st)
    d.stats = stats.data_ptr()
    d.B, d.H, d.Tq, d.Tk = B, H, Tq, Tk
    d.mask_mode = mask_mode
    d.score_scale = score_scale
    return d


def attn_dropmask(device, B, H, Tq, Tk):
    """Buffer for the keep bits of one attention call with dropout (tmi_attn_desc.drop_mask): written by the forward, read by
    the backward of the same call, so the caller keeps one per dropout site from forward to backward."""
    return torch.empty(int(lib().tmi_attn_dropmask_bytes(B, H, Tq, Tk)), dtype=torch.uint8, device=device)


def _set_dropout(d, dropout_p, dropout_seed, drop_mask):
    d.dropout_p, d.dropout_seed = dropout_p, dropout_seed
    if dropout_p > 0.0:
        if drop_mask is None:
            raise ValueError("attention dropout needs a drop_mask buffer (ops.attn_dropmask): the forward stores the mask, "
                             "the backward reads it")
        d.drop_mask, d.drop_mask_bytes = drop_mask.data_ptr(), drop_mask.numel() * drop_mask.element_size()


def _set_key_bias(d, key_bias, B, Tk):
    if key_bias is None:
        return
    if key_bias.dtype != torch.float32 or key_bias.dim() != 2 or key_bias.shape != (B, Tk) or key_bias.stride(1) != 1:
        raise ValueError("key_bias must be float32 [B, Tk] with contiguous rows")
    d.key_bias, d.kb_sb = key_bias.data_ptr(), key_bias.stride(0)


def attn_fwd(q, k, v, o, stats, B, H, Tq, Tk, mask_mode=0, score_scale=1.0, dropout_p=0.0, dropout_seed=0, drop_mask=None,
             key_bias=None):
    """``key_bias`` (mask_mode 2): fp32 [B, Tk], added to the scores of key column j of batch b (natural-log units)."""
    with _probe("attention", 4.0 * B * H * Tq * Tk * 64):
        d = _attn_desc(q, k, v, o, stats, B, H, Tq, Tk, mask_mode, score_scale)
        _set_dropout(d, dropout_p, dropout_seed, drop_mask)
        _set_key_bias(d, key_bias, B, Tk)
        check(lib().tmi_attn_fwd(C.byref(d), stream()), "tmi_attn_fwd")


def attn_bwd(q, k, v, o, stats, do, dq, dk, dv, delta, B, H, Tq, Tk, mask_mode=0, dq_scale=1.0, score_scale=1.0,
             dropout_p=0.0, dropout_seed=0, passes=0, drop_mask=None):
    """``passes``: 0 both, 1 the dQ pass (fills ``delta``), 2 the dK/dV pass (needs ``delta`` from pass 1).
    ``drop_mask``: the buffer the forward of this call filled (dropout_p > 0)."""
    d = _attn_desc(q, k, v, o, stats, B, H, Tq, Tk, mask_mode, score_scale)
    _set_dropout(d, dropout_p, dropout_seed, drop_mask)
    d.bwd_passes = passes
    for name, field, (t, off, sb, st) in (("d_o", "do", do), ("dq", "dq", dq), ("dk", "dk", dk), ("dv", "dv", dv)):
        setattr(d, name, t.data_ptr() + off * t.element_size())
        setattr(d, f"{field}_sb", sb)
        setattr(d, f"{field}_st", st)
    d.delta = delta.data_ptr()
    d.dq_scale = dq_scale
    # algorithmic work as SURVEY 8(d) defines it: fwd + bwd = 3 x forward, i.e. backward = 2 x 4.B.H.Tq.Tk.64
    # (the two passes execute seven products: both recompute S and dP)
    # (3 of the 7 products are the dQ pass, 4 the dK/dV pass)
    with _probe("attention", 8.0 * B * H * Tq * Tk * 64 * (1.0 if passes in (0, 3) else (3.0 / 7.0 if passes == 1 else 4.0 / 7.0))):
        check(lib().tmi_attn_bwd(C.byref(d), stream()), "tmi_attn_bwd")


def attn_probs(q, k, stats, out, B, H, Tq, Tk, mask_mode=0, score_scale=1.0, key_bias=None):
    """The attention weights of the ``attn_fwd`` call that left ``stats`` (tmi_attn_probs): ``out`` fp32 or bf16 with
    ``out[b, h, q, key]`` at ``(b * H + h) * out.stride(1) + q * out.stride(2) + key`` (4-D, unit stride along the keys,
    ``stride(0) == H * stride(1)``); q, k as for ``attn_fwd``.  The probabilities before dropout."""
    if out.dim() != 4 or tuple(out.shape) != (B, H, Tq, Tk) or out.stride(3) != 1 or (B > 1 and out.stride(0) != H * out.stride(1)):
        raise ValueError("attn_probs: out must be [B, H, Tq, Tk] with unit key stride and stride(0) == H * stride(1)")
    d = _attn_desc(q, k, q, q, stats, B, H, Tq, Tk, mask_mode, score_scale)
    d.workspace, d.workspace_bytes = None, 0
    _set_key_bias(d, key_bias, B, Tk)
    check(lib().tmi_attn_probs(C.byref(d), out.data_ptr(), dt(out), out.stride(1), out.stride(2), stream()), "tmi_attn_probs")


def _i32_dev(t, n, what):
    if t.dtype != torch.int32 or not t.is_contiguous() or t.numel() < n:
        raise ValueError(f"{what} must be a contiguous int32 tensor of at least {n} entries")


def align_cost_tile(medfilt_width: int) -> int:
    """Output frames per workgroup of tmi_align_cost for this filter width."""
    n = int(lib().tmi_align_cost_tile(int(medfilt_width)))
    if n < 0:
        raise ValueError(f"medfilt_width must be odd in 1..9, got {medfilt_width}")
    return n


def align_cost(probs, rows, cols, head_weight, cost, medfilt_width=7, normalize=True, accumulate=False):
    """The DTW cost of one decoder layer's cross-attention weights (tmi_align_cost in include/tethys_mi.h): ``probs``
    [N, H, S, T] fp32 or bf16 with unit stride along T and ``stride(0) == H * stride(1)`` (a slice past the start token's
    row is fine), ``rows`` / ``cols`` int32 [N] on the device, ``head_weight`` fp32 [H] on the device (0: head skipped),
    ``cost`` fp32 [N, S, T] with unit stride along T; ``accumulate`` adds onto what ``cost`` holds."""
    if probs.dim() != 4 or probs.stride(3) != 1 or (probs.shape[0] > 1 and probs.stride(0) != probs.shape[1] * probs.stride(1)):
        raise ValueError("align_cost: probs must be [N, H, S, T] with unit frame stride and stride(0) == H * stride(1)")
    N, H, S, T = probs.shape
    if cost.dtype != torch.float32 or cost.dim() != 3 or tuple(cost.shape) != (N, S, T) or cost.stride(2) != 1:
        raise ValueError("align_cost: cost must be float32 [N, S, T] with unit frame stride")
    _i32_dev(rows, N, "align_cost: rows")
    _i32_dev(cols, N, "align_cost: cols")
    _f32_flat(head_weight, H, "align_cost: head_weight")
    with _probe("align_cost", 1.0 * N * H * S * T * probs.element_size()):
        check(lib().tmi_align_cost(probs.data_ptr(), dt(probs), probs.stride(1), probs.stride(2), rows.data_ptr(), cols.data_ptr(),
                                   head_weight.data_ptr(), cost.data_ptr(), cost.stride(0), cost.stride(1), N, H, S, T,
                                   int(medfilt_width), 1 if normalize else 0, 1 if accumulate else 0, stream()), "tmi_align_cost")


def dtw_workspace_elems(N: int, S_max: int, T_max: int) -> int:
    """int32 elements of tmi_dtw's workspace (tmi_dtw_workspace_bytes / 4)."""
    n = int(lib().tmi_dtw_workspace_bytes(N, S_max, T_max))
    if n < 0:
        raise ValueError(f"tmi_dtw takes 1 <= N <= 65535 items of at most 1024 rows x 4096 columns, got {N} x {S_max} x {T_max}")
    return n // 4


def dtw(cost, rows, cols, tok_start, tok_end, total, workspace, path=None, path_len=None):
    """Dynamic time warping over ``cost`` fp32 [N, S_max, T_max] (unit stride along the columns), item n on its first
    rows[n] x cols[n] cells (tmi_dtw in include/tethys_mi.h): ``tok_start`` / ``tok_end`` int32 [N, S_max], ``total`` fp32 [N],
    optionally ``path`` int32 [N, S_max + T_max - 1, 2] with ``path_len`` int32 [N]; ``workspace`` int32,
    ``dtw_workspace_elems`` entries, any contents."""
    if cost.dtype != torch.float32 or cost.dim() != 3 or cost.stride(2) != 1:
        raise ValueError("dtw: cost must be float32 [N, S_max, T_max] with unit column stride")
    N, S, T = cost.shape
    _i32_dev(rows, N, "dtw: rows")
    _i32_dev(cols, N, "dtw: cols")
    _i32_dev(tok_start, N * S, "dtw: tok_start")
    _i32_dev(tok_end, N * S, "dtw: tok_end")
    _f32_flat(total, N, "dtw: total")
    _i32_dev(workspace, dtw_workspace_elems(N, S, T), "dtw: workspace")
    if (path is None) != (path_len is None):
        raise ValueError("dtw: path and path_len come together")
    if path is not None:
        _i32_dev(path, N * (S + T - 1) * 2, "dtw: path")
        _i32_dev(path_len, N, "dtw: path_len")
    with _probe("dtw", 4.0 * N * S * T):
        check(lib().tmi_dtw(cost.data_ptr(), cost.stride(0), cost.stride(1), rows.data_ptr(), cols.data_ptr(), N, S, T,
                            tok_start.data_ptr(), tok_end.data_ptr(), total.data_ptr(), ptr(path), ptr(path_len),
                            workspace.data_ptr(), workspace.numel() * 4, stream()), "tmi_dtw")


EDIT_MAX_COLS = 4096  # tmi_edit_distance: columns read of either side


def _edit_rows(t, what):
    if not isinstance(t, torch.Tensor) or t.device.type == "cpu" or t.dtype != torch.int32 or t.dim() != 2:
        raise ValueError(f"edit_distance: {what} must be an int32 [rows, cols] tensor on the device")
    rows, cols = t.shape
    if cols > EDIT_MAX_COLS:
        raise ValueError(f"edit_distance: {what} has {cols} columns, at most {EDIT_MAX_COLS} are read")
    if cols > 1 and t.stride(1) != 1:
        raise ValueError(f"edit_distance: {what} must have unit column stride")
    ld = t.stride(0) if rows > 1 else max(cols, 1)
    if ld < cols:
        raise ValueError(f"edit_distance: the rows of {what} overlap")
    return rows, cols, ld


def edit_distance(hyp, ref, hyp_len=None, ref_len=None, R=1, stop_id=-1, skip=(0, 0), out=None):
    """Levenshtein distance with operation counts of every (hypothesis, reference) pair, on the device (tmi_edit_distance in
    include/tethys_mi.h states the rule).  ``hyp`` int32 [N, n_cols], ``ref`` int32 [N / R, m_cols]: pair i is hypothesis i
    against reference i // R.  Both may be strided views with unit column stride (``sequences[:, 1 + P:]`` needs no copy).
    ``hyp_len`` [N], ``ref_len`` [N / R] int32 or None (the whole row).  Both sides are cut before ``stop_id`` (-1: no cut)
    and lose every token in [skip[0], skip[1]).  -> ``out`` int32 [N, 6] = (d, sub, del, ins, n, m) per pair (``out``: write
    there instead, int32 [N, >= 6] with unit column stride)."""
    N, hc, h_ld = _edit_rows(hyp, "hyp")
    Nr, rc, r_ld = _edit_rows(ref, "ref")
    R = int(R)
    if ref.device != hyp.device:
        raise ValueError("edit_distance: hyp and ref are on different devices")
    if N < 1 or N > 65535 or R < 1 or Nr * R != N:
        raise ValueError(f"edit_distance: 1 <= N <= 65535 hypotheses, R >= 1 per reference; got {N} against {Nr} with R = {R}")
    for t, n, w in ((hyp_len, N, "hyp_len"), (ref_len, Nr, "ref_len")):
        if t is not None:
            _i32_dev(t, n, "edit_distance: " + w)
            if t.device != hyp.device or t.numel() != n:
                raise ValueError(f"edit_distance: {w} must hold {n} entries on the device of hyp")
    if out is None:
        out = torch.empty(N, 6, dtype=torch.int32, device=hyp.device)
    elif (out.dtype != torch.int32 or out.device != hyp.device or out.dim() != 2 or out.shape[0] != N or out.shape[1] < 6 or
          out.stride(1) != 1 or (N > 1 and out.stride(0) < 6)):
        raise ValueError("edit_distance: out must be int32 [N, >= 6] with unit column stride on the device of hyp")
    with _probe("edit_distance", 8.0 * N * max(hc, 1) * max(rc, 1)):
        check(lib().tmi_edit_distance(hyp.data_ptr(), h_ld, hc, ptr(hyp_len), ref.data_ptr(), r_ld, rc, ptr(ref_len), N, R,
                                      int(stop_id), int(skip[0]), int(skip[1]), out.data_ptr(),
                                      out.stride(0) if N > 1 else max(out.shape[1], 6), stream()), "tmi_edit_distance")
    return out


EDIT_ALIGN_WORKSPACE_CAP = 256 << 20  # bytes of workspace ``edit_align`` allocates at most, when more than one chunk would need more


def edit_align_workspace_elems(N: int, hyp_cols: int, ref_cols: int) -> int:
    """int32 elements of tmi_edit_align's workspace (tmi_edit_align_workspace_bytes / 4)."""
    n = int(lib().tmi_edit_align_workspace_bytes(N, hyp_cols, ref_cols))
    if n < 0:
        raise ValueError(f"tmi_edit_align takes 1 <= N <= 65535 pairs of at most {EDIT_MAX_COLS} columns a side, got {N} x "
                         f"{hyp_cols} x {ref_cols}")
    return n // 4


def edit_align_chunks(N: int, R: int, pair_bytes: int, cap: int = EDIT_ALIGN_WORKSPACE_CAP):
    """The (first pair, pairs) pieces in which ``edit_align`` runs N pairs so that pairs * pair_bytes stays under ``cap``:
    every piece is a multiple of R (the R hypotheses of a reference stay together) and at least R, whatever the cap."""
    per = max(R, cap // max(pair_bytes, 1) // R * R)
    return [(s, min(per, N - s)) for s in range(0, N, per)]


def _edit_align_args(hyp, ref, hyp_len, ref_len, R, what):
    N, hc, h_ld = _edit_rows(hyp, "hyp")
    Nr, rc, r_ld = _edit_rows(ref, "ref")
    R = int(R)
    if ref.device != hyp.device:
        raise ValueError(f"{what}: hyp and ref are on different devices")
    if N < 1 or N > 65535 or R < 1 or Nr * R != N:
        raise ValueError(f"{what}: 1 <= N <= 65535 hypotheses, R >= 1 per reference; got {N} against {Nr} with R = {R}")
    for t, n, w in ((hyp_len, N, "hyp_len"), (ref_len, Nr, "ref_len")):
        if t is not None:
            _i32_dev(t, n, f"{what}: {w}")
            if t.device != hyp.device or t.numel() != n:
                raise ValueError(f"{what}: {w} must hold {n} entries on the device of hyp")
    return N, hc, h_ld, rc, r_ld, R


def edit_align(hyp, ref, hyp_len=None, ref_len=None, R=1, stop_id=-1, skip=(0, 0), workspace=None):
    """``edit_distance`` with the alignment (tmi_edit_align in include/tethys_mi.h): the same arguments and host checks, ->
    ``(out, steps, n_steps)``: ``out`` int32 [N, 6] as ``edit_distance`` gives it, ``steps`` int32 [N, hyp_cols + ref_cols, 3]
    of which the first ``n_steps[i]`` rows of pair i are written - (op, column in hyp, column in ref), op 0 match,
    1 substitution, 2 deletion, 3 insertion, the columns those of the tensors as passed in, -1 for the missing side -
    and ``n_steps`` int32 [N].  ``workspace``: int32, ``edit_align_workspace_elems(N, hyp_cols, ref_cols)`` entries, any
    contents, for ONE launch; None: allocated here, and the pairs run in the pieces of ``edit_align_chunks`` so that it
    stays under ``EDIT_ALIGN_WORKSPACE_CAP`` (pairs are independent: the pieces cannot change a result)."""
    N, hc, h_ld, rc, r_ld, R = _edit_align_args(hyp, ref, hyp_len, ref_len, R, "edit_align")
    dev = hyp.device
    out = torch.empty(N, 6, dtype=torch.int32, device=dev)
    steps = torch.empty(N, max(hc + rc, 1), 3, dtype=torch.int32, device=dev)
    n_steps = torch.empty(N, dtype=torch.int32, device=dev)
    if workspace is None:
        pieces = edit_align_chunks(N, R, 4 * edit_align_workspace_elems(1, hc, rc))
        workspace = torch.empty(edit_align_workspace_elems(pieces[0][1], hc, rc), dtype=torch.int32, device=dev)
    else:
        pieces = [(0, N)]
        _i32_dev(workspace, edit_align_workspace_elems(N, hc, rc), "edit_align: workspace")
        if workspace.device != dev:
            raise ValueError("edit_align: workspace must be on the device of hyp")
    for s, c in pieces:
        with _probe("edit_align", 8.0 * c * max(hc, 1) * max(rc, 1)):
            check(lib().tmi_edit_align(hyp[s:s + c].data_ptr(), h_ld, hc, ptr(None if hyp_len is None else hyp_len[s:s + c]),
                                       ref[s // R:(s + c) // R].data_ptr(), r_ld, rc,
                                       ptr(None if ref_len is None else ref_len[s // R:(s + c) // R]), c, R, int(stop_id),
                                       int(skip[0]), int(skip[1]), out[s:s + c].data_ptr(), 6, steps[s:s + c].data_ptr(),
                                       steps.stride(0), n_steps[s:s + c].data_ptr(), workspace.data_ptr(), workspace.numel() * 4,
                                       stream()), "tmi_edit_align")
    return out, steps[:, :hc + rc], n_steps


def edit_confusion(steps, n_steps, hyp, ref, V, R=1, first_only=True, counts=None):
    """The confusion table of the alignments ``edit_align`` returned for ``hyp`` and ``ref`` (tmi_edit_confusion in
    include/tethys_mi.h): ``counts`` int32 [(V + 1) * (V + 1) + 1] on the device - row = the reference token, column = the
    hypothesis token, index V = none, the trailing element = the steps whose tokens lie outside [0, V).  ``counts`` None:
    a fresh, zeroed table; given: the steps are ADDED to it (batches sum on the device).  ``first_only``: only the first of
    every reference's R hypotheses counts.  -> counts (``counts[:-1].view(V + 1, V + 1)`` is the table)."""
    N, hc, h_ld, rc, r_ld, R = _edit_align_args(hyp, ref, None, None, R, "edit_confusion")
    V = int(V)
    if V < 1 or V > 1024:
        raise ValueError(f"edit_confusion: 1 <= V <= 1024, got {V}")
    if (not isinstance(steps, torch.Tensor) or steps.dtype != torch.int32 or steps.device != hyp.device or steps.dim() != 3 or
            tuple(steps.shape) != (N, hc + rc, 3) or (hc + rc > 0 and (steps.stride(2) != 1 or steps.stride(1) != 3)) or
            (N > 1 and steps.stride(0) < 3 * (hc + rc))):
        raise ValueError(f"edit_confusion: steps must be int32 [{N}, {hc + rc}, 3] with dense rows on the device of hyp")
    _i32_dev(n_steps, N, "edit_confusion: n_steps")
    size = (V + 1) * (V + 1) + 1
    accumulate = counts is not None
    if counts is None:
        counts = torch.empty(size, dtype=torch.int32, device=hyp.device)
    else:
        _i32_dev(counts, size, "edit_confusion: counts")
    if n_steps.device != hyp.device or n_steps.numel() != N or counts.device != hyp.device or counts.numel() != size:
        raise ValueError(f"edit_confusion: n_steps [{N}] and counts [{size}] must be on the device of hyp")
    steps_ld = steps.stride(0) if N > 1 else max(3 * (hc + rc), steps.stride(0) if hc + rc > 0 else 3)
    with _probe("edit_confusion", 12.0 * N * max(hc + rc, 1)):
        check(lib().tmi_edit_confusion(steps.data_ptr(), steps_ld, n_steps.data_ptr(), hyp.data_ptr(), h_ld, hc, ref.data_ptr(),
                                       r_ld, rc, N, R, 1 if first_only else 0, V, counts.data_ptr(), 1 if accumulate else 0,
                                       stream()), "tmi_edit_confusion")
    return counts


EDIT_OPS = ("match", "substitution", "deletion", "insertion")  # the op codes 0..3 of tmi_edit_align's steps


def edit_alignment_items(steps, n_steps, hyp, ref, R=1):
    """The alignments of ``edit_align`` on the host, for the FIRST of every reference's R hypotheses: per item the list of
    (op, hyp_token, ref_token, hyp_column, ref_column) in order, None for the missing side.  The tokens are gathered by
    the steps' columns with torch on the device, then everything comes over in ONE read-back."""
    st, ns, h = steps[::R], n_steps[::R], hyp[::R]
    B, S = st.shape[0], st.shape[1]
    if S == 0:
        return [[] for _ in range(B)]
    live = torch.arange(S, device=st.device)[None, :] < ns[:, None]

    def tokens(rows, col):
        if rows.shape[1] == 0:
            return torch.zeros(B, S, dtype=torch.int32, device=st.device)
        return torch.gather(rows, 1, torch.where(live & (col >= 0), col, torch.zeros_like(col)).long().clamp_(max=rows.shape[1] - 1))

    host = torch.cat([st.reshape(B, 3 * S), tokens(h, st[:, :, 1]), tokens(ref, st[:, :, 2]), ns[:, None]], 1).cpu().numpy()
    items = []
    for b in range(B):
        row, n = host[b], int(host[b, 5 * S])
        items.append([(int(row[3 * k]), None if row[3 * k + 1] < 0 else int(row[3 * S + k]), None if row[3 * k + 2] < 0 else int(row[4 * S + k]),
                       None if row[3 * k + 1] < 0 else int(row[3 * k + 1]), None if row[3 * k + 2] < 0 else int(row[3 * k + 2]))
                      for k in range(n)])
    return items


def edit_counts(out, R=1, valid=None):
    """The sums of an ``edit_distance`` result as Python floats (fp64: shards can be added) - torch reductions on the device,
    then ONE read-back.  The error counts are over the first of every item's ``R`` rows; "n_oracle_edits" is the sum of the
    per-item minimum of d over its rows (``valid`` bool [items, R]: over these rows only; the first row always counts)."""
    o = out[:, :6].reshape(-1, R, 6)
    first = o[:, 0, :].long()
    d_all = o[:, :, 0].long()
    if valid is not None:
        keep = valid.clone()
        keep[:, 0] = True
        d_all = torch.where(keep, d_all, torch.full_like(d_all, 1 << 40))
    sums = torch.cat([first.sum(0), (first[:, 0] == 0).sum().view(1), d_all.min(1).values.sum().view(1)])
    d, s, dl, ins, nh, nr, ex, orc = (float(x) for x in sums.cpu().tolist())
    return finish_edit_counts({"n_edits": d, "n_sub": s, "n_del": dl, "n_ins": ins, "n_ref_tokens": nr, "n_hyp_tokens": nh,
                               "n_exact": ex, "n_items": float(o.shape[0]), "n_oracle_edits": orc})


EDIT_COUNT_KEYS = ("n_edits", "n_sub", "n_del", "n_ins", "n_ref_tokens", "n_hyp_tokens", "n_exact", "n_items", "n_oracle_edits")


def finish_edit_counts(c):
    """Adds the two rates to a dictionary of ``EDIT_COUNT_KEYS`` sums (NaN where there is no reference token)."""
    n = c["n_ref_tokens"]
    c["token_error_rate"] = c["n_edits"] / n if n > 0 else float("nan")
    c["oracle_error_rate"] = c["n_oracle_edits"] / n if n > 0 else float("nan")
    return c


def _ctc_logp(logp, what):
    if logp.dtype != torch.float32 or logp.dim() != 3 or logp.stride(2) != 1 or logp.stride(0) < logp.shape[1] * logp.stride(1):
        raise ValueError(f"{what}: logp must be float32 [N, T, V] with unit column stride")
    return logp.shape


def ctc_logsoftmax(logits, V, logp, argmax):
    """Row-wise log-softmax and argmax over the first ``V`` columns (tmi_ctc_logsoftmax in include/tethys_mi.h): ``logits``
    and ``logp`` fp32 [R, >= V] with unit column stride, ``argmax`` int32 [R]."""
    R = logits.shape[0]
    if (logits.dtype != torch.float32 or logp.dtype != torch.float32 or logits.dim() != 2 or logp.dim() != 2 or
            logits.stride(1) != 1 or logp.stride(1) != 1 or logp.shape[0] != R):
        raise ValueError("ctc_logsoftmax: logits and logp must be float32 [R, >= V] with unit column stride")
    _i32_dev(argmax, R, "ctc_logsoftmax: argmax")
    with _probe("ctc_logsoftmax", 8.0 * R * V):
        check(lib().tmi_ctc_logsoftmax(logits.data_ptr(), logits.stride(0), R, int(V), logp.data_ptr(), logp.stride(0),
                                       argmax.data_ptr(), stream()), "tmi_ctc_logsoftmax")


def ctc_greedy(argmax, logp, frame_lens, blank, tokens, out_len, tok_start, tok_end, best_logprob):
    """The greedy CTC collapse of every item (tmi_ctc_greedy): ``argmax`` int32 [N, T], ``logp`` fp32 [N, T, V] contiguous
    in (t, v); ``tokens`` / ``tok_start`` / ``tok_end`` int32 [N, T], ``out_len`` int32 [N], ``best_logprob`` fp32 [N]."""
    N, T, _ = _ctc_logp(logp, "ctc_greedy")
    if logp.stride(0) != T * logp.stride(1):
        raise ValueError("ctc_greedy: logp must be [N, T, lp_ld] without an item stride of its own")
    for t, n, w in ((argmax, N * T, "argmax"), (frame_lens, N, "frame_lens"), (tokens, N * T, "tokens"), (out_len, N, "out_len"),
                    (tok_start, N * T, "tok_start"), (tok_end, N * T, "tok_end")):
        _i32_dev(t, n, "ctc_greedy: " + w)
    _f32_flat(best_logprob, N, "ctc_greedy: best_logprob")
    with _probe("ctc_greedy", 8.0 * N * T):
        check(lib().tmi_ctc_greedy(argmax.data_ptr(), logp.data_ptr(), logp.stride(1), frame_lens.data_ptr(), int(blank),
                                   tokens.data_ptr(), out_len.data_ptr(), tok_start.data_ptr(), tok_end.data_ptr(),
                                   best_logprob.data_ptr(), N, T, stream()), "tmi_ctc_greedy")


def ctc_forward(logp, labels, label_lens, frame_lens, blank, nll, infeasible, zero_infinity=False):
    """The CTC negative log-likelihood of every item (tmi_ctc_forward): ``logp`` fp32 [N, T, V], ``labels`` int32
    [N, L_max] contiguous, lengths int32 [N]; ``nll`` fp32 [N], ``infeasible`` int32 [N]."""
    N, T, _ = _ctc_logp(logp, "ctc_forward")
    if labels.dim() != 2 or labels.shape[0] != N:
        raise ValueError("ctc_forward: labels must be int32 [N, L_max]")
    L = labels.shape[1]
    for t, n, w in ((labels, N * L, "labels"), (label_lens, N, "label_lens"), (frame_lens, N, "frame_lens"),
                    (infeasible, N, "infeasible")):
        _i32_dev(t, n, "ctc_forward: " + w)
    _f32_flat(nll, N, "ctc_forward: nll")
    with _probe("ctc_forward", 4.0 * N * T * (2 * L + 1)):
        check(lib().tmi_ctc_forward(logp.data_ptr(), logp.stride(0), logp.stride(1), labels.data_ptr(), label_lens.data_ptr(),
                                    frame_lens.data_ptr(), int(blank), nll.data_ptr(), infeasible.data_ptr(), N, L, T,
                                    1 if zero_infinity else 0, stream()), "tmi_ctc_forward")


def ctc_workspace_elems(N: int, L_max: int, T_max: int) -> int:
    """int32 elements of tmi_ctc_viterbi's workspace (tmi_ctc_workspace_bytes / 4)."""
    n = int(lib().tmi_ctc_workspace_bytes(N, L_max, T_max))
    if n < 0:
        raise ValueError(f"tmi_ctc_viterbi takes 1 <= N <= 65535 items of at most 511 labels x 4096 frames, got {N} x {L_max} x {T_max}")
    return n // 4


def ctc_viterbi(logp, labels, label_lens, frame_lens, blank, tok_start, tok_end, total, infeasible, workspace, states=None):
    """The best CTC path of every item (tmi_ctc_viterbi): inputs as ``ctc_forward``; ``tok_start`` / ``tok_end`` int32
    [N, L_max], ``total`` fp32 [N], ``infeasible`` int32 [N], ``states`` None or int32 [N, T]; ``workspace`` int32 of
    ``ctc_workspace_elems`` entries, any contents."""
    N, T, _ = _ctc_logp(logp, "ctc_viterbi")
    if labels.dim() != 2 or labels.shape[0] != N:
        raise ValueError("ctc_viterbi: labels must be int32 [N, L_max]")
    L = labels.shape[1]
    for t, n, w in ((labels, N * L, "labels"), (label_lens, N, "label_lens"), (frame_lens, N, "frame_lens"),
                    (tok_start, N * L, "tok_start"), (tok_end, N * L, "tok_end"), (infeasible, N, "infeasible"),
                    (workspace, ctc_workspace_elems(N, L, T), "workspace")):
        _i32_dev(t, n, "ctc_viterbi: " + w)
    if states is not None:
        _i32_dev(states, N * T, "ctc_viterbi: states")
    _f32_flat(total, N, "ctc_viterbi: total")
    with _probe("ctc_viterbi", 4.0 * N * T * (2 * L + 1)):
        check(lib().tmi_ctc_viterbi(logp.data_ptr(), logp.stride(0), logp.stride(1), labels.data_ptr(), label_lens.data_ptr(),
                                    frame_lens.data_ptr(), int(blank), tok_start.data_ptr(), tok_end.data_ptr(),
                                    total.data_ptr(), ptr(states), infeasible.data_ptr(), N, L, T, workspace.data_ptr(),
                                    workspace.numel() * 4, stream()), "tmi_ctc_viterbi")


def ctc_posteriors(logp, labels, label_lens, frame_lens, blank, nll, infeasible, gamma, occ, tok_frames, tok_center, grad=None,
                   zero_infinity=False):
    """The CTC forward-backward pass of every item (tmi_ctc_posteriors in include/tethys_mi.h): inputs as ``ctc_forward``
    with 2 <= V <= 64; ``nll`` fp32 [N], ``infeasible`` int32 [N], ``gamma`` fp32 [N, T, 2 L_max + 1] contiguous (the state
    posteriors; the call's scratch for alpha first), ``occ`` and optionally ``grad`` fp32 [N, T, V] with unit column stride
    (the symbol posteriors and d nll / d logits), ``tok_frames`` / ``tok_center`` fp32 [N, L_max].  At most 4096 frames."""
    N, T, V = _ctc_logp(logp, "ctc_posteriors")
    if labels.dim() != 2 or labels.shape[0] != N:
        raise ValueError("ctc_posteriors: labels must be int32 [N, L_max]")
    L = labels.shape[1]
    for t, n, w in ((labels, N * L, "labels"), (label_lens, N, "label_lens"), (frame_lens, N, "frame_lens"),
                    (infeasible, N, "infeasible")):
        _i32_dev(t, n, "ctc_posteriors: " + w)
    for t, n, w in ((nll, N, "nll"), (gamma, N * T * (2 * L + 1), "gamma"), (tok_frames, N * L, "tok_frames"),
                    (tok_center, N * L, "tok_center")):
        _f32_flat(t, n, "ctc_posteriors: " + w)
    for t, w in ((occ, "occ"),) + (() if grad is None else ((grad, "grad"),)):
        if tuple(_ctc_logp(t, "ctc_posteriors: " + w)) != (N, T, V):
            raise ValueError(f"ctc_posteriors: {w} must be float32 [N, T, V] as logp")
    with _probe("ctc_posteriors", 4.0 * N * T * (3 * (2 * L + 1) + 3 * V)):
        check(lib().tmi_ctc_posteriors(logp.data_ptr(), logp.stride(0), logp.stride(1), V, labels.data_ptr(),
                                       label_lens.data_ptr(), frame_lens.data_ptr(), int(blank), nll.data_ptr(),
                                       infeasible.data_ptr(), gamma.data_ptr(), occ.data_ptr(), occ.stride(0), occ.stride(1),
                                       ptr(grad), 0 if grad is None else grad.stride(0), 0 if grad is None else grad.stride(1),
                                       tok_frames.data_ptr(), tok_center.data_ptr(), N, L, T, 1 if zero_infinity else 0,
                                       stream()), "tmi_ctc_posteriors")


def ctc_beam_workspace_elems(N: int, K: int, T_max: int) -> int:
    """int32 elements of tmi_ctc_beam's workspace (tmi_ctc_beam_workspace_bytes / 4)."""
    n = int(lib().tmi_ctc_beam_workspace_bytes(int(N), int(K), int(T_max)))
    if n < 0:
        raise ValueError(f"tmi_ctc_beam takes 1 <= N <= 65535 items, 1 <= K <= 16 beams and at most 65536 frames, got {N} x {K} x {T_max}")
    return n // 4


def ctc_beam(logp, frame_lens, blank, K, tokens, lengths, scores, n_beams, workspace):
    """CTC prefix beam search of every item (tmi_ctc_beam in include/tethys_mi.h): ``logp`` fp32 [N, T, V] with 2 <= V <= 64,
    ``frame_lens`` int32 [N]; ``tokens`` int32 [N, K, T], ``lengths`` int32 [N, K], ``scores`` fp32 [N, K], ``n_beams`` int32
    [N]; ``workspace`` int32 of ``ctc_beam_workspace_elems`` entries, any contents."""
    N, T, V = _ctc_logp(logp, "ctc_beam")
    K = int(K)
    for t, n, w in ((frame_lens, N, "frame_lens"), (tokens, N * K * T, "tokens"), (lengths, N * K, "lengths"),
                    (n_beams, N, "n_beams"), (workspace, ctc_beam_workspace_elems(N, K, T), "workspace")):
        _i32_dev(t, n, "ctc_beam: " + w)
    _f32_flat(scores, N * K, "ctc_beam: scores")
    with _probe("ctc_beam", 4.0 * N * T * V):
        check(lib().tmi_ctc_beam(logp.data_ptr(), logp.stride(0), logp.stride(1), V, frame_lens.data_ptr(), int(blank), K,
                                 tokens.data_ptr(), lengths.data_ptr(), scores.data_ptr(), n_beams.data_ptr(), N, T,
                                 workspace.data_ptr(), workspace.numel() * 4, stream()), "tmi_ctc_beam")


def ctc_beam_lm(logp, frame_lens, blank, K, lm, lm_order, lm_alpha, lm_beta, tokens, lengths, scores, ctc_scores, lm_scores,
                n_beams, workspace):
    """``ctc_beam`` with an n-gram table in the ranking (tmi_ctc_beam_lm in include/tethys_mi.h): ``lm`` fp32, contiguous,
    V^lm_order entries on the device (finite or -inf: ``wav2vec2.check_ctc_lm_args``), 1 <= lm_order <= 4; ``scores`` the
    fused score, ``ctc_scores`` and ``lm_scores`` fp32 [N, K] its two terms."""
    N, T, V = _ctc_logp(logp, "ctc_beam_lm")
    K, lm_order = int(K), int(lm_order)
    if not 1 <= lm_order <= 4 or V ** lm_order > 1 << 24:
        raise ValueError(f"ctc_beam_lm: 1 <= lm_order <= 4 and V^lm_order <= 2^24, got order {lm_order} at V = {V}")
    for t, n, w in ((frame_lens, N, "frame_lens"), (tokens, N * K * T, "tokens"), (lengths, N * K, "lengths"),
                    (n_beams, N, "n_beams"), (workspace, ctc_beam_workspace_elems(N, K, T), "workspace")):
        _i32_dev(t, n, "ctc_beam_lm: " + w)
    for t, n, w in ((scores, N * K, "scores"), (ctc_scores, N * K, "ctc_scores"), (lm_scores, N * K, "lm_scores"),
                    (lm, V ** lm_order, "lm")):
        _f32_flat(t, n, "ctc_beam_lm: " + w)
    if lm.device != logp.device:
        raise ValueError("ctc_beam_lm: lm must be on the device of logp")
    with _probe("ctc_beam_lm", 4.0 * N * T * V):
        check(lib().tmi_ctc_beam_lm(logp.data_ptr(), logp.stride(0), logp.stride(1), V, frame_lens.data_ptr(), int(blank), K,
                                    lm.data_ptr(), lm_order, float(lm_alpha), float(lm_beta), tokens.data_ptr(),
                                    lengths.data_ptr(), scores.data_ptr(), ctc_scores.data_ptr(), lm_scores.data_ptr(),
                                    n_beams.data_ptr(), N, T, workspace.data_ptr(), workspace.numel() * 4, stream()),
              "tmi_ctc_beam_lm")


def masked_mean_pool(x, mask, out, B, T, C):
    """out[b, c] = sum_t x[b, t, c] mask[b, t] / sum_t mask[b, t] (fp32 [B, C]); ``mask`` fp32 [B, T] or None: the plain mean."""
    if not x.is_contiguous() or out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != B * C or x.numel() != B * T * C:
        raise ValueError("masked_mean_pool: x [B, T, C] contiguous, out float32 [B, C] contiguous")
    if mask is not None and (mask.dtype != torch.float32 or not mask.is_contiguous() or mask.numel() != B * T):
        raise ValueError("masked_mean_pool: mask must be float32 [B, T] contiguous")
    check(lib().tmi_masked_mean_pool(x.data_ptr(), dt(x), ptr(mask), out.data_ptr(), B, T, C, stream()), "tmi_masked_mean_pool")


def cls_head_workspace_elems(N: int, H: int, P: int, C: int) -> int:
    """float32 elements of tmi_cls_head_bwd's workspace (tmi_cls_head_workspace_bytes / 4)."""
    n = int(lib().tmi_cls_head_workspace_bytes(int(N), int(H), int(P), int(C)))
    if n < 0:
        raise ValueError(f"tmi_cls_head takes 1 <= N <= 65535 rows, H <= 4096 a multiple of 4, P even <= 1024 and 1 <= C <= 1024, "
                         f"got {N} x {H} x {P} x {C}")
    return n // 4


def _cls_rows(t, cols, what):
    """A float32 2-D tensor with unit column stride and at least ``cols`` columns -> its row stride."""
    if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] < cols or (t.shape[1] > 1 and t.stride(1) != 1) or t.stride(0) < cols:
        raise ValueError(f"{what} must be float32 [rows, >= {cols}] with unit column stride")
    return t.stride(0)


def _cls_head_args(pooled, row_index, labels, N, H, what):
    ld_x = _cls_rows(pooled, H, what + ": pooled")
    if row_index is not None:
        _i32_dev(row_index, N, what + ": row_index")
    elif pooled.shape[0] < N:
        raise ValueError(f"{what}: pooled holds {pooled.shape[0]} rows, the call asks for {N}")
    if labels is not None:
        _i32_dev(labels, N, what + ": labels")
    return ld_x, int(pooled.shape[0])


def cls_head_fwd(pooled, Wp, bp, Wc, bc, logits, pred, N=None, row_index=None, labels=None, p=0.0, seed=0, z=None,
                 log_probs=None, nll=None, label_rank=None, confusion=None):
    """The classification head on ``N`` pooled rows (tmi_cls_head_fwd in include/tethys_mi.h): ``pooled`` fp32 [n_src, H]
    (any row stride), gathered through ``row_index`` int32 [N] when given; ``Wp`` [H, P], ``bp`` [P], ``Wc`` [P, C], ``bc``
    [C] contiguous fp32; ``logits`` fp32 [N, C] and ``pred`` int32 [N] are written, and of the optional outputs those given:
    ``z`` fp32 [N, P] (tanh before dropout), ``log_probs`` fp32 [N, C], ``nll`` fp32 [N], ``label_rank`` int32 [N],
    ``confusion`` int64 [C, C] (added to: the caller zeroes it).  ``labels`` int32 [N] (outside [0, C): unlabelled)."""
    H, P = Wp.shape
    C = Wc.shape[1]
    N = int(pooled.shape[0] if N is None and row_index is None else (row_index.numel() if N is None else N))
    ld_x, n_src = _cls_head_args(pooled, row_index, labels, N, H, "cls_head_fwd")
    for t, n, w in ((Wp, H * P, "Wp"), (bp, P, "bp"), (Wc, P * C, "Wc"), (bc, C, "bc")) + \
            (() if nll is None else ((nll, N, "nll"),)):
        _f32_flat(t, n, "cls_head_fwd: " + w)
    if Wc.shape[0] != P or logits.shape[0] < N:
        raise ValueError("cls_head_fwd: Wc must be [P, C] and logits hold N rows")
    ld_lg = _cls_rows(logits, C, "cls_head_fwd: logits")
    ld_z = 0 if z is None else _cls_rows(z, P, "cls_head_fwd: z")
    ld_lp = 0 if log_probs is None else _cls_rows(log_probs, C, "cls_head_fwd: log_probs")
    _i32_dev(pred, N, "cls_head_fwd: pred")
    if label_rank is not None:
        _i32_dev(label_rank, N, "cls_head_fwd: label_rank")
    ld_cf = 0
    if confusion is not None:
        if confusion.dtype != torch.int64 or confusion.dim() != 2 or confusion.shape[0] < C or confusion.shape[1] < C or confusion.stride(1) != 1:
            raise ValueError("cls_head_fwd: confusion must be int64 [C, C] with unit column stride")
        ld_cf = confusion.stride(0)
    with _probe("cls_head_fwd", 2.0 * N * (H * P + P * C)):
        check(lib().tmi_cls_head_fwd(pooled.data_ptr(), ld_x, n_src, ptr(row_index), Wp.data_ptr(), bp.data_ptr(), Wc.data_ptr(),
                                     bc.data_ptr(), ptr(labels), float(p), int(seed) & 0xFFFFFFFFFFFFFFFF, logits.data_ptr(),
                                     ld_lg, pred.data_ptr(), ptr(z), ld_z, ptr(log_probs), ld_lp, ptr(nll), ptr(label_rank),
                                     ptr(confusion), ld_cf, N, H, P, C, stream()), "tmi_cls_head_fwd")


def cls_head_bwd(pooled, Wc, labels, z, log_probs, gWp, gbp, gWc, gbc, loss, workspace, N=None, row_index=None, p=0.0, seed=0):
    """The head's backward (tmi_cls_head_bwd in include/tethys_mi.h) from the ``z`` and ``log_probs`` that ``cls_head_fwd``
    saved with the same ``row_index``, ``labels``, ``p`` and ``seed``: ``gWp`` [H, P], ``gbp`` [P], ``gWc`` [P, C], ``gbc``
    [C] (written, not accumulated) and the mean loss over the labelled rows in ``loss`` [1].  ``workspace``: float32, of
    ``cls_head_workspace_elems(N, H, P, C)`` elements, any contents; dpre [N, P] is left behind its 64-element header."""
    H, P = gWp.shape
    C = Wc.shape[1]
    N = int(pooled.shape[0] if N is None and row_index is None else (row_index.numel() if N is None else N))
    if labels is None:
        raise ValueError("cls_head_bwd: labels are required")
    ld_x, n_src = _cls_head_args(pooled, row_index, labels, N, H, "cls_head_bwd")
    for t, n, w in ((Wc, P * C, "Wc"), (gWp, H * P, "gWp"), (gbp, P, "gbp"), (gWc, P * C, "gWc"), (gbc, C, "gbc"), (loss, 1, "loss"),
                    (workspace, cls_head_workspace_elems(N, H, P, C), "workspace")):
        _f32_flat(t, n, "cls_head_bwd: " + w)
    if Wc.shape[0] != P or z.shape[0] < N or log_probs.shape[0] < N:
        raise ValueError("cls_head_bwd: Wc must be [P, C]; z and log_probs hold N rows")
    ld_z, ld_lp = _cls_rows(z, P, "cls_head_bwd: z"), _cls_rows(log_probs, C, "cls_head_bwd: log_probs")
    with _probe("cls_head_bwd", 2.0 * N * (H * P + 3 * P * C)):
        check(lib().tmi_cls_head_bwd(pooled.data_ptr(), ld_x, n_src, ptr(row_index), Wc.data_ptr(), labels.data_ptr(), float(p),
                                     int(seed) & 0xFFFFFFFFFFFFFFFF, z.data_ptr(), ld_z, log_probs.data_ptr(), ld_lp,
                                     gWp.data_ptr(), gbp.data_ptr(), gWc.data_ptr(), gbc.data_ptr(), loss.data_ptr(),
                                     workspace.data_ptr(), workspace.numel() * 4, N, H, P, C, stream()), "tmi_cls_head_bwd")


def ctc_head_workspace_elems(N: int, T_max: int, H: int, V: int) -> int:
    """float32 elements of tmi_ctc_head_bwd's workspace (tmi_ctc_head_workspace_bytes / 4)."""
    n = int(lib().tmi_ctc_head_workspace_bytes(int(N), int(T_max), int(H), int(V)))
    if n < 0:
        raise ValueError(f"tmi_ctc_head takes 1 <= N <= 65535 items of 1 <= T_max <= 4096 frames, N * T_max <= 2^22, 8 <= H <= 4096 a "
                         f"multiple of 8 and 2 <= V <= 64, got {N} x {T_max} x {H} x {V}")
    return n // 4


def _ctc_head_args(hidden, row_index, frame_lens, N, T_max, H, what):
    """``hidden`` bf16 / fp32 [n_src, >= T_max, >= H] with unit column stride -> (x_sn, x_st, n_src)."""
    if hidden.dtype not in (torch.float32, torch.bfloat16) or hidden.dim() != 3 or hidden.shape[1] < T_max or hidden.shape[2] < H or \
            hidden.stride(2) != 1 or hidden.stride(1) < H or hidden.stride(0) < T_max * hidden.stride(1):
        raise ValueError(f"{what}: hidden must be bfloat16 or float32 [n_src, >= {T_max}, >= {H}] with unit column stride")
    if row_index is not None:
        _i32_dev(row_index, N, what + ": row_index")
    elif hidden.shape[0] < N:
        raise ValueError(f"{what}: hidden holds {hidden.shape[0]} items, the call asks for {N}")
    _i32_dev(frame_lens, N, what + ": frame_lens")
    return hidden.stride(0), hidden.stride(1), int(hidden.shape[0])


def _mask_bits(bits, N, cols, what):
    """A span mask of ``spec_masks`` (or None) -> (pointer, ld): uint32 bits held in an int32 tensor [>= N, ld], unit column
    stride, ld >= ceil(cols / 32)."""
    if bits is None:
        return None, 0
    if bits.dtype != torch.int32 or bits.dim() != 2 or bits.shape[0] < N or bits.shape[1] < (cols + 31) // 32 or \
            bits.stride(1) != 1 or bits.stride(0) < bits.shape[1]:
        raise ValueError(f"{what} must be an int32 tensor [>= {N}, >= {(cols + 31) // 32}] with unit column stride (spec_masks)")
    return bits.data_ptr(), bits.stride(0)


def spec_masks_words(cols: int) -> int:
    """uint32 words per row of a span mask over ``cols`` columns."""
    return (int(cols) + 31) // 32


def spec_masks(N, T_max, H, time_bits=None, feat_bits=None, counts=None, time_prob=0.05, time_length=10, feat_prob=0.05,
               feat_length=10, seed=0):
    """The SpecAugment span masks of one call as bits (tmi_spec_masks in include/tethys_mi.h), both from one launch:
    ``time_bits`` int32 [N, >= ceil(T_max / 32)] (frame t is bit t % 32 of word t / 32) and ``feat_bits`` int32
    [N, >= ceil(H / 32)], either None (that mask is off), and ``counts`` int32 [N, 2] (or None): the set bits per row.
    ``seed`` is the site seed."""
    tb, ld_t = _mask_bits(time_bits, N, T_max, "spec_masks: time_bits")
    fb, ld_f = _mask_bits(feat_bits, N, H, "spec_masks: feat_bits")
    if counts is not None:
        _i32_dev(counts, 2 * N, "spec_masks: counts")
    check(lib().tmi_spec_masks(tb, ld_t, fb, ld_f, ptr(counts), int(N), int(T_max), int(H), float(time_prob), int(time_length),
                               float(feat_prob), int(feat_length), int(seed) & 0xFFFFFFFFFFFFFFFF, stream()), "tmi_spec_masks")


def span_mask_apply(x, out, time_bits=None, feat_bits=None):
    """``out`` = ``x`` with the masked elements set to +0 (tmi_span_mask_apply in include/tethys_mi.h): ``x`` and ``out``
    bf16 / fp32 [N, T, H] of one dtype with unit column stride; ``time_bits`` / ``feat_bits`` as ``spec_masks`` writes them."""
    if x.dtype not in (torch.float32, torch.bfloat16) or out.dtype != x.dtype or x.dim() != 3 or out.shape != x.shape or \
            x.stride(2) != 1 or out.stride(2) != 1:
        raise ValueError("span_mask_apply: x and out must be bfloat16 or float32 [N, T, H] of one dtype with unit column stride")
    N, T, H = x.shape
    tb, ld_t = _mask_bits(time_bits, N, T, "span_mask_apply: time_bits")
    fb, ld_f = _mask_bits(feat_bits, N, H, "span_mask_apply: feat_bits")
    check(lib().tmi_span_mask_apply(x.data_ptr(), dt(x), x.stride(0), x.stride(1), tb, ld_t, fb, ld_f, out.data_ptr(),
                                    out.stride(0), out.stride(1), N, T, H, stream()), "tmi_span_mask_apply")


def ctc_head_fwd(hidden, W, b, frame_lens, logp, row_index=None, p=0.0, seed=0, logits=None, argmax=None, time_bits=None,
                 feat_bits=None):
    """Dropout, the Dense head and the log-softmax over cached encoder features (tmi_ctc_head_fwd in include/tethys_mi.h):
    ``hidden`` bf16 / fp32 [n_src, >= T_max, H], gathered per item through ``row_index`` int32 [N] when given; ``W`` [H, V],
    ``b`` [V] contiguous fp32; ``frame_lens`` int32 [N] by position; ``logp`` fp32 [N, T_max, V] is written on the frames
    inside each length, and so are ``logits`` (the same shape) and ``argmax`` int32 [N, T_max] when given.  ``time_bits`` /
    ``feat_bits`` (``spec_masks``, by position): tmi_ctc_head_fwd_m zeroes the features under them; both None: the plain call."""
    N, T_max, V = _ctc_logp(logp, "ctc_head_fwd")
    H = W.shape[0]
    x_sn, x_st, n_src = _ctc_head_args(hidden, row_index, frame_lens, N, T_max, H, "ctc_head_fwd")
    if W.dim() != 2 or W.shape[1] != V:
        raise ValueError("ctc_head_fwd: W must be [H, V] with V the columns of logp")
    _f32_flat(W, H * V, "ctc_head_fwd: W")
    _f32_flat(b, V, "ctc_head_fwd: b")
    if logits is not None and tuple(_ctc_logp(logits, "ctc_head_fwd: logits")) != (N, T_max, V):
        raise ValueError("ctc_head_fwd: logits must be float32 [N, T, V] as logp")
    if argmax is not None:
        _i32_dev(argmax, N * T_max, "ctc_head_fwd: argmax")
    args = (hidden.data_ptr(), dt(hidden), x_sn, x_st, n_src, ptr(row_index), frame_lens.data_ptr(), W.data_ptr(), b.data_ptr(),
            float(p), int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(logits), 0 if logits is None else logits.stride(0),
            0 if logits is None else logits.stride(1), logp.data_ptr(), logp.stride(0), logp.stride(1), ptr(argmax), N, T_max, H, V)
    masks = _mask_bits(time_bits, N, T_max, "ctc_head_fwd: time_bits") + _mask_bits(feat_bits, N, H, "ctc_head_fwd: feat_bits")
    with _probe("ctc_head_fwd", 2.0 * N * T_max * H * V):
        if time_bits is None and feat_bits is None:
            check(lib().tmi_ctc_head_fwd(*args, stream()), "tmi_ctc_head_fwd")
        else:
            check(lib().tmi_ctc_head_fwd_m(*args, *masks, stream()), "tmi_ctc_head_fwd_m")


def ctc_head_bwd(hidden, frame_lens, label_lens, grad, nll, infeasible, gW, gb, loss, n_infeasible, workspace, L_max,
                 row_index=None, p=0.0, seed=0, reduction="mean", time_bits=None, feat_bits=None):
    """The head's weight and bias gradients (tmi_ctc_head_bwd in include/tethys_mi.h) from the ``grad`` fp32 [N, T_max, V],
    ``nll`` and ``infeasible`` that ``ctc_posteriors`` wrote for the log-probs of ``ctc_head_fwd`` with the same ``hidden``,
    ``row_index``, ``frame_lens``, ``p`` and ``seed``: ``gW`` [H, V], ``gb`` [V], ``loss`` [1] fp32 and ``n_infeasible`` [1] int32
    are written, not accumulated.  ``workspace``: float32, ``ctc_head_workspace_elems(N, T_max, H, V)`` elements, any contents.
    ``time_bits`` / ``feat_bits``: the masks of the forward (tmi_ctc_head_bwd_m); both None: the plain call."""
    N, T_max, V = _ctc_logp(grad, "ctc_head_bwd")
    H = gW.shape[0]
    if reduction not in ("sum", "mean"):
        raise ValueError('ctc_head_bwd: reduction must be "sum" or "mean"')
    x_sn, x_st, n_src = _ctc_head_args(hidden, row_index, frame_lens, N, T_max, H, "ctc_head_bwd")
    for t, n, w in ((label_lens, N, "label_lens"), (infeasible, N, "infeasible"), (n_infeasible, 1, "n_infeasible")):
        _i32_dev(t, n, "ctc_head_bwd: " + w)
    for t, n, w in ((nll, N, "nll"), (gW, H * V, "gW"), (gb, V, "gb"), (loss, 1, "loss"),
                    (workspace, ctc_head_workspace_elems(N, T_max, H, V), "workspace")):
        _f32_flat(t, n, "ctc_head_bwd: " + w)
    if gW.dim() != 2 or gW.shape[1] != V:
        raise ValueError("ctc_head_bwd: gW must be [H, V] with V the columns of grad")
    args = (hidden.data_ptr(), dt(hidden), x_sn, x_st, n_src, ptr(row_index), frame_lens.data_ptr(), label_lens.data_ptr(),
            grad.data_ptr(), grad.stride(0), grad.stride(1), nll.data_ptr(), infeasible.data_ptr(), float(p),
            int(seed) & 0xFFFFFFFFFFFFFFFF, 1 if reduction == "mean" else 0, gW.data_ptr(), gb.data_ptr(), loss.data_ptr(),
            n_infeasible.data_ptr(), workspace.data_ptr(), workspace.numel() * 4, N, T_max, int(L_max), H, V)
    masks = _mask_bits(time_bits, N, T_max, "ctc_head_bwd: time_bits") + _mask_bits(feat_bits, N, H, "ctc_head_bwd: feat_bits")
    with _probe("ctc_head_bwd", 2.0 * N * T_max * H * V):
        if time_bits is None and feat_bits is None:
            check(lib().tmi_ctc_head_bwd(*args, stream()), "tmi_ctc_head_bwd")
        else:
            check(lib().tmi_ctc_head_bwd_m(*args, *masks, stream()), "tmi_ctc_head_bwd_m")


def layer_mix_workspace_elems(N: int, T_max: int, H: int, V: int, K: int) -> int:
    """float32 elements of tmi_layer_mix_bwd's workspace (tmi_layer_mix_workspace_bytes / 4)."""
    n = int(lib().tmi_layer_mix_workspace_bytes(int(N), int(T_max), int(H), int(V), int(K)))
    if n < 0:
        raise ValueError(f"tmi_layer_mix takes 1 <= K <= 64 layers and the sizes of tmi_ctc_head (1 <= N <= 65535, 1 <= T_max <= "
                         f"4096, N * T_max <= 2^22, 8 <= H <= 4096 a multiple of 8, 2 <= V <= 64), got K {K}, {N} x {T_max} x {H} x {V}")
    return n // 4


def _layer_mix_args(layers, row_index, frame_lens, N, T_max, H, what):
    """``layers``: one stacked tensor [K, n_src, >= T_max, >= H] or a sequence of K tensors [n_src, >= T_max, >= H] of one
    dtype, shape and strides -> (host array of K device pointers, K, a layer, x_sn, x_st, n_src)."""
    if torch.is_tensor(layers):
        if layers.dim() != 4:
            raise ValueError(f"{what}: stacked layers must be [K, n_src, T, H]")
        layers = layers.unbind(0)
    layers = list(layers)
    K = len(layers)
    if not 1 <= K <= 64:
        raise ValueError(f"{what}: 1 <= K <= 64 layers, got {K}")
    x0 = layers[0]
    for x in layers:
        if not torch.is_tensor(x) or x.dtype != x0.dtype or x.shape != x0.shape or x.stride() != x0.stride() or x.device != x0.device:
            raise ValueError(f"{what}: every layer must have the dtype, shape, strides and device of the first")
    x_sn, x_st, n_src = _ctc_head_args(x0, row_index, frame_lens, N, T_max, H, what)
    table = (C.c_void_p * K)(*[x.data_ptr() for x in layers])
    return table, K, x0, x_sn, x_st, n_src


def layer_mix_fwd(layers, a, frame_lens, mixed, row_index=None, w_out=None):
    """The softmax-weighted sum of K layers of hidden states (tmi_layer_mix_fwd in include/tethys_mi.h): ``layers`` one
    stacked bf16 / fp32 tensor [K, n_src, >= T_max, H] or a sequence of K tensors [n_src, >= T_max, H] of one layout, gathered
    per item through ``row_index`` int32 [N] when given; ``a`` fp32 with at least K entries, the mixing logits;
    ``frame_lens`` int32 [N] by position; ``mixed`` fp32 [N, T_max, H] is written on the frames inside each length, by
    position; ``w_out`` fp32 (at least K entries) receives softmax(a) when given."""
    if mixed.dtype != torch.float32 or mixed.dim() != 3 or mixed.stride(2) != 1:
        raise ValueError("layer_mix_fwd: mixed must be float32 [N, T_max, H] with unit column stride")
    N, T_max, H = mixed.shape
    table, K, x0, x_sn, x_st, n_src = _layer_mix_args(layers, row_index, frame_lens, N, T_max, H, "layer_mix_fwd")
    _f32_flat(a, K, "layer_mix_fwd: a")
    if w_out is not None:
        _f32_flat(w_out, K, "layer_mix_fwd: w_out")
    with _probe("layer_mix_fwd", 2.0 * N * T_max * H * K):
        check(lib().tmi_layer_mix_fwd(table, K, dt(x0), x_sn, x_st, n_src, ptr(row_index), frame_lens.data_ptr(), a.data_ptr(),
                                      ptr(w_out), mixed.data_ptr(), mixed.stride(0), mixed.stride(1), N, T_max, H, stream()),
              "tmi_layer_mix_fwd")


def layer_mix_bwd(layers, a, frame_lens, label_lens, grad, infeasible, W, g_a, workspace, L_max, row_index=None, p=0.0, seed=0,
                  reduction="mean", d=None, time_bits=None, feat_bits=None):
    """The gradient of the head's loss with respect to the mixing logits (tmi_layer_mix_bwd in include/tethys_mi.h) from the
    ``grad`` fp32 [N, T_max, V] and ``infeasible`` that ``ctc_posteriors`` wrote for the log-probs ``ctc_head_fwd`` formed
    from ``layer_mix_fwd``'s output with dropout (``p``, ``seed``) and the head's ``W`` fp32 [H, V]: ``g_a`` fp32 (at least K
    entries) and, when given, ``d`` (the gradient with respect to the weights) are written, not accumulated.  ``workspace``:
    float32, ``layer_mix_workspace_elems(N, T_max, H, V, K)`` elements, any contents.  ``time_bits`` / ``feat_bits``: the masks
    the head's forward applied to the mixed features (tmi_layer_mix_bwd_m); both None: the plain call."""
    N, T_max, V = _ctc_logp(grad, "layer_mix_bwd")
    H = W.shape[0]
    if reduction not in ("sum", "mean"):
        raise ValueError('layer_mix_bwd: reduction must be "sum" or "mean"')
    table, K, x0, x_sn, x_st, n_src = _layer_mix_args(layers, row_index, frame_lens, N, T_max, H, "layer_mix_bwd")
    if W.dim() != 2 or W.shape[1] != V:
        raise ValueError("layer_mix_bwd: W must be [H, V] with V the columns of grad")
    for t, n, w in ((label_lens, N, "label_lens"), (infeasible, N, "infeasible")):
        _i32_dev(t, n, "layer_mix_bwd: " + w)
    for t, n, w in ((W, H * V, "W"), (a, K, "a"), (g_a, K, "g_a"),
                    (workspace, layer_mix_workspace_elems(N, T_max, H, V, K), "workspace")) + (() if d is None else ((d, K, "d"),)):
        _f32_flat(t, n, "layer_mix_bwd: " + w)
    args = (table, K, dt(x0), x_sn, x_st, n_src, ptr(row_index), frame_lens.data_ptr(), label_lens.data_ptr(), grad.data_ptr(),
            grad.stride(0), grad.stride(1), infeasible.data_ptr(), float(p), int(seed) & 0xFFFFFFFFFFFFFFFF,
            1 if reduction == "mean" else 0, W.data_ptr(), a.data_ptr(), g_a.data_ptr(), ptr(d), workspace.data_ptr(),
            workspace.numel() * 4, N, T_max, int(L_max), H, V)
    masks = _mask_bits(time_bits, N, T_max, "layer_mix_bwd: time_bits") + _mask_bits(feat_bits, N, H, "layer_mix_bwd: feat_bits")
    with _probe("layer_mix_bwd", 2.0 * N * T_max * H * (V + K)):
        if time_bits is None and feat_bits is None:
            check(lib().tmi_layer_mix_bwd(*args, stream()), "tmi_layer_mix_bwd")
        else:
            check(lib().tmi_layer_mix_bwd_m(*args, *masks, stream()), "tmi_layer_mix_bwd_m")


def fill_zero(t):
    """t[...] = 0 on the launch stream through the library (tmi_memset_async / tmi_memset2d_async), so that the fill is part
    of a recorded launch plan: a torch ``zero_()`` between two recorded launches would be missing from every replay.
    Contiguous tensors, or views whose slices along dim 0 are contiguous (the pad rows of a [B, T, C] buffer)."""
    es = t.element_size()
    if t.is_contiguous():
        check(lib().tmi_memset_async(t.data_ptr(), 0, t.numel() * es, stream()), "tmi_memset_async")
        return
    if t.dim() < 2 or not t[0].is_contiguous():
        raise ValueError("fill_zero: contiguous tensor or a view with contiguous slices along dim 0")
    if t.numel() == 0:
        return
    check(lib().tmi_memset2d_async(t.data_ptr(), t.stride(0) * es, 0, t[0].numel() * es, t.shape[0], stream()),
          "tmi_memset2d_async")


def copy(dst, src):
    """dst[...] = src[...] (same dtype and element count, both contiguous) on the launch stream, through the library."""
    if dst.dtype != src.dtype or dst.numel() != src.numel() or not dst.is_contiguous() or not src.is_contiguous():
        raise ValueError("copy: contiguous tensors of one dtype and size")
    check(lib().tmi_memcpy_async(dst.data_ptr(), src.data_ptr(), dst.numel() * dst.element_size(), stream()), "tmi_memcpy_async")


def dropout(x, out, rows, cols, p, seed, resid=None):
    """out = (resid or 0) + Dropout_p(x) over [rows, cols] (row strides from the tensors); the same call on the
    incoming gradient, with the same seed, is the backward.  See tmi_dropout in include/tethys_mi.h."""
    if PROFILE is not None:
        with _probe("dropout", (3.0 if resid is not None else 2.0) * rows * cols * x.element_size()):
            check(lib().tmi_dropout(x.data_ptr(), x.stride(0), ptr(resid), resid.stride(0) if resid is not None else 0,
                                    out.data_ptr(), out.stride(0), rows, cols, p, seed, dt(x), stream()), "tmi_dropout")
        return
    check(lib().tmi_dropout(x.data_ptr(), x.stride(0), ptr(resid), resid.stride(0) if resid is not None else 0,
                            out.data_ptr(), out.stride(0), rows, cols, p, seed, dt(x), stream()), "tmi_dropout")


def embed_fwd(labels, table, pe, out, B, S, D, start_id):
    check(lib().tmi_embed_fwd(labels.data_ptr(), table.data_ptr(), pe.data_ptr(), out.data_ptr(), B, S, D,
                              start_id, dt(out), stream()), "tmi_embed_fwd")


def embed_bwd(labels, dy, dtable, B, S, D, start_id):
    check(lib().tmi_embed_bwd(labels.data_ptr(), dy.data_ptr(), dtable.data_ptr(), B, S, D, start_id,
                              dt(dy), stream()), "tmi_embed_bwd")


def xent_fwd_bwd(logits, ld, labels, row_loss, B, S, V, grad_scale, lm=None):
    """``lm = (x, x_ld, w, w_sk, w_sn, d)``: the logits are the LM head's output x . w - tmi_linear_xent takes the target logit of
    the loss from those operands in fp32 instead of from the bf16-rounded logits."""
    # (the kernel holds a row on chip: ONE read and one write of the logits, csrc/softmax_xent.hip - not the three passes of an
    # unfused softmax + loss + gradient)
    with _probe("xent", 2.0 * B * S * V * logits.element_size()):
        if lm is None:
            check(lib().tmi_xent_fwd_bwd(logits.data_ptr(), ld, labels.data_ptr(), row_loss.data_ptr(), B, S, V,
                                         grad_scale, dt(logits), stream()), "tmi_xent_fwd_bwd")
        else:
            x, x_ld, w, w_sk, w_sn, d = lm
            check(lib().tmi_linear_xent(x.data_ptr(), x_ld, w.data_ptr(), w_sk, w_sn, d, logits.data_ptr(), ld, labels.data_ptr(),
                                        row_loss.data_ptr(), B, S, V, grad_scale, dt(logits), stream()), "tmi_linear_xent")


def _f32_flat(t, n, what):
    if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() < n:
        raise ValueError(f"{what}: float32, contiguous, at least {n} elements")


def xent_weights(mask, B, S, row_w, inv_wsum):
    """tmi_xent_weights: row_w[b*S+t] = mask[b, t] (t < S-1; 0 for t = S-1 and for entries that are not > 0) and
    inv_wsum[0] = 1 / sum(row_w), or 0 when that sum is 0 - on the device, in a fixed order, with no host read.
    ``mask`` [B, S] float32 with unit column stride (any row stride >= S)."""
    if mask.dtype != torch.float32 or tuple(mask.shape) != (B, S) or mask.stride(1) != 1 or (B > 1 and mask.stride(0) < S):
        raise ValueError("xent_weights: mask must be float32 [B, S] with unit column stride")
    _f32_flat(row_w, B * S, "xent_weights: row_w")
    _f32_flat(inv_wsum, 1, "xent_weights: inv_wsum")
    check(lib().tmi_xent_weights(mask.data_ptr(), mask.stride(0) if B > 1 else S, B, S, row_w.data_ptr(), inv_wsum.data_ptr(),
                                 stream()), "tmi_xent_weights")


def xent_fwd_bwd_weighted(logits, ld, labels, row_w, inv_wsum, row_loss, B, S, V, loss_scale, lm=None):
    """``xent_fwd_bwd`` under the row weights of ``xent_weights`` (W:596-598): a row with weight 0 is not read, its gradient is
    +0 and its loss 0; a scored row's gradient scale is loss_scale * row_w[r] * inv_wsum[0] and row_loss[r] = row_w[r] * nll.
    Every weight 0: loss 0 and all-zero gradients (the reference would divide 0 by 0).  ``lm`` as in ``xent_fwd_bwd``."""
    _f32_flat(row_w, B * S, "xent_fwd_bwd_weighted: row_w")
    _f32_flat(inv_wsum, 1, "xent_fwd_bwd_weighted: inv_wsum")
    with _probe("xent", 2.0 * B * S * V * logits.element_size()):
        if lm is None:
            check(lib().tmi_xent_weighted(logits.data_ptr(), ld, labels.data_ptr(), row_w.data_ptr(), inv_wsum.data_ptr(),
                                          row_loss.data_ptr(), B, S, V, loss_scale, dt(logits), stream()), "tmi_xent_weighted")
        else:
            x, x_ld, w, w_sk, w_sn, d = lm
            check(lib().tmi_linear_xent_weighted(x.data_ptr(), x_ld, w.data_ptr(), w_sk, w_sn, d, logits.data_ptr(), ld,
                                                 labels.data_ptr(), row_w.data_ptr(), inv_wsum.data_ptr(), row_loss.data_ptr(), B, S,
                                                 V, loss_scale, dt(logits), stream()), "tmi_linear_xent_weighted")


def _lm_head_argmax(cons, x, x_ld, w, w_ld, M, d, V, ids, ids_ld, workspace, gamma, beta, eps, eos_id, eos_count):
    """The one marshalling of tmi_lm_head_argmax and, with ``cons`` = (seen, banned, penalty), of tmi_lm_head_argmax_c: the
    _c entry point takes the same arguments with the constraint's four in front of the stream."""
    c = cons is not None
    tail = _cons_tail(cons, M, V) if c else ()
    with _probe("lm_head_argmax_c" if c else "lm_head_argmax", float(d) * w_ld * w.element_size()):
        check((lib().tmi_lm_head_argmax_c if c else lib().tmi_lm_head_argmax)(
            x.data_ptr(), x_ld, dt(x), ptr(gamma), ptr(beta), eps, w.data_ptr(), w_ld, dt(w), M, d, V, ids.data_ptr(), ids_ld,
            eos_id, ptr(eos_count), workspace.data_ptr(), workspace.numel() * workspace.element_size(), *tail, stream()),
            "tmi_lm_head_argmax_c" if c else "tmi_lm_head_argmax")


def lm_head_argmax(x, x_ld, w, w_ld, M, d, V, ids, ids_ld, workspace, gamma=None, beta=None, eps=1e-5, eos_id=-1,
                   eos_count=None):
    """ids[r * ids_ld] = argmax_{n < V} (LayerNorm(x[r]) . w)[n] for M rows of x (row stride x_ld), w the LM head in its
    stored [d, w_ld] layout (fp32 arena or bf16 mirror); eos_count[0] = how many of them equal eos_id.  ``workspace``: an
    int64 tensor of >= M + 1 elements, zero before the first call (tmi_lm_head_argmax leaves it zero)."""
    _lm_head_argmax(None, x, x_ld, w, w_ld, M, d, V, ids, ids_ld, workspace, gamma, beta, eps, eos_id, eos_count)


def lm_head_topk_workspace_elems(M, V, N):
    """int64 elements of tmi_lm_head_topk's workspace: 8 * M * (1 + ceil(V / 128) * (N + 1)) bytes."""
    return M * (1 + (V + 127) // 128 * (N + 1))


def _lm_head_topk(cons, x, x_ld, w, w_ld, M, d, V, N, ids, logprobs, workspace, gamma, beta, eps, temperature, lse):
    """The one marshalling of tmi_lm_head_topk / tmi_lm_head_topk_c (as ``_lm_head_argmax``)."""
    c = cons is not None
    tail = _cons_tail(cons, M, V) if c else ()
    with _probe("lm_head_topk_c" if c else "lm_head_topk", float(d) * w_ld * w.element_size()):
        check((lib().tmi_lm_head_topk_c if c else lib().tmi_lm_head_topk)(
            x.data_ptr(), x_ld, dt(x), ptr(gamma), ptr(beta), eps, w.data_ptr(), w_ld, dt(w), M, d, V, 1.0 / float(temperature), N,
            ids.data_ptr(), logprobs.data_ptr(), ptr(lse), workspace.data_ptr(), workspace.numel() * workspace.element_size(),
            *tail, stream()), "tmi_lm_head_topk_c" if c else "tmi_lm_head_topk")


def lm_head_topk(x, x_ld, w, w_ld, M, d, V, N, ids, logprobs, workspace, gamma=None, beta=None, eps=1e-5,
                 temperature=1.0, lse=None):
    """Per row r of M rows of x (row stride x_ld): s = (LayerNorm(x[r]) . w)[:V] / temperature; ids[r, :N] the N largest
    columns of s (ties: the smaller column first), logprobs[r, :N] their s - logsumexp(s) (fp32), lse[r] the logsumexp.
    ``ids`` int32 and ``logprobs`` fp32 are contiguous [M, N].  ``workspace``: an int64 tensor of at least
    ``lm_head_topk_workspace_elems(M, V, N)`` elements, zero before the first call (tmi_lm_head_topk leaves it zero)."""
    _lm_head_topk(None, x, x_ld, w, w_ld, M, d, V, N, ids, logprobs, workspace, gamma, beta, eps, temperature, lse)


def lm_head_sample_workspace_elems(M, V, top_k):
    """int64 elements of tmi_lm_head_sample's workspace (tmi_lm_head_sample_workspace_bytes / 8)."""
    n = lib().tmi_lm_head_sample_workspace_bytes(M, V, top_k)
    if n < 0:
        raise ValueError(f"tmi_lm_head_sample takes no M {M}, V {V}, top_k {top_k}")
    return n // 8


def _lm_head_sample(cons, x, x_ld, w, w_ld, M, d, V, ids, ids_ld, finished, n_finished, workspace, temperature, top_k, top_p,
                    seed, suppress_id, eos_id, pad_id, logprob, gamma, beta, eps):
    """The one marshalling of tmi_lm_head_sample / tmi_lm_head_sample_c (as ``_lm_head_argmax``)."""
    c = cons is not None
    tail = _cons_tail(cons, M, V) if c else ()
    with _probe("lm_head_sample_c" if c else "lm_head_sample", float(d) * w_ld * w.element_size()):
        check((lib().tmi_lm_head_sample_c if c else lib().tmi_lm_head_sample)(
            x.data_ptr(), x_ld, dt(x), ptr(gamma), ptr(beta), eps, w.data_ptr(), w_ld, dt(w), M, d, V, float(temperature),
            int(top_k), float(top_p), int(seed) & 0xFFFFFFFFFFFFFFFF, suppress_id, eos_id, pad_id, finished.data_ptr(),
            ids.data_ptr(), ids_ld, ptr(logprob), n_finished.data_ptr(), workspace.data_ptr(),
            workspace.numel() * workspace.element_size(), *tail, stream()),
            "tmi_lm_head_sample_c" if c else "tmi_lm_head_sample")


def lm_head_sample(x, x_ld, w, w_ld, M, d, V, ids, ids_ld, finished, n_finished, workspace, temperature=1.0, top_k=50,
                   top_p=1.0, seed=0, suppress_id=-1, eos_id=-1, pad_id=0, logprob=None, gamma=None, beta=None, eps=1e-5):
    """One sampled token per row of M rows of x (row stride x_ld): ids[r * ids_ld] drawn from softmax((LayerNorm(x[r]) . w)
    [:V] / temperature) cut to its ``top_k`` largest columns and their ``top_p`` nucleus (top_k 0: the whole vocabulary,
    Gumbel-max), logprob[r] = its log-probability under the uncut distribution; the rule is include/tethys_mi.h's.
    ``finished`` int32 [M] in and out, ``n_finished`` int32 [1]; ``workspace``: an int64 tensor of at least
    ``lm_head_sample_workspace_elems(M, V, top_k)`` elements, zero before the first call (left zero by every call)."""
    _lm_head_sample(None, x, x_ld, w, w_ld, M, d, V, ids, ids_ld, finished, n_finished, workspace, temperature, top_k, top_p,
                    seed, suppress_id, eos_id, pad_id, logprob, gamma, beta, eps)


def constraint_words(V: int) -> int:
    """uint32 words per row of a decode-constraint bit set over V columns (column n: bit n & 31 of word n >> 5)."""
    return (int(V) + 31) // 32


def _bits(t, rows, V, what):
    if t is None:
        return None, 0
    if t.dtype != torch.int32 or t.dim() != 2 or t.shape[0] < rows or t.stride(1) != 1 or t.shape[1] < constraint_words(V):
        raise ValueError(f"{what} must be an int32 [>= {rows}, >= {constraint_words(V)}] bit set with unit column stride")
    return t, t.stride(0)


def _cons_args(seen, banned, rows, V):
    seen, ld_s = _bits(seen, rows, V, "seen")
    banned, ld_b = _bits(banned, rows, V, "banned")
    if seen is not None and banned is not None and ld_s != ld_b:
        raise ValueError("seen and banned must share their row stride")
    return ptr(seen), ptr(banned), ld_s or ld_b


def _cons_tail(cons, rows, V):
    """``cons`` = (seen, banned, penalty) -> the four trailing arguments of a _c LM head."""
    return (*_cons_args(cons[0], cons[1], rows, V), float(cons[2]))


def decode_constraints(prefix, ld, M, t, V, seen, banned, ngram=0, static_banned=None):
    """The two bit sets of the constrained LM heads for M rows (tmi_decode_constraints; the rule is include/tethys_mi.h's):
    ``seen[r]`` = the tokens in prefix[r, :t], ``banned[r]`` = ``static_banned`` plus the tokens that would complete an
    ``ngram``-gram the prefix already holds (0: none).  ``prefix`` int32 with row stride ``ld``; ``seen`` and ``banned``
    int32 [M, >= constraint_words(V)] of one row stride, every word of [:, :constraint_words(V)] written;
    ``static_banned`` int32 [constraint_words(V)] or None."""
    sp, bp, bits_ld = _cons_args(seen, banned, M, V)
    if sp is None or bp is None:
        raise ValueError("decode_constraints writes both seen and banned")
    if static_banned is not None and (static_banned.dtype != torch.int32 or not static_banned.is_contiguous()
                                      or static_banned.numel() < constraint_words(V)):
        raise ValueError(f"static_banned must be a contiguous int32 tensor of >= {constraint_words(V)} words")
    check(lib().tmi_decode_constraints(prefix.data_ptr(), ld, M, t, V, ptr(static_banned), int(ngram), sp, bp, bits_ld,
                                       stream()), "tmi_decode_constraints")


def lm_head_argmax_c(x, x_ld, w, w_ld, M, d, V, ids, ids_ld, workspace, seen=None, banned=None, penalty=1.0, gamma=None,
                     beta=None, eps=1e-5, eos_id=-1, eos_count=None):
    """``lm_head_argmax`` over the constrained logits z' (include/tethys_mi.h, "Decode constraints"): a column whose bit
    is set in ``banned[r]`` is -inf, one set in ``seen[r]`` is divided (z > 0) or multiplied (z <= 0) by ``penalty``.
    ``seen`` / ``banned``: int32 [M, >= constraint_words(V)] bit sets or None (empty); the workspace is lm_head_argmax's."""
    _lm_head_argmax((seen, banned, penalty), x, x_ld, w, w_ld, M, d, V, ids, ids_ld, workspace, gamma, beta, eps, eos_id,
                    eos_count)


def lm_head_topk_c(x, x_ld, w, w_ld, M, d, V, N, ids, logprobs, workspace, seen=None, banned=None, penalty=1.0, gamma=None,
                   beta=None, eps=1e-5, temperature=1.0, lse=None):
    """``lm_head_topk`` over the constrained logits z' (as ``lm_head_argmax_c``): s = z' / temperature, the logsumexp over
    the columns that are not banned, a banned column's log-probability -inf; the workspace is lm_head_topk's."""
    _lm_head_topk((seen, banned, penalty), x, x_ld, w, w_ld, M, d, V, N, ids, logprobs, workspace, gamma, beta, eps,
                  temperature, lse)


def lm_head_sample_c(x, x_ld, w, w_ld, M, d, V, ids, ids_ld, finished, n_finished, workspace, seen=None, banned=None,
                     penalty=1.0, temperature=1.0, top_k=50, top_p=1.0, seed=0, suppress_id=-1, eos_id=-1, pad_id=0,
                     logprob=None, gamma=None, beta=None, eps=1e-5):
    """``lm_head_sample`` over the constrained logits z' (as ``lm_head_argmax_c``): a banned column is one more
    suppressed id and the candidates are ranked on z'; the workspace is lm_head_sample's."""
    _lm_head_sample((seen, banned, penalty), x, x_ld, w, w_ld, M, d, V, ids, ids_ld, finished, n_finished, workspace,
                    temperature, top_k, top_p, seed, suppress_id, eos_id, pad_id, logprob, gamma, beta, eps)


def timestamp_rules(prefix, ld, M, t, P, V, tb, banned, no_timestamps_id=-1, eos_id=-1, max_initial=-1, max_ts=1500):
    """Rules a - f of the timestamp grammar (tmi_timestamp_rules; include/tethys_mi.h, "Timestamp rules") OR-ed into
    ``banned`` int32 [M, >= constraint_words(V)] for M rows: ``prefix`` int32 with row stride ``ld``, columns [0, t) read, P
    prompt tokens behind the start token; ``tb`` the first timestamp id; ``max_initial`` (< 0: no cap) and ``max_ts`` in
    timestamp units."""
    _, bp, bits_ld = _cons_args(None, banned, M, V)
    if bp is None:
        raise ValueError("timestamp_rules writes banned")
    check(lib().tmi_timestamp_rules(prefix.data_ptr(), ld, M, t, P, V, tb, int(no_timestamps_id), int(eos_id), int(max_initial),
                                    int(max_ts), bp, bits_ld, stream()), "tmi_timestamp_rules")


def lm_head_timestamp_gate_workspace_elems(M, V):
    """int64 elements of tmi_lm_head_timestamp_gate's workspace (tmi_lm_head_timestamp_gate_workspace_bytes / 8)."""
    n = lib().tmi_lm_head_timestamp_gate_workspace_bytes(M, V)
    if n < 0:
        raise ValueError(f"tmi_lm_head_timestamp_gate takes no M {M}, V {V}")
    return n // 8


def lm_head_timestamp_gate(x, x_ld, w, w_ld, M, d, V, tb, fired, workspace, seen=None, banned=None, penalty=1.0, gamma=None,
                           beta=None, eps=1e-5):
    """Rule g of the timestamp grammar (tmi_lm_head_timestamp_gate): over the constrained logits z' of ``lm_head_argmax_c``,
    fired[r] = logsumexp(z' over the timestamp columns [tb, V)) > max(z' over the columns [0, tb)), banned columns left out;
    where it fired the columns [0, tb) are OR-ed into ``banned[r]``.  ``fired`` int32 [M]; ``workspace``: an int64 tensor
    of at least ``lm_head_timestamp_gate_workspace_elems(M, V)`` elements, 16-byte aligned, zero before the first call (left
    zero by every call)."""
    sp, bp, bits_ld = _cons_args(seen, banned, M, V)
    if bp is None:
        raise ValueError("lm_head_timestamp_gate writes banned")
    with _probe("lm_head_timestamp_gate", float(d) * w_ld * w.element_size()):
        check(lib().tmi_lm_head_timestamp_gate(
            x.data_ptr(), x_ld, dt(x), ptr(gamma), ptr(beta), eps, w.data_ptr(), w_ld, dt(w), M, d, V, sp, bp, bits_ld,
            float(penalty), tb, fired.data_ptr(), workspace.data_ptr(), workspace.numel() * workspace.element_size(), stream()),
            "tmi_lm_head_timestamp_gate")


def beam_step(cand_ids, cand_lp, N, B, K, sums, cur, nxt, ld, t, eos_id, len_pow, early_stopping, pool_ids, pool_scores,
              pool_len, pool_cnt, done, done_count, finalize=False):
    """One step of beam search's bookkeeping on the device (tmi_beam_step; the rule is whisper.generate's): candidates
    [B*K, N] -> the next prefix rows ``nxt`` [B*K, ld], the running ``sums``, the pool [B, K(, ld)], the done flags and
    ``done_count``.  ``len_pow`` = t ** length_penalty as an fp32 value.  ``finalize``: offer the live beams of the items
    not done (prefix rows ``cur`` of length t) to their pools instead; the candidates and ``nxt`` are not read."""
    check(lib().tmi_beam_step(ptr(cand_ids), ptr(cand_lp), N, B, K, sums.data_ptr(), cur.data_ptr(), ptr(nxt), ld, t, eos_id,
                              len_pow, 1 if early_stopping else 0, pool_ids.data_ptr(), pool_scores.data_ptr(),
                              pool_len.data_ptr(), pool_cnt.data_ptr(), done.data_ptr(), done_count.data_ptr(),
                              1 if finalize else 0, stream()), "tmi_beam_step")


def logprob_chunk_cols() -> int:
    """The chunk width of the chunked LM head (tmi_logprob_chunk_cols)."""
    return int(lib().tmi_logprob_chunk_cols())


def logprob_state_elems(M: int) -> int:
    """int64 elements of tmi_logprob_fold's state for M rows (tmi_logprob_state_bytes / 8)."""
    n = int(lib().tmi_logprob_state_bytes(M))
    if n < 0:
        raise ValueError(f"tmi_logprob_fold takes no M {M}")
    return n // 8


def logprob_chunks(V: int, ld: int, nc: int):
    """The chunk schedule of a [*, ld] LM head with V real columns at chunk width ``nc``: [(col0, ncols)] in ascending col0,
    ncols = min(nc, ld - col0) the columns the GEMM writes (pad columns of the last chunk included; the fold cuts them at V).
    The real columns [col0, min(col0 + ncols, V)) tile [0, V) exactly once."""
    if V < 1 or ld < V or nc < 1:
        raise ValueError("logprob_chunks: need 1 <= V <= ld and nc >= 1")
    return [(c0, min(nc, ld - c0)) for c0 in range(0, V, nc)]


def check_targets(targets, V: int):
    """Host check of a target tensor (one device read): every entry in [-1, V)."""
    if targets.numel():
        lo, hi = int(targets.min()), int(targets.max())
        if lo < -1 or hi >= V:
            raise ValueError(f"targets must be in [-1, {V}) (-1: row not scored); got [{lo}, {hi}]")


def logprob_fold(chunk, ld, M, V, col0, ncols, targets, state, first, last, lse=None, logprob=None, argmax=None, lm=None,
                 validate=True):
    """One chunk of the chunked log-softmax / argmax / target log-prob (tmi_logprob_fold in include/tethys_mi.h): ``chunk``
    holds the logit columns [col0, col0 + ncols) of M rows at row stride ``ld``; ``state`` an int64 tensor of at least
    ``logprob_state_elems(M)`` elements (any contents); ``lm = (x, x_ld, w, w_sk, w_sn, d)``: the bf16 operands the chunk
    was computed from (the target logit is then recomputed in fp32).  ``validate``: on the first chunk, check on the host
    that the targets are in [-1, V) - the library cannot see them - and raise before anything is launched."""
    if targets.dtype != torch.int32 or not targets.is_contiguous() or targets.numel() < M:
        raise ValueError("logprob_fold: targets must be a contiguous int32 tensor of M entries")
    for t, want in ((lse, torch.float32), (logprob, torch.float32), (argmax, torch.int32)):
        if t is not None and (t.dtype != want or not t.is_contiguous() or t.numel() < M):
            raise ValueError("logprob_fold: lse / logprob float32 and argmax int32, contiguous, M entries")
    if validate and first:
        check_targets(targets[:M], V)
    x, x_ld, w, w_sk, w_sn, d = lm if lm is not None else (None, 0, None, 0, 0, 0)
    if lm is not None and chunk.dtype == torch.bfloat16 and (x.dtype != torch.bfloat16 or w.dtype != torch.bfloat16):
        raise TypeError("logprob_fold: the operands of a bf16 chunk must be bf16")
    with _probe("logprob_fold", 1.0 * M * ncols * chunk.element_size()):
        check(lib().tmi_logprob_fold(chunk.data_ptr(), ld, dt(chunk), M, V, col0, ncols, targets.data_ptr(), ptr(x), x_ld, ptr(w),
                                     w_sk, w_sn, d, state.data_ptr(), state.numel() * state.element_size(), 1 if first else 0,
                                     1 if last else 0, ptr(lse), ptr(logprob), ptr(argmax), stream()), "tmi_logprob_fold")


def logprob_from_logits(logits, V, targets, state, lse, logprob, argmax, nc=None, lm=None, validate=True):
    """A testing hook, not part of the evaluation path (``evaluate`` / ``score`` never hold whole logits): tmi_logprob_fold
    over a materialised ``logits`` [M, ld] (row stride ld, V real columns), chunk by chunk in place, so that a test can hand
    the kernel logits it wrote itself."""
    M, ld = logits.shape[0], logits.stride(0)
    sched = logprob_chunks(V, ld, nc or logprob_chunk_cols())
    for i, (c0, n) in enumerate(sched):
        logprob_fold(logits[:, c0:], ld, M, V, c0, n, targets, state, i == 0, i == len(sched) - 1, lse, logprob, argmax,
                     lm=lm, validate=validate)


def sum_scale(x, out, n, scale):
    check(lib().tmi_sum_scale(x.data_ptr(), out.data_ptr(), n, scale, stream()), "tmi_sum_scale")


def sum_scale_dev(x, out, n, scale):
    """out[0] = sum(x[:n]) * scale[0], ``sum_scale`` with the scale in device memory (a 1-element float32 tensor)."""
    _f32_flat(scale, 1, "sum_scale_dev: scale")
    check(lib().tmi_sum_scale_dev(x.data_ptr(), out.data_ptr(), n, scale.data_ptr(), stream()), "tmi_sum_scale_dev")


def adam_step(p, g, m, v, n, lr, beta1, beta2, eps, step, eps_mode=0, weight_decay=0.0, gscale=1.0, mirror=None,
              zero_grad=False, max_blocks=0):
    with _probe("adam", (28.0 + (2.0 if mirror is not None else 0.0)) * n):
        check(lib().tmi_adam_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, lr, beta1, beta2,
                                  eps, step, eps_mode, weight_decay, gscale, ptr(mirror), 1 if zero_grad else 0,
                                  max_blocks, stream()), "tmi_adam_step")


def segment_chunks(seg_off, chunk=8192, device=None):
    """(lo, hi, variable) pieces of at most ``chunk`` elements that tile the variables of ``seg_off`` (a host list or
    tensor of nseg + 1 element offsets): the table tmi_adam_step_segments walks."""
    offs = [int(x) for x in (seg_off.tolist() if hasattr(seg_off, "tolist") else seg_off)]
    rows = []
    for s_, (lo, hi) in enumerate(zip(offs[:-1], offs[1:])):
        a = lo
        while a < hi:
            b = min(hi, a + chunk)
            rows.append((a, b, s_))
            a = b
    return torch.tensor(rows, dtype=torch.int64, device=device).reshape(-1, 3)


def adam_step_segments(p, g, m, v, n, chunks, sumsq, nseg, clip_global, clip_each, lr, beta1, beta2, eps, step, eps_mode=0,
                       weight_decay=0.0, gscale=1.0, mirror=None, zero_grad=False, max_blocks=0):
    """``chunks`` may be a row range of the model's table (absolute arena offsets): the same update, restricted to those rows;
    ``n`` = the elements they cover (probe accounting only)."""
    with _probe("adam", (28.0 + (2.0 if mirror is not None else 0.0)) * n):
        check(lib().tmi_adam_step_segments(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), chunks.data_ptr(),
                                           chunks.shape[0], ptr(sumsq), nseg, clip_global, clip_each, lr, beta1, beta2, eps, step, eps_mode,
                                           weight_decay, gscale, ptr(mirror), 1 if zero_grad else 0, max_blocks, stream()),
              "tmi_adam_step_segments")


def adam_step_rows(p, g, m, v, nrows, row_len, active, lr, beta1, beta2, eps, step, eps_mode=0, gscale=1.0, mirror=None,
                   zero_grad=False):
    """Adam over an embedding table, idle rows skipped (tmi_adam_step_rows).  Its own probe class: the ALGORITHMIC bytes are the
    dense kernel's (28 B/param whatever the kernel skips), but it moves only the rows with a gradient or a
    live moment (known on the device, not here) - bench.py reports the "adam" class from the dense launches (bytes really
    moved) and the algorithmic figure, rows included, beside it."""
    with _probe("adam_rows", (28.0 + (2.0 if mirror is not None else 0.0)) * nrows * row_len):
        check(lib().tmi_adam_step_rows(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), nrows, row_len,
                                       active.data_ptr(), lr, beta1, beta2, eps, step, eps_mode, 0.0, gscale, ptr(mirror),
                                       1 if zero_grad else 0, stream()), "tmi_adam_step_rows")


def adam_scalars(lr, beta1, beta2, step, eps_mode=0, weight_decay=0.0):
    """[step_size, vcorr_inv_sqrt, decay] of one Adam step (host floats, as tmi_adam_step derives them)."""
    out = (C.c_float * 3)()
    check(lib().tmi_adam_scalars(lr, beta1, beta2, step, eps_mode, weight_decay, C.cast(out, C.c_void_p)), "tmi_adam_scalars")
    return [out[0], out[1], out[2]]


def adam_step_dev(p, g, m, v, n, beta1, beta2, eps, dev_scalars, eps_mode=0, gscale=1.0, mirror=None):
    check(lib().tmi_adam_step_dev(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, beta1, beta2, eps,
                                  dev_scalars.data_ptr(), eps_mode, gscale, ptr(mirror), stream()), "tmi_adam_step_dev")


def grad_pack(src, dst, n, scale=1.0):
    check(lib().tmi_grad_pack(src.data_ptr(), dst.data_ptr(), n, scale, stream()), "tmi_grad_pack")


def grad_unpack(src, dst, n, nparts=1, part_stride=0, scale=1.0):
    check(lib().tmi_grad_unpack(src.data_ptr(), dt(src), nparts, part_stride, dst.data_ptr(), n, scale, stream()),
          "tmi_grad_unpack")


def cast_bf16(src, lds, dst, ldd, rows, cols, src_off=0, dst_off=0):
    check(lib().tmi_cast_bf16(src.data_ptr() + 4 * src_off, lds, dst.data_ptr() + 2 * dst_off, ldd, rows, cols,
                              stream()), "tmi_cast_bf16")


def transpose_cast_bf16(src, lds, dst, ldd, rows, cols, src_off=0, dst_off=0):
    check(lib().tmi_transpose_cast_bf16(src.data_ptr() + 4 * src_off, lds, dst.data_ptr() + 2 * dst_off, ldd,
                                        rows, cols, stream()), "tmi_transpose_cast_bf16")


def feat_to_channels_last(feats, out, B, Cn, T, pad_left, pad_right):
    check(lib().tmi_feat_to_channels_last(feats.data_ptr(), out.data_ptr(), B, Cn, T, pad_left, pad_right,
                                          dt(out), stream()), "tmi_feat_to_channels_last")


def sumsq(x, out, n, accumulate=False):
    check(lib().tmi_sumsq(x.data_ptr(), out.data_ptr(), n, 1 if accumulate else 0, stream()), "tmi_sumsq")


# ---------------------------------------------------------------- Wav2Vec2 operators
def groupnorm_chunks(T: int) -> int:
    return int(lib().tmi_groupnorm_chunks(T))


def groupnorm_gelu_fwd(x, x_sb, gamma, beta, y, y_sb, stats, part, B, T, Cn, G, eps=1e-5, x_off=0, y_off=0):
    # algorithmic bytes: statistics need the whole (time, C/G) slab before any output, so 2 reads + 1 write
    with _probe("groupnorm", 3.0 * B * T * Cn * x.element_size()):
        check(lib().tmi_groupnorm_gelu_fwd(x.data_ptr() + x_off * x.element_size(), x_sb, gamma.data_ptr(), beta.data_ptr(),
                                           y.data_ptr() + y_off * y.element_size(), y_sb, stats.data_ptr(), part.data_ptr(),
                                           B, T, Cn, G, eps, dt(x), stream()), "tmi_groupnorm_gelu_fwd")
    return
    check(lib().tmi_groupnorm_gelu_fwd(x.data_ptr() + x_off * x.element_size(), x_sb, gamma.data_ptr(), beta.data_ptr(),
                                       y.data_ptr() + y_off * y.element_size(), y_sb, stats.data_ptr(), part.data_ptr(),
                                       B, T, Cn, G, eps, dt(x), stream()), "tmi_groupnorm_gelu_fwd")


def groupnorm_gelu_bwd(x, x_sb, dy, dy_sb, gamma, beta, stats, dx, dx_sb, dgamma, dbeta, part, sums, B, T, Cn, G,
                       x_off=0, dy_off=0, dx_off=0):
    es = x.element_size()
    # algorithmic bytes: x and dy are each read twice (sums, then dx), dx written once
    with _probe("groupnorm", 5.0 * B * T * Cn * es):
        check(lib().tmi_groupnorm_gelu_bwd(x.data_ptr() + x_off * es, x_sb, dy.data_ptr() + dy_off * es, dy_sb,
                                           gamma.data_ptr(), beta.data_ptr(), stats.data_ptr(),
                                           dx.data_ptr() + dx_off * es, dx_sb, dgamma.data_ptr(), dbeta.data_ptr(),
                                           part.data_ptr(), sums.data_ptr(), B, T, Cn, G, dt(x), stream()),
              "tmi_groupnorm_gelu_bwd")
    return
    check(lib().tmi_groupnorm_gelu_bwd(x.data_ptr() + x_off * es, x_sb, dy.data_ptr() + dy_off * es, dy_sb,
                                       gamma.data_ptr(), beta.data_ptr(), stats.data_ptr(),
                                       dx.data_ptr() + dx_off * es, dx_sb, dgamma.data_ptr(), dbeta.data_ptr(),
                                       part.data_ptr(), sums.data_ptr(), B, T, Cn, G, dt(x), stream()),
          "tmi_groupnorm_gelu_bwd")


def fir_chunks(T: int) -> int:
    return int(lib().tmi_fir_chunks(T))


def fir_gn_workspace_floats(B, T, Cn):
    return int(lib().tmi_fir_gn_workspace_floats(B, T, Cn))


def fir_groupnorm_gelu_fwd(audio, pad_left, w, k, stride, gamma, beta, y, y_sb, stats, part, B, T, Cn, G, eps=1e-5, y_off=0):
    """Conv layer 0 as a filter bank + GroupNorm + GELU (tmi_fir_groupnorm_gelu_fwd): audio fp32 [B, Tin]."""
    # algorithmic bytes: the output written once (the audio is ~1/250 of it)
    with _probe("groupnorm", 1.0 * B * T * Cn * y.element_size()):
        check(lib().tmi_fir_groupnorm_gelu_fwd(audio.data_ptr(), audio.stride(0), audio.shape[1], pad_left, w.data_ptr(), k, stride,
                                               gamma.data_ptr(), beta.data_ptr(), y.data_ptr() + y_off * y.element_size(), y_sb,
                                               stats.data_ptr(), part.data_ptr(), B, T, Cn, G, eps, dt(y), stream()),
              "tmi_fir_groupnorm_gelu_fwd")


def fir_groupnorm_gelu_bwd(audio, pad_left, w, k, stride, dy, dy_sb, gamma, beta, stats, dW, dgamma, dbeta, part, sums, wpart,
                           B, T, Cn, G, dy_off=0):
    with _probe("groupnorm", 2.0 * B * T * Cn * dy.element_size()):  # dy read by both passes
        check(lib().tmi_fir_groupnorm_gelu_bwd(audio.data_ptr(), audio.stride(0), audio.shape[1], pad_left, w.data_ptr(), k, stride,
                                               dy.data_ptr() + dy_off * dy.element_size(), dy_sb, gamma.data_ptr(), beta.data_ptr(),
                                               stats.data_ptr(), dW.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(),
                                               part.data_ptr(), sums.data_ptr(), wpart.data_ptr(), B, T, Cn, G, dt(dy), stream()),
              "tmi_fir_groupnorm_gelu_bwd")


def group_pack(x, xg, B, T, Cn, G, Tp, pad_left):
    check(lib().tmi_group_pack(x.data_ptr(), xg.data_ptr(), B, T, Cn, G, Tp, pad_left, dt(x), stream()), "tmi_group_pack")


def group_unpack(yg, bias, resid, out, B, T, Cn, G, Tp, row_off):
    check(lib().tmi_group_unpack(yg.data_ptr(), ptr(bias), ptr(resid), out.data_ptr(), B, T, Cn, G, Tp, row_off,
                                 dt(out), stream()), "tmi_group_unpack")


def posconv_pack_weights(w, wf, wb, k, Cg, G, w_off=0):
    check(lib().tmi_posconv_pack_weights(w.data_ptr() + 4 * w_off, wf.data_ptr(), wb.data_ptr(), k, Cg, G, dt(wf),
                                         stream()), "tmi_posconv_pack_weights")


def vq_assign(codebook, idx, q, perplexity, rows, G, Nc, gd):
    check(lib().tmi_vq_assign(codebook.data_ptr(), idx.data_ptr(), q.data_ptr(), perplexity.data_ptr(), rows, G, Nc, gd,
                              dt(q), stream()), "tmi_vq_assign")


def vq_nearest(h, codebook, idx, q, perplexity, rows, G, Nc, gd):
    check(lib().tmi_vq_nearest(h.data_ptr(), codebook.data_ptr(), idx.data_ptr(), q.data_ptr(), perplexity.data_ptr(),
                               rows, G, Nc, gd, dt(h), stream()), "tmi_vq_nearest")


def vq_bwd(idx, dq, dcodebook, rows, G, Nc, gd):
    check(lib().tmi_vq_bwd(idx.data_ptr(), dq.data_ptr(), dcodebook.data_ptr(), rows, G, Nc, gd, dt(dq), stream()),
          "tmi_vq_bwd")


def contrastive_fwd_bwd(S, neg, row_loss, B, T, Nn, temperature, grad_scale, per_time=False):
    """``neg`` [B, Nn] (one row of indices per batch row, V:908-937) or, with ``per_time``, [T, Nn] (one row per
    time step shared by the batch, whisper_single.py:789-839)."""
    sb, st = (0, Nn) if per_time else (Nn, 0)
    check(lib().tmi_contrastive_fwd_bwd(S.data_ptr(), neg.data_ptr(), sb, st, row_loss.data_ptr(), B, T, Nn, temperature,
                                        grad_scale, stream()), "tmi_contrastive_fwd_bwd")


def check_negative_indices(neg, T: int):
    """Host check of a negative-index tensor (one device read): every entry in [0, T)."""
    if neg.numel():
        lo, hi = int(neg.min()), int(neg.max())
        if lo < 0 or hi >= T:
            raise ValueError(f"negative indices must be in [0, {T}); got [{lo}, {hi}]")


def contrastive_score(h, q, neg, row_loss, row_correct, B, T, pd, Nn, temperature, mask=None, per_time=False, ld=None,
                      validate=True):
    """Gathered contrastive loss and argmax flag per row (tmi_contrastive_score in include/tethys_mi.h): ``h`` / ``q``
    [B, T, pd] at row stride ``ld`` (default pd), ``neg`` int32 [B, Nn] or, with ``per_time``, [T, Nn]; ``mask`` float32
    [B, T] or None.  ``validate``: check on the host that the indices are in [0, T) - the library cannot see them - and
    raise before anything is launched."""
    ld = pd if ld is None else ld
    if h.dtype != q.dtype:
        raise TypeError("contrastive_score: h and q must have one dtype")
    if neg.dtype != torch.int32 or not neg.is_contiguous() or neg.numel() < (T if per_time else B) * Nn:
        raise ValueError("contrastive_score: neg must be a contiguous int32 tensor of [B, Nn] (per_time: [T, Nn]) entries")
    if mask is not None and (mask.dtype != torch.float32 or not mask.is_contiguous() or mask.numel() < B * T):
        raise ValueError("contrastive_score: mask must be float32 [B, T] contiguous")
    if (row_loss.dtype != torch.float32 or row_correct.dtype != torch.int32 or not row_loss.is_contiguous()
            or not row_correct.is_contiguous() or row_loss.numel() < B * T or row_correct.numel() < B * T):
        raise ValueError("contrastive_score: row_loss float32 and row_correct int32, contiguous, B * T entries")
    if validate:
        check_negative_indices(neg, T)
    sb, st = (0, Nn) if per_time else (Nn, 0)
    with _probe("contrastive_score", 2.0 * B * T * (Nn + 1) * pd):
        check(lib().tmi_contrastive_score(h.data_ptr(), q.data_ptr(), ld, dt(h), neg.data_ptr(), sb, st, ptr(mask),
                                          row_loss.data_ptr(), row_correct.data_ptr(), B, T, pd, Nn, temperature, stream()),
              "tmi_contrastive_score")


def vq_count(idx, mask, counts, rows, G, Nc):
    """counts[g, clamp(idx[r, g])] += 1 over the rows whose mask is > 0 (tmi_vq_count): ``idx`` int32 [rows, G], ``mask``
    float32 [rows] or None, ``counts`` int64 [G, Nc].  ACCUMULATES: zero ``counts`` once per evaluation."""
    if idx.dtype != torch.int32 or not idx.is_contiguous() or idx.numel() < rows * G:
        raise ValueError("vq_count: idx must be a contiguous int32 tensor of rows * G entries")
    if mask is not None and (mask.dtype != torch.float32 or not mask.is_contiguous() or mask.numel() < rows):
        raise ValueError("vq_count: mask must be float32 [rows] contiguous")
    if counts.dtype != torch.int64 or not counts.is_contiguous() or counts.numel() != G * Nc:
        raise ValueError("vq_count: counts must be a contiguous int64 tensor of G * Nc entries")
    check(lib().tmi_vq_count(idx.data_ptr(), ptr(mask), counts.data_ptr(), rows, G, Nc, stream()), "tmi_vq_count")


def segment_sumsq_chunks(g, chunks, out, nseg):
    """Per-variable sums of squares over the chunk table of ``segment_chunks`` (tmi_segment_sumsq_chunks)."""
    check(lib().tmi_segment_sumsq_chunks(g.data_ptr(), chunks.data_ptr(), chunks.shape[0], out.data_ptr(), nseg, stream()),
          "tmi_segment_sumsq_chunks")


def segment_sumsq(g, seg_off, out, nseg):
    check(lib().tmi_segment_sumsq(g.data_ptr(), seg_off.data_ptr(), out.data_ptr(), nseg, stream()), "tmi_segment_sumsq")


def segment_clip(g, seg_off, sumsq, nseg, clip):
    check(lib().tmi_segment_clip(g.data_ptr(), seg_off.data_ptr(), sumsq.data_ptr(), nseg, clip, stream()),
          "tmi_segment_clip")


def loss_combine(a, b, w, scale, out):
    check(lib().tmi_loss_combine(a.data_ptr(), b.data_ptr(), w, scale, out.data_ptr(), stream()), "tmi_loss_combine")
