"""The GEMM form table: every way the training step calls tmi_gemm, at the smallest shape that keeps the form's alignment
class, ragged edges and an odd K-tile count.  One table for the CPU checks of the reference (tests/test_gemm_ref_cpu.py), the
in-process GPU test (tests/test_gemm_forms_gpu.py) and the forced-configuration children (tests/_gemm_forms_child.py).

A case is a list of launches (the arguments of ``ops.gemm`` / ``_gemm_ref.gemm_ref``; ``bias`` / ``aux_in`` / ``resid`` /
``aux_out`` are flags here) over shared flat buffers, the path ``launch_fast`` / ``launch_f32`` / ``gemm.hip::launch`` takes
for it under the library's rules (``expect`` = (kernel, nsplit, flags), see tmi_gemm_last_path) and an independent
float64 formulation (``indep``) of each launch's window.

Buffers (``prepare``): values are drawn in float64 from a seeded generator with a per-row scale spread over 2^6, rounded to
the operand type; every element the contract's formula does not address holds NaN (operands), every element of C and
aux_out is NaN beforehand except C_old where ``accumulate`` is set (or zero where the split-K atomics need a zeroed C).
Every buffer is longer than what is addressed: whole 16-byte chunks plus 64 elements.
"""
import math

import numpy as np

import _gemm_ref as R

GENERIC, F32 = 1, 32                      # TMI_GEMM_KERNEL_*
PERSISTENT, ATOMIC, SLABS, XCD_GROUPS, XCD_DEAL, WIDE = 1, 2, 4, 8, 16, 32   # TMI_GEMM_PATH_*
FORCED = (4, 5, 6, 12, 13, 15, 16, 10, 14)


def rup(x, q):
    return (x + q - 1) // q * q


def _bf16(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(torch.bfloat16).double().numpy()


def _f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def round_to(x, bf16):
    return _bf16(x) if bf16 else _f32(x)


# ---------------------------------------------------------------------------------------------- epilogue, restated
def _t(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x))


def epi_indep(pre, *, bias=None, scale_cols=0, scale=1.0, c_old=None, act=0, aux_in=None, keep=None, keep_scale=1.0,
              resid=None):
    """The documented epilogue order on float64 torch tensors (erf from torch, not from _gemm_ref).  -> (C, aux)."""
    import torch
    v = _t(pre).clone()
    if bias is not None:
        v = v + _t(bias)
    if scale_cols > 0:
        v[..., :scale_cols] = v[..., :scale_cols] * float(np.float32(scale))
    if c_old is not None:
        v = v + _t(c_old)
    aux = v.clone()
    if act == 1:
        v = torch.nn.functional.gelu(v)
    if aux_in is not None:
        u = _t(aux_in)
        v = v * (0.5 * (1 + torch.erf(u / math.sqrt(2))) + u * torch.exp(-0.5 * u * u) / math.sqrt(2 * math.pi))
    if keep is not None:
        v = v * _t(keep) * keep_scale
    if resid is not None:
        v = v + _t(resid)
    return v.numpy(), aux.numpy()


# ---------------------------------------------------------------------------------------------- the table
CASES = []


def _add(name, launches, indep, *, in_f32=False, out_bf16=True, expect=None, ws=True, zero_c=False, gen="randn",
         a_scale=1.0, b_scale=None, fill=None, deterministic=False, repeat_equal=False, exact=False, site="", children="all", acc_chain=None):
    """``children``: which forced-kernel children run the case too ("all"; "p8": the eight-phase values only; "none": the
    multi-million-element cases that exist for one path of the library's own rules)."""
    if isinstance(launches, dict):
        launches = [launches]
    CASES.append(dict(name=name, launches=launches, indep=indep, in_f32=in_f32, out_bf16=out_bf16, expect=expect, ws=ws,
                      zero_c=zero_c, gen=gen, a_scale=a_scale, b_scale=b_scale, fill=fill, deterministic=deterministic,
                      repeat_equal=repeat_equal, exact=exact, site=site, children=children, acc_chain=acc_chain))


def _win(buf, off, sb, ld, nb, M, N):
    """[nb, M, N] gathered window of a flat buffer, by slicing (independent of _gemm_ref's index arithmetic)."""
    out = np.empty((nb, M, N))
    for b in range(nb):
        if ld >= N:     # rows do not overlap: one strided slice per column block
            out[b] = _pad(buf[off + b * sb:], M * ld).reshape(M, ld)[:, :N]
            continue
        for m in range(M):
            s = off + b * sb + m * ld
            out[b, m] = buf[s:s + N]
    return out


def _pad(buf, n):
    """The first n elements of a flat buffer (NaN where the buffer is shorter: nothing addressed lies there)."""
    if len(buf) >= n:
        return buf[:n]
    return np.concatenate([buf, np.full(n - len(buf), np.nan)])


def _zero_rows(buf, nb, sb, row_len, r0, r1):
    """Zero rows r0 .. r1 - 1 (row_len elements each) of each of nb images sb apart, in place, clipped to the buffer."""
    for b in range(nb):
        lo, hi = b * sb + r0 * row_len, b * sb + r1 * row_len
        buf[min(lo, len(buf)):min(hi, len(buf))] = 0.0


def _keep(L):
    from oracle import dropout as DO
    return DO.keep_flat(L["dropout_seed"], L["M"], L["N"], L["dropout_p"]).astype(np.float64), float(DO.keep_scale(L["dropout_p"]))


def _epi_from(L, bufs, pre):
    """Independent epilogue of launch L on pre [nb, M, N] (one batch level)."""
    nb, M, N = pre.shape
    kw = dict(scale_cols=L.get("scale_cols", 0), scale=L.get("scale", 1.0), act=L.get("act", 0))
    if L.get("bias"):
        bo = L.get("bias_off", 0)
        kw["bias"] = np.stack([bufs["bias"][bo + b * L.get("bias_sb", 0):][:N] for b in range(nb)])[:, None, :]
    if L.get("accumulate"):
        kw["c_old"] = _win(bufs["C"], L.get("c_off", 0), L.get("c_sb", 0), L["ldc"], nb, M, N)
    if L.get("aux_in"):
        kw["aux_in"] = _win(bufs["aux_in"], L.get("c_off", 0), L.get("c_sb", 0), L["ldc"], nb, M, N)
    if L.get("dropout_p", 0.0) > 0:
        k, s = _keep(L)
        kw["keep"], kw["keep_scale"] = k[None], s
    if L.get("resid"):
        kw["resid"] = _win(bufs["resid"], 0, L.get("r_sb", 0), L["r_ld"], nb, M, N)
    return epi_indep(pre, **kw)


# --- 1. Linear forward (blocks.py _gemm_xw): A k-contiguous, B = [K, ldw] with ldw > N and b_off selecting a column block
def _linear(name, epi, *, M=200, N=108, K=576, ld_a=584, ldw=264, n_off=64, ldc=120, expect=(15, 1, WIDE), **kw):
    L = dict(M=M, N=N, K=K, a_sm=ld_a, a_sk=1, b_sk=ldw, b_sn=1, ldc=ldc, b_off=n_off, **epi)

    def indep(bufs, L=L):
        A = _pad(bufs["A"], M * ld_a).reshape(M, ld_a)[:, :K]
        W = _pad(bufs["B"], K * ldw).reshape(K, ldw)[:, n_off:n_off + N]
        return [_epi_from(L, bufs, (_t(A) @ _t(W)).numpy()[None])]
    _add(name, L, indep, b_scale=1.0 / math.sqrt(K), expect=expect, site="blocks.py _gemm_xw", **kw)


_linear("linear_bias", dict(bias=True))
_linear("linear_gelu_aux", dict(bias=True, act=1, aux_out=True))
_linear("linear_scale64", dict(bias=True, scale_cols=64, scale=0.125))
_linear("linear_scale72", dict(bias=True, scale_cols=72, scale=0.125))
_linear("linear_scale100", dict(bias=True, scale_cols=100, scale=0.125))
_linear("linear_drop_resid", dict(bias=True, dropout_p=0.1, dropout_seed=1234, resid=True, r_ld=136))
_linear("linear_gelu_aux_resid", dict(bias=True, act=1, aux_out=True, resid=True, r_ld=136))
# an unaligned bias pointer (4 bytes off) and an unaligned c_off: the element epilogue (no WIDE flag)
_linear("linear_unaligned_bias_c", dict(bias=True, bias_off=1, c_off=3), expect=(15, 1, 0))
# K = 192: below the K-groups' threshold, the plain four-wave 64x64 tile
_linear("linear_shortk_bias", dict(bias=True), K=192, ld_a=200, expect=(12, 1, WIDE))


# more than one 64x64 tile per CU, up to two (Whisper-large's decoder): the K-groups on 2-stage rings; odd trip count (17)
_linear("linear_decoder_large_ring2", dict(bias=True), M=790, N=1304, K=1088, ld_a=1096, ldw=1312, n_off=0, ldc=1304,
        expect=(16, 1, WIDE))


# --- 2. Dgrad (blocks.py dgrad): dy [M, ld_dy] x W^T, W = [K_in, ldw] read k-contiguously (b_sn = ldw), ldc > N
def _dgrad(name, epi, *, M=200, N=108, K=192, ld_dy=200, ldw=208, ldc=120, expect=(12, 1, WIDE)):
    L = dict(M=M, N=N, K=K, a_sm=ld_dy, a_sk=1, b_sk=1, b_sn=ldw, ldc=ldc, **epi)

    def indep(bufs, L=L):
        A = _pad(bufs["A"], M * ld_dy).reshape(M, ld_dy)[:, :K]
        W = _pad(bufs["B"], N * ldw).reshape(N, ldw)[:, :K]
        return [_epi_from(L, bufs, (_t(A) @ _t(W).t()).numpy()[None])]
    _add(name, L, indep, b_scale=1.0 / math.sqrt(K), expect=expect, site="blocks.py dgrad")


_dgrad("dgrad_acc", dict(accumulate=True))
_dgrad("dgrad_auxin", dict(aux_in=True))
_dgrad("dgrad_acc_auxin", dict(accumulate=True, aux_in=True))


# --- 3. Wav2Vec2 fused QKV (wav2vec2.py): three [H, H] kernels, column-block outputs; its dgrad walks three K batches
def _w2v_qkv():
    Rr, H = 136, 128
    L = dict(M=Rr, N=H, K=H, a_sm=H, a_sk=1, b_sk=H, b_sn=1, ldc=3 * H, nbatch=3, b_sb=H * H, c_sb=H, bias=True, bias_sb=H)

    def indep(bufs):
        x = _t(_pad(bufs["A"], Rr * H).reshape(Rr, H))
        w = _t(_pad(bufs["B"], 3 * H * H).reshape(3, H, H))
        pre = np.stack([(x @ w[j]).numpy() for j in range(3)])
        return [_epi_from(L, bufs, pre)]
    _add("w2v_qkv_fwd", L, indep, b_scale=1.0 / math.sqrt(H), expect=(12, 1, WIDE), site="wav2vec2.py qkv forward")

    L2 = dict(M=Rr, N=H, K=H, a_sm=3 * H, a_sk=1, b_sk=1, b_sn=H, ldc=H, kbatch=3, a_skb=H, b_skb=H * H)

    def indep2(bufs):
        dq = _t(_pad(bufs["A"], Rr * 3 * H).reshape(Rr, 3, H))
        w = _t(_pad(bufs["B"], 3 * H * H).reshape(3, H, H))           # [j][n][k]
        import torch
        return [_epi_from(L2, bufs, torch.einsum("rjk,jnk->rn", dq, w).numpy()[None])]
    _add("w2v_qkv_dgrad", L2, indep2, b_scale=1.0 / math.sqrt(3 * H), expect=(12, 1, WIDE), site="wav2vec2.py qkv dgrad")


_w2v_qkv()


def _qkv_dgrad_large():
    """The qkv dgrad of a long batch: 200 tiles of 128 x 128 (not the small-problem rule), three K batches (not the
    eight-phase kernel), K_total = 1536 into bf16: the 256 x 256 tile."""
    Rr, H, N = 2560, 512, 1280
    L = dict(M=Rr, N=N, K=H, a_sm=3 * H, a_sk=1, b_sk=1, b_sn=H, ldc=N, kbatch=3, a_skb=H, b_skb=N * H)

    def indep(bufs):
        import torch
        dq = _t(_pad(bufs["A"], Rr * 3 * H).reshape(Rr, 3, H))
        w = _t(_pad(bufs["B"], 3 * N * H).reshape(3, N, H))
        return [_epi_from(L, bufs, torch.einsum("rjk,jnk->rn", dq, w).numpy()[None])]
    _add("qkv_dgrad_large_tile256", L, indep, b_scale=1.0 / 40, expect=(5, 1, WIDE), site="wav2vec2.py qkv dgrad, long batch",
         children="none")


_qkv_dgrad_large()


# --- 4. Weight gradients: dW[K_in, N] = X^T dY, both operands k-strided, fp32 out, library-chosen split
def _wgrad(name, *, K_in=136, N=104, T=200, ld_x=None, ld_dy=None, ldc=None, accumulate=False, expect=None, ws=True,
           zero_c=False, gen="randn", deterministic=False, repeat_equal=False, exact=False, splitk=0, in_f32=False,
           children="all", site="blocks.py weight_grads"):
    ld_x = ld_x or rup(K_in, 8)
    ld_dy = ld_dy or rup(N, 8)
    ldc = ldc or N
    L = dict(M=K_in, N=N, K=T, a_sm=1, a_sk=ld_x, b_sk=ld_dy, b_sn=1, ldc=ldc, splitk=splitk, accumulate=accumulate)

    def indep(bufs, L=L):
        X = _pad(bufs["A"], T * ld_x).reshape(T, ld_x)[:, :K_in]
        dY = _pad(bufs["B"], T * ld_dy).reshape(T, ld_dy)[:, :N]
        return [_epi_from(L, bufs, (_t(X).t() @ _t(dY)).numpy()[None])]
    _add(name, L, indep, out_bf16=False, expect=expect, ws=ws, zero_c=zero_c, gen=gen, deterministic=deterministic,
         repeat_equal=repeat_equal, exact=exact, site=site, in_f32=in_f32, children=children)


# 4 K-tiles: its / 4 = 1, no split (and `accumulate` never splits)
_wgrad("wgrad_nosplit", expect=(4, 1, WIDE))
_wgrad("wgrad_nosplit_acc", accumulate=True, expect=(4, 1, WIDE))
# 17 K-tiles (K tail 8): 4 ranges; fewer than 64 K-tiles and / or no workspace: fp32 atomics into a zeroed C
_wgrad("wgrad_atomic_no_workspace", T=1032, ws=False, zero_c=True, expect=(4, 4, ATOMIC | XCD_GROUPS | WIDE))
_wgrad("wgrad_atomic_deterministic", T=1032, ws=False, zero_c=True, deterministic=True, repeat_equal=True,
       expect=(4, 2, ATOMIC | XCD_GROUPS | WIDE))
# 65 K-tiles with a workspace: 8 slabs
_wgrad("wgrad_slabs", T=4104, repeat_equal=True, expect=(4, 8, SLABS | XCD_GROUPS | WIDE))
# N % 4 != 0 with b_sk = round_up(N, 8): the slab reduce's scalar path, element epilogue into the slabs
_wgrad("wgrad_slabs_scalar_reduce", N=106, T=4104, repeat_equal=True, expect=(4, 8, SLABS | XCD_GROUPS))


# the parity mode's weight gradients (fp32 operands, launch_f32): 32 slabs of 32 k, its / 8 = 4 K ranges - through workspace
# slabs, or fp32 atomics into a zeroed C without a workspace
_wgrad("wgrad_f32_slabs", T=1024, in_f32=True, repeat_equal=True, expect=(F32, 4, SLABS | WIDE))
_wgrad("wgrad_f32_atomic_no_workspace", T=1024, in_f32=True, ws=False, zero_c=True, expect=(F32, 4, ATOMIC | WIDE))
# bf16 result of a deep reduction with a K tail (both operands k-strided, K = 1544): the single-group 4-stage ring
_KS_TAIL = dict(M=136, N=104, K=1544, a_sm=1, a_sk=136, b_sk=104, b_sn=1, ldc=104)
_add("kstrided_bf16_deep_k_tail", _KS_TAIL,
     lambda bufs: [((_t(_pad(bufs["A"], 1544 * 136).reshape(1544, 136)).t() @ _t(_pad(bufs["B"], 1544 * 104).reshape(1544, 104))).numpy()[None], None)],
     b_scale=1.0 / 40, expect=(13, 1, WIDE), site="transposed-A product into bf16 (tools, contrastive-style)")


def _wgrad_stacked():
    """Stacked layers (wav2vec2.py qkv weight gradient, blocks.py batched_weight_grads): nbatch = layers, c_sb = the layer
    stride of the gradient arena, b_off / c_off = the j-th of three column blocks."""
    H, T, nl, lstride = 72, 4104, 2, 3 * 72 * 72 + 3 * 72 + 40
    L = dict(M=H, N=H, K=T, a_sm=1, a_sk=H, b_sk=3 * H, b_sn=1, ldc=H, nbatch=nl, a_sb=T * H, b_sb=T * 3 * H, c_sb=lstride,
             b_off=H, c_off=H * H, splitk=0)

    def indep(bufs):
        X = _t(_pad(bufs["A"], nl * T * H).reshape(nl, T, H))
        dY = _t(_pad(bufs["B"], nl * T * 3 * H).reshape(nl, T, 3, H))[:, :, 1]
        import torch
        return [_epi_from(L, bufs, torch.einsum("ltk,ltn->lkn", X, dY).numpy())]
    _add("wgrad_stacked_layers", L, indep, out_bf16=False, repeat_equal=True, expect=(4, 8, SLABS | WIDE),
         site="wav2vec2.py stacked qkv weight gradient")


_wgrad_stacked()


def _wgrad_posconv():
    """Positional conv weight gradient (wav2vec2.py): overlapping k-strided rows of the packed input, ldc = C, c_sb = Cg."""
    Cg, kp, G, B, Tpp = 16, 5, 3, 2, 40
    Mw, C = B * Tpp - (kp - 1), 3 * 16
    L = dict(M=kp * Cg, N=Cg, K=Mw, a_sm=1, a_sk=Cg, b_sk=Cg, b_sn=1, ldc=C, nbatch=G, a_sb=B * Tpp * Cg, b_sb=B * Tpp * Cg,
             c_sb=Cg, splitk=0)

    def indep(bufs):
        import torch
        xg = _t(_pad(bufs["A"], G * B * Tpp * Cg).reshape(G, B * Tpp, Cg))
        dy = _t(_pad(bufs["B"], G * B * Tpp * Cg).reshape(G, B * Tpp, Cg))[:, :Mw]
        win = torch.stack([xg[:, j:j + Mw] for j in range(kp)], dim=2)          # [G, Mw, kp, Cg]
        return [_epi_from(L, bufs, torch.einsum("gtjc,gtn->gjcn", win, dy).reshape(G, kp * Cg, Cg).numpy())]
    _add("wgrad_posconv", L, indep, out_bf16=False, expect=(4, 1, WIDE), site="wav2vec2.py pos-conv weight gradient")


_wgrad_posconv()


# --- 5. Conv1D as GEMM
def _conv_fwd(name, stride):
    """Forward over overlapping rows of the padded channels-last input, nbatch = B, the stem's epilogue: bias + GELU + saved
    pre-activation + a residual shared by the batch (r_sb = 0: the positional encoding), output at a row offset (c_off)."""
    from oracle import whisper_oracle as O
    B, T, Cin, Cout, k = 2, 130, 64, 72, 3
    Tout, pl, pr = O.same_pad(T, k, stride)
    Tp = T + pl + pr
    rows = Tp + 2                                     # the +2-row slack of the conv buffers
    out_rows, pl2 = Tout + 3, 1
    L = dict(M=Tout, N=Cout, K=k * Cin, a_sm=stride * Cin, a_sk=1, b_sk=Cout, b_sn=1, ldc=Cout, nbatch=B, a_sb=rows * Cin,
             c_sb=out_rows * Cout, c_off=pl2 * Cout, bias=True, act=1, aux_out=True, resid=True, r_ld=80, r_sb=0)

    def fill(bufs):                                  # the conv's own zero padding (addressed, so not poison)
        _zero_rows(bufs["A"], B, rows * Cin, Cin, 0, pl)
        _zero_rows(bufs["A"], B, rows * Cin, Cin, pl + T, rows)

    def indep(bufs):
        import torch
        x = _t(_pad(bufs["A"], B * rows * Cin).reshape(B, rows, Cin)[:, pl:pl + T])
        w = _t(_pad(bufs["B"], k * Cin * Cout).reshape(k, Cin, Cout))
        pre = O.conv1d_same(x, w, _t(bufs["bias"][:Cout]), stride)
        res = _t(_win(bufs["resid"], 0, 0, 80, 1, Tout, Cout))
        return [((torch.nn.functional.gelu(pre) + res).numpy(), pre.numpy())]
    _add(name, L, indep, b_scale=1.0 / math.sqrt(k * Cin), fill=fill, expect=(12, 1, WIDE), site="whisper.py conv stem forward")


_conv_fwd("conv_fwd_stride1", 1)
_conv_fwd("conv_fwd_stride2", 2)


def _conv_wgrad():
    """Conv weight gradient (whisper.py conv1 / conv2, wav2vec2.py conv stack): the reduction runs over windows of every
    sample (kbatch = B, a_sk = s * cin), dY sits at a row offset (b_off)."""
    from oracle import whisper_oracle as O
    B, T, cin, c, kc, s = 2, 100, 32, 72, 3, 2
    Ti, pl, pr = O.same_pad(T, kc, s)
    rows, drows = T + pl + pr + 2, Ti + 2
    L = dict(M=kc * cin, N=c, K=Ti, a_sm=1, a_sk=s * cin, b_sk=c, b_sn=1, ldc=c, kbatch=B, a_skb=rows * cin, b_skb=drows * c,
             b_off=c, splitk=0)

    def fill(bufs):
        _zero_rows(bufs["A"], B, rows * cin, cin, 0, pl)
        _zero_rows(bufs["A"], B, rows * cin, cin, pl + T, rows)

    def indep(bufs):
        import torch
        x = _t(_pad(bufs["A"], B * rows * cin).reshape(B, rows, cin)[:, pl:pl + T])
        dy = _t(_pad(bufs["B"], B * drows * c).reshape(B, drows, c)[:, 1:1 + Ti])
        w = torch.zeros(kc, cin, c, dtype=torch.float64, requires_grad=True)
        (O.conv1d_same(x, w, None, s) * dy).sum().backward()
        return [(w.grad.reshape(1, kc * cin, c).numpy(), None)]
    _add("conv_wgrad_kbatch", L, indep, out_bf16=False, fill=fill, expect=(4, 1, WIDE), site="whisper.py / wav2vec2.py conv weight gradient")


_conv_wgrad()


def _conv_dgrad_pair():
    """The stride-2 conv dgrad as two launches into one interleaved buffer (whisper.py conv2, wav2vec2.py conv stack): even
    padded rows take taps 0 and 2 (kbatch = 2, a_skb = -c: the previous output row), odd rows tap 1 (c_off = cin);
    ldc = 2 * cin, aux_in (the GELU of the layer below) shares c_off."""
    from oracle import whisper_oracle as O
    B, Ti, cin, c, ldw = 2, 70, 72, 64, 72
    drows = Ti + 2                                   # row 0: the zero row tap 2 reads for t = 0
    irows = Ti + 2                                   # rows of [2 * cin]: padded input rows 2j, 2j + 1
    base = dict(M=Ti, N=cin, K=c, a_sm=c, a_sk=1, b_sk=1, b_sn=ldw, ldc=2 * cin, nbatch=B, a_sb=drows * c,
                c_sb=irows * 2 * cin, a_off=c, aux_in=True)
    L0 = dict(base, kbatch=2, a_skb=-c, b_skb=2 * cin * ldw)
    L1 = dict(base, b_off=cin * ldw, c_off=cin)

    def fill(bufs):
        _zero_rows(bufs["A"], B, drows * c, c, 0, 1)

    def indep(bufs):
        import torch
        dy = _t(_pad(bufs["A"], B * drows * c).reshape(B, drows, c)[:, 1:1 + Ti])
        w = _t(_pad(bufs["B"], 3 * cin * ldw).reshape(3, cin, ldw)[:, :, :c])
        # the padded input has 2 * Ti + 1 rows: x = rows 1 .. 2 Ti - 1 ... take the gradient with respect to the padded rows
        xp = torch.zeros(B, 2 * Ti + 1, cin, dtype=torch.float64, requires_grad=True)
        y = torch.nn.functional.conv1d(xp.transpose(1, 2), w.permute(2, 1, 0), stride=2).transpose(1, 2)   # [B, Ti, c]
        (y * dy).sum().backward()
        g = xp.grad                                                      # [B, 2 Ti + 1, cin]
        even, odd = g[:, 0:2 * Ti:2], g[:, 1:2 * Ti:2]
        outs = []
        for L, pre in ((L0, even), (L1, odd)):
            outs.append(_epi_from(L, bufs, pre.numpy()))
        return outs
    _add("conv_dgrad_interleaved_pair", [L0, L1], indep, b_scale=1.0 / math.sqrt(2 * c), fill=fill, expect=(12, 1, WIDE),
         site="whisper.py / wav2vec2.py conv dgrad pair")


_conv_dgrad_pair()


# --- 6. Grouped positional conv, forward and dgrad (wav2vec2.py): nbatch = G, overlapping rows, M = B * Tpp - (k - 1)
def _posconv(name, Tpp):
    Cg, kp, G, B = 64, 3, 2, 2
    M = B * Tpp - (kp - 1)
    L = dict(M=M, N=Cg, K=kp * Cg, a_sm=Cg, a_sk=1, b_sk=Cg, b_sn=1, ldc=Cg, nbatch=G, a_sb=B * Tpp * Cg, b_sb=kp * Cg * Cg,
             c_sb=B * Tpp * Cg)

    def indep(bufs):
        import torch
        xg = _t(_pad(bufs["A"], G * B * Tpp * Cg).reshape(G, B * Tpp, Cg))
        w = _t(_pad(bufs["B"], G * kp * Cg * Cg).reshape(G, kp, Cg, Cg))
        win = torch.stack([xg[:, j:j + M] for j in range(kp)], dim=2)          # [G, M, kp, Cg]
        return [_epi_from(L, bufs, torch.einsum("gtjc,gjcn->gtn", win, w).numpy())]
    _add(name, L, indep, b_scale=1.0 / math.sqrt(kp * Cg), expect=(12, 1, WIDE), site="wav2vec2.py grouped pos-conv")


_posconv("posconv_fwd", 35)
_posconv("posconv_dgrad", 37)


# --- 7. Contrastive scores and their gradients (wav2vec2.py): T = 49 is no multiple of 8, dS rows are Tp = 56 apart
def _contrastive():
    import torch  # noqa: F401
    B, T, Tp, pd = 2, 49, 56, 64
    L = dict(M=T, N=T, K=pd, a_sm=pd, a_sk=1, b_sk=1, b_sn=pd, ldc=T, nbatch=B, a_sb=T * pd, b_sb=T * pd, c_sb=T * T)

    def indep(bufs):
        ph = _t(_pad(bufs["A"], B * T * pd).reshape(B, T, pd))
        pq = _t(_pad(bufs["B"], B * T * pd).reshape(B, T, pd))
        return [_epi_from(L, bufs, (ph @ pq.transpose(1, 2)).numpy())]
    _add("contrastive_scores", L, indep, b_scale=0.125, expect=(4, 1, 0), site="wav2vec2.py contrastive scores")

    # dpq = dS^T ph: A k-strided with a_sk = Tp = round_up(T, 8) and M = T columns (M % 8 != 0), K = T (a K tail)
    L2 = dict(M=T, N=pd, K=T, a_sm=1, a_sk=Tp, b_sk=pd, b_sn=1, ldc=pd, nbatch=B, a_sb=T * Tp, b_sb=T * pd, c_sb=T * pd)

    def indep2(bufs):
        dS = _t(_pad(bufs["A"], B * T * Tp).reshape(B, T, Tp)[:, :, :T])
        ph = _t(_pad(bufs["B"], B * T * pd).reshape(B, T, pd))
        return [_epi_from(L2, bufs, (dS.transpose(1, 2) @ ph).numpy())]
    _add("contrastive_dpq_kstrided", L2, indep2, b_scale=0.125, expect=(4, 1, WIDE), site="wav2vec2.py contrastive dpq")

    # dph = dS pq with K = Tp: the pad columns of dS are part of the sum (zero in the step), the rows T .. Tp - 1 of pq's
    # batch run into the next sample / the slack - all addressed, all finite here; K % 64 != 0 with k-contiguous A: gemm.hip
    L3 = dict(M=T, N=pd, K=Tp, a_sm=Tp, a_sk=1, b_sk=pd, b_sn=1, ldc=pd, nbatch=B, a_sb=T * Tp, b_sb=T * pd, c_sb=T * pd)

    def fill3(bufs):
        for r in range(B * T):
            bufs["A"][r * Tp + T:(r + 1) * Tp] = 0.0

    def indep3(bufs):
        dS = _t(_pad(bufs["A"], B * T * Tp).reshape(B, T, Tp))
        pq = np.stack([bufs["B"][b * T * pd:b * T * pd + Tp * pd].reshape(Tp, pd) for b in range(B)])
        return [_epi_from(L3, bufs, (dS @ _t(pq)).numpy())]
    _add("contrastive_dph_generic", L3, indep3, b_scale=0.125, fill=fill3, expect=(GENERIC, 1, 0), site="wav2vec2.py contrastive dph")


_contrastive()


# --- 8. fp32 parity attention (blocks.py _attn_fwd_parity / _attn_bwd_parity): six launches with nbatch2 = B on slices of one
# fused [B, T, 3D] tensor
def _parity_attention():
    B, H, hd, T = 2, 2, 32, 40
    D = H * hd
    D3, PP = 3 * D, H * T * T

    def heads(x, off):                                # [B, T, 3D] flat -> [B, H, T, hd] of the slice at column `off`
        return _t(_pad(x, B * T * D3).reshape(B, T, D3)[:, :, off:off + D].reshape(B, T, H, hd)).permute(0, 2, 1, 3)

    def probs(x):
        return _t(_pad(x, B * PP).reshape(B, H, T, T))

    def ctx(x):
        return _t(_pad(x, B * T * D).reshape(B, T, H, hd)).permute(0, 2, 1, 3)

    def add(name, L, f, expect=(F32, 1, WIDE)):
        def indep(bufs, L=L, f=f):
            pre = f(bufs).numpy()
            if L.get("scale_cols", 0) > 0:
                pre = pre * float(np.float32(L["scale"]))          # (scale_cols = N in all of these)
            return [(pre, None)]
        _add(name, L, indep, in_f32=True, out_bf16=False, expect=expect, site="blocks.py fp32 parity attention")

    two = dict(nbatch=H, nbatch2=B)
    add("parity_scores", dict(M=T, N=T, K=hd, a_sm=D3, a_sk=1, b_sk=1, b_sn=D3, ldc=T, a_sb=hd, b_sb=hd, c_sb=T * T, a_off=0,
                              b_off=D, scale_cols=T, scale=hd ** -0.5, a_sb2=T * D3, b_sb2=T * D3, c_sb2=PP, **two),
        lambda bufs: heads(bufs["A"], 0) @ heads(bufs["B"], D).transpose(-1, -2))
    add("parity_context", dict(M=T, N=hd, K=T, a_sm=T, a_sk=1, b_sk=D3, b_sn=1, ldc=D, a_sb=T * T, b_sb=hd, c_sb=hd, b_off=2 * D,
                               a_sb2=PP, b_sb2=T * D3, c_sb2=T * D, **two),
        lambda bufs: probs(bufs["A"]) @ heads(bufs["B"], 2 * D))
    add("parity_dprobs", dict(M=T, N=T, K=hd, a_sm=D, a_sk=1, b_sk=1, b_sn=D3, ldc=T, a_sb=hd, b_sb=hd, c_sb=T * T, b_off=2 * D,
                              a_sb2=T * D, b_sb2=T * D3, c_sb2=PP, **two),
        lambda bufs: ctx(bufs["A"]) @ heads(bufs["B"], 2 * D).transpose(-1, -2))
    add("parity_dv_kstrided", dict(M=T, N=hd, K=T, a_sm=1, a_sk=T, b_sk=D, b_sn=1, ldc=D3, a_sb=T * T, b_sb=hd, c_sb=hd,
                                   c_off=2 * D, a_sb2=PP, b_sb2=T * D, c_sb2=T * D3, **two),
        lambda bufs: probs(bufs["A"]).transpose(-1, -2) @ ctx(bufs["B"]))
    add("parity_dq", dict(M=T, N=hd, K=T, a_sm=T, a_sk=1, b_sk=D3, b_sn=1, ldc=D3, a_sb=T * T, b_sb=hd, c_sb=hd, b_off=D, c_off=0,
                          scale_cols=hd, scale=hd ** -0.5, a_sb2=PP, b_sb2=T * D3, c_sb2=T * D3, **two),
        lambda bufs: probs(bufs["A"]) @ heads(bufs["B"], D))
    add("parity_dk_kstrided", dict(M=T, N=hd, K=T, a_sm=1, a_sk=T, b_sk=D3, b_sn=1, ldc=D3, a_sb=T * T, b_sb=hd, c_sb=hd, b_off=0,
                                   c_off=D, scale_cols=hd, scale=hd ** -0.5, a_sb2=PP, b_sb2=T * D3, c_sb2=T * D3, **two),
        lambda bufs: probs(bufs["A"]).transpose(-1, -2) @ heads(bufs["B"], 0))


_parity_attention()


# --- 9. Log-mel DFT (frontend.py): fp32, overlapping rows of the waveform (a_sm = hop < K), one basis for the batch (b_sb = 0)
def _dft(name="logmel_dft", F_=45, expect=(F32, 1, WIDE), nb2=40, ldb=None):
    B, n_fft, hop = 2, 64, 16
    ldb = ldb or nb2
    Nw = (F_ - 1) * hop + n_fft + 8
    L = dict(M=F_, N=nb2, K=n_fft, a_sm=hop, a_sk=1, b_sk=ldb, b_sn=1, ldc=nb2, nbatch=B, a_sb=Nw, b_sb=0, c_sb=F_ * nb2)

    def indep(bufs):
        import torch
        w = _t(_pad(bufs["A"], B * Nw).reshape(B, Nw))
        frames = w.unfold(1, n_fft, hop)[:, :F_]                     # [B, F, n_fft]
        return [((frames @ _t(_pad(bufs["B"], n_fft * ldb).reshape(n_fft, ldb)[:, :nb2])).numpy(), None)]
    _add(name, L, indep, in_f32=True, out_bf16=False, b_scale=0.125, expect=expect, site="frontend.py DFT")


_dft()
# a clip of fewer than 32 frames: below the fp32 kernel's smallest problem, the generic kernel on fp32 operands
_dft("logmel_dft_few_frames", F_=20, expect=(GENERIC, 1, 0))
# an odd number of bins (n_fft / 2 + 1): spectrum rows that are no whole 16-byte chunks, the fp32 kernel's element epilogue
_dft("logmel_dft_odd_bins", nb2=41, ldb=44, expect=(F32, 1, 0))


# --- 10. LM head (whisper.py), at the smallest shapes that satisfy launch_fast's rules for it.  Millions of elements each:
# they exist for one path of the library's own rules and stay out of the forced children.
def _lm_head_dgrad(name, K, expect):
    """dX[R, d] = dlogits x W^T over the padded vocabulary, fp32 out: slab splits on the eight-phase kernel's 192-row tiles -
    8 K ranges over XCD groups at K = 16384, 16 / 32 ranges dealt two / four per XCD at K = 32768 / 65536."""
    M, N, ldw = 520, 256, K
    L = dict(M=M, N=N, K=K, a_sm=K, a_sk=1, b_sk=1, b_sn=ldw, ldc=N, splitk=0)

    def indep(bufs):
        A = _t(_pad(bufs["A"], M * K).reshape(M, K))
        W = _t(_pad(bufs["B"], N * ldw).reshape(N, ldw))
        return [((A @ W.t()).numpy()[None], None)]
    # (non-negative operands: with signed ones the worst-case accumulation bound of K = 16384, ~1e-3 * sum |a||b|, is ~10 % of
    # a typical |result| and hides a missing K-tile; without cancellation sum |a||b| IS the result)
    _add(name, L, indep, out_bf16=False, b_scale=1.0 / 128, repeat_equal=True, gen="abs", expect=expect,
         site="whisper.py LM head dgrad", children="all" if K == 16384 else "none",
         # (16 / 32 ranges, only ever run under the rules: each range sums K / ranges products in a chain, the reduce pass adds the
         # ranges in order - the depth of that tree bounds the error, see _gemm_ref)
         acc_chain=None if K == 16384 else K // expect[1] + expect[1])


_lm_head_dgrad("lm_head_dgrad_deep_k", 16384, (14, 8, SLABS | XCD_GROUPS | WIDE))
_lm_head_dgrad("lm_head_dgrad_16_splits", 32768, (14, 16, SLABS | XCD_DEAL | WIDE))
_lm_head_dgrad("lm_head_dgrad_32_splits", 65536, (14, 32, SLABS | XCD_DEAL | WIDE))


def _lm_head_fwd():
    """logits[R, Vp] = x W over a padded vocabulary (ldw = ldc = Vp > V): 3 x 171 = 513 tiles of 256 x 256 from R = 520 rows,
    the fewest that send so short an M to the eight-phase kernel - its persistent form on 256-row tiles."""
    M, V, Vp, K = 520, 43700, 43776, 128
    L = dict(M=M, N=V, K=K, a_sm=K, a_sk=1, b_sk=Vp, b_sn=1, ldc=Vp)

    def indep(bufs):
        A = _t(_pad(bufs["A"], M * K).reshape(M, K))
        W = _t(_pad(bufs["B"], K * Vp).reshape(K, Vp)[:, :V])
        return [((A @ W).numpy()[None], None)]
    _add("lm_head_forward_padded_vocab", L, indep, b_scale=1.0 / math.sqrt(K), expect=(10, 1, PERSISTENT | WIDE),
         site="whisper.py LM head forward", children="none")


_lm_head_fwd()
# dW[d, Vp] = x^T dlogits from K = R rows: 2 x 256 = 512 tiles, the wide-output rule - eight-phase kernel, no split
_wgrad("lm_head_weight_gradient", K_in=264, N=65300, T=520, ld_dy=65304, ldc=65304, expect=(10, 1, WIDE), children="none",
       site="whisper.py LM head weight gradient")


# --- 10b. The eight-phase kernel's PERSISTENT form (more than 256 tile slots: the LM head's forward, the d_model-wide
# projections of a 12000-token batch) at its smallest: 17 x 16 tiles of 256 x 256 / 22 x 16 of 192 x 256 with a ragged last
# row tile (4104 = 16 * 256 + 8 = 21 * 192 + 72) and a ragged last column tile (4032 = 15 * 256 + 192), K = 128 (two K-tiles,
# its minimum) and K = 192 (the first count at which the ring carries over between tiles), each for every lean epilogue class
# and for one combination outside them.  The rules give these the 192-row tiles
# (fewer CU-rounds); TMI_GEMM_CFG=10 runs the same cases on 256-row tiles (tests/test_gemm_forced_gpu.py).
def _persistent(name, epi, K, b_kn):
    M, N, ldc = 4104, 4032, 4040
    ld_a = K + 8
    if b_kn:
        ldb, b_sk, b_sn = N + 8, N + 8, 1
    else:
        ldb, b_sk, b_sn = K + 8, 1, K + 8
    L = dict(M=M, N=N, K=K, a_sm=ld_a, a_sk=1, b_sk=b_sk, b_sn=b_sn, ldc=ldc, **epi)

    def indep(bufs, L=L):
        A = _t(_pad(bufs["A"], M * ld_a).reshape(M, ld_a)[:, :K])
        if b_kn:
            W = _t(_pad(bufs["B"], K * ldb).reshape(K, ldb)[:, :N])
        else:
            W = _t(_pad(bufs["B"], N * ldb).reshape(N, ldb)[:, :K]).t()
        return [_epi_from(L, bufs, (A @ W).numpy()[None])]
    _add(name, L, indep, b_scale=1.0 / math.sqrt(K), expect=(14, 1, PERSISTENT | WIDE), site="eight-phase kernel, persistent form",
         children="p8")


for _K in (128, 192):
    _persistent(f"persistent_simple_k{_K}", dict(bias=True, scale_cols=1000, scale=0.125), _K, True)
    _persistent(f"persistent_auxin_k{_K}", dict(aux_in=True), _K, False)
    _persistent(f"persistent_resid_drop_k{_K}", dict(bias=True, dropout_p=0.1, dropout_seed=77, resid=True, r_ld=4048), _K, _K == 192)
    _persistent(f"persistent_acc_k{_K}", dict(accumulate=True), _K, _K == 192)
    _persistent(f"persistent_generic_k{_K}", dict(bias=True, scale_cols=72, scale=0.125, resid=True, r_ld=4048), _K, _K == 128)


# --- 11. Exact cases: no tolerance
def _exact_identity(name, a_t, b_t):
    """A = a row-permuted identity (M = K): C must be the permuted rows of B bit for bit (one non-zero product per sum)."""
    M = K = 128
    N, ldb, ldc = 104, 112, 112
    a_sm, a_sk = (1, M) if a_t else (K, 1)
    b_sk, b_sn = (1, K) if b_t else (ldb, 1)
    L = dict(M=M, N=N, K=K, a_sm=a_sm, a_sk=a_sk, b_sk=b_sk, b_sn=b_sn, ldc=ldc)
    perm = np.random.default_rng(7).permutation(M)

    def fill(bufs):
        P = np.zeros((M, K))
        P[np.arange(M), perm] = 1.0
        bufs["A"][:M * K] = (P.T if a_t else P).reshape(-1)

    def indep(bufs):
        Bm = _pad(bufs["B"], N * K).reshape(N, K).T if b_t else _pad(bufs["B"], K * ldb).reshape(K, ldb)[:, :N]
        return [(Bm[perm][None].copy(), None)]
    _add(name, L, indep, fill=fill, exact=True, expect=(12, 1, WIDE), site="exact: permuted identity")   # (tt too: the bf16
    # tiles are instantiated for a k-strided A with a k-contiguous B; only the eight-phase and fp32 kernels are not)


_exact_identity("exact_identity_nn", False, False)
_exact_identity("exact_identity_nt", False, True)
_exact_identity("exact_identity_tn", True, False)
_exact_identity("exact_identity_tt", True, True)

# bf16 integers in [-2, 2], fp32 out: sums of at most 4 * K_total < 2^24 are exact in any order, so every split form must
# give the int64 product exactly.  (No rule sends a bf16 reduction of <= 1024 through slabs - they start at 64 K-tiles -
# so the slab form runs K = 4104: 4 * 4104 is still far below 2^24.)
_wgrad("exact_int_nosplit", T=200, gen="int", exact=True, expect=(4, 1, WIDE))
_wgrad("exact_int_atomic", T=1032, ws=False, zero_c=True, gen="int", exact=True, expect=(4, 4, ATOMIC | XCD_GROUPS | WIDE))
# (a caller-chosen split is no "weight-gradient-like" launch for launch_fast: the small-problem rule, Tile64Waves2)
_wgrad("exact_int_caller_splitk3", T=1032, zero_c=True, gen="int", exact=True, splitk=3, expect=(6, 3, ATOMIC | WIDE))
_wgrad("exact_int_slabs", T=4104, gen="int", exact=True, expect=(4, 8, SLABS | XCD_GROUPS | WIDE))

BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# ---------------------------------------------------------------------------------------------- which kernel can run a case
def fast_class(L, in_f32):
    """(eligible for gemm_fast.hip's bf16 kernels, A k-strided, B k-strided): the conditions of tmi_gemm_fast_try, pointer
    alignment taken from the element offsets (the buffers themselves are 16-byte aligned)."""
    if in_f32 or L.get("nbatch2", 1) > 1:
        return False, False, False
    g = L.get
    if g("a_off", 0) % 8 or g("b_off", 0) % 8 or g("a_sb", 0) % 8 or g("b_sb", 0) % 8 or g("a_skb", 0) % 8 or g("b_skb", 0) % 8:
        return False, False, False
    M, N, K = L["M"], L["N"], L["K"]
    a_kc = L["a_sk"] == 1 and L["a_sm"] % 8 == 0
    b_kc = L["b_sk"] == 1 and L["b_sn"] % 8 == 0
    a_ks = L["a_sm"] == 1 and L["a_sk"] % 8 == 0 and (M % 8 == 0 or L["a_sk"] >= rup(M, 8)) and M >= 8
    b_ks = L["b_sn"] == 1 and L["b_sk"] % 8 == 0 and (N % 8 == 0 or L["b_sk"] >= rup(N, 8)) and N >= 8
    if not (a_kc or a_ks) or not (b_kc or b_ks):
        return False, False, False
    A_KS, B_KS = not a_kc, not b_kc
    if K % 64 != 0 and not (A_KS and B_KS):
        return False, False, False
    return True, A_KS, B_KS


def can_run(L, in_f32, cfg):
    """Whether TMI_GEMM_CFG=cfg runs launch L on that kernel (the conditions at the top of launch_fast)."""
    ok, A_KS, B_KS = fast_class(L, in_f32)
    if not ok:
        return False
    splitk = L.get("splitk", 1)
    if cfg in (4, 5, 6):
        return True
    if cfg in (12, 13):
        return splitk <= 1
    if cfg in (15, 16):
        return splitk <= 1 and L["K"] % 64 == 0
    K = L["K"]
    k_ok = K % 64 == 0 or (A_KS and B_KS and K % 8 == 0)
    p8 = (L.get("kbatch", 1) <= 1 and k_ok and K >= 128 and L["a_sm"] >= 0 and L["b_sn"] >= 0 and L["a_sk"] >= 0 and
          L["b_sk"] >= 0)
    if cfg == 10:
        return p8 and splitk <= 1 and (not A_KS or B_KS)
    if cfg == 14:
        return p8 and splitk <= 1 and not A_KS
    return False


# ---------------------------------------------------------------------------------------------- buffers and references
def _extent(idx):
    assert idx.min() >= 0, int(idx.min())
    return int(idx.max()) + 1


def _ref_kwargs(L):
    kw = {k: v for k, v in L.items() if k not in ("M", "N", "K", "a_sm", "a_sk", "b_sk", "b_sn", "ldc", "bias", "aux_in",
                                                  "resid", "aux_out", "bias_off")}
    return kw


def _noise(rng, n, row, scale):
    rows = (n + row - 1) // row
    s = np.exp2(rng.uniform(-3.0, 3.0, size=rows))
    return (rng.standard_normal(n) * np.repeat(s, row)[:n]) * scale


def prepare(case):
    """-> (bufs, refs): float64 images of every buffer (poison = NaN) and gemm_ref's result per launch."""
    import zlib
    rng = np.random.default_rng(zlib.crc32(case["name"].encode()))
    in_bf16, out_bf16 = not case["in_f32"], case["out_bf16"]
    Ls = case["launches"]
    idx = []
    for L in Ls:
        nb2, nb, kb = max(1, L.get("nbatch2", 1)), max(1, L.get("nbatch", 1)), max(1, L.get("kbatch", 1))
        g = L.get
        a = R.operand_indices(g("a_off", 0), g("a_sb2", 0), g("a_sb", 0), g("a_skb", 0), L["a_sm"], L["a_sk"], nb2, nb, kb, L["M"], L["K"])
        b = R.operand_indices(g("b_off", 0), g("b_sb2", 0), g("b_sb", 0), g("b_skb", 0), L["b_sn"], L["b_sk"], nb2, nb, kb, L["N"], L["K"])
        c = R.window_indices(g("c_off", 0), g("c_sb2", 0), g("c_sb", 0), L["ldc"], nb2, nb, L["M"], L["N"])
        bi = g("bias_off", 0) + np.arange(nb)[:, None] * g("bias_sb", 0) + np.arange(L["N"])[None, :] if g("bias") else None
        ri = R.window_indices(0, 0, g("r_sb", 0), L["r_ld"], 1, nb, L["M"], L["N"]) if g("resid") else None
        idx.append(dict(A=a, B=b, C=c, bias=bi, resid=ri))

    def size(key):
        ext = max([_extent(i[key]) for i in idx if i[key] is not None], default=0)
        return rup(ext, 8) + 64 if ext else 0

    L0 = Ls[0]
    lead = lambda s0, s1: max(8, abs(s0) if abs(s0) > 1 else abs(s1))
    bufs = {}
    if case["gen"] == "int":
        bufs["A"] = rng.integers(-2, 3, size=size("A")).astype(np.float64)
        bufs["B"] = rng.integers(-2, 3, size=size("B")).astype(np.float64)
    else:
        b_scale = case["b_scale"] if case["b_scale"] is not None else 1.0
        sgn = np.abs if case["gen"] == "abs" else (lambda x: x)
        bufs["A"] = round_to(sgn(_noise(rng, size("A"), lead(L0["a_sm"], L0["a_sk"]), case["a_scale"])), in_bf16)
        bufs["B"] = round_to(sgn(_noise(rng, size("B"), lead(L0["b_sn"], L0["b_sk"]), b_scale)), in_bf16)
    nC = size("C")
    bufs["C"] = round_to(_noise(rng, nC, max(8, L0["ldc"]), 1.0), out_bf16)
    if any(L.get("aux_in") for L in Ls):
        bufs["aux_in"] = round_to(_noise(rng, nC, max(8, L0["ldc"]), 0.5), out_bf16)
    if size("bias"):
        bufs["bias"] = _f32(rng.standard_normal(size("bias")))
    if size("resid"):
        bufs["resid"] = round_to(_noise(rng, size("resid"), max(8, L0["r_ld"]), 1.0), out_bf16)
    if case["fill"] is not None:
        case["fill"](bufs)
        bufs["A"], bufs["B"] = round_to(bufs["A"], in_bf16), round_to(bufs["B"], in_bf16)
    # poison: whatever no launch addresses
    for key, names in (("A", ("A",)), ("B", ("B",)), ("bias", ("bias",)), ("resid", ("resid",)), ("C", ("C", "aux_in"))):
        used = np.zeros(len(bufs[names[0]]) if names[0] in bufs else 0, dtype=bool)
        for n, (i, L) in enumerate(zip(idx, Ls)):
            if i[key] is not None:
                used[i[key].reshape(-1)] = True
        for nm in names:
            if nm not in bufs:
                continue
            if nm == "C":
                keep = np.zeros_like(used)
                for i, L in zip(idx, Ls):
                    if L.get("accumulate") or case["zero_c"]:
                        keep[i["C"].reshape(-1)] = True
                if case["zero_c"]:
                    bufs["C"][keep] = 0.0
                bufs["C"][~keep] = np.nan
            elif nm == "aux_in":
                keep = np.zeros_like(used)
                for i, L in zip(idx, Ls):
                    if L.get("aux_in"):
                        keep[i["C"].reshape(-1)] = True
                bufs["aux_in"][~keep] = np.nan
            else:
                bufs[nm][~used] = np.nan
    return bufs, [ref_launch(case, L, bufs) for L in Ls]


def ref_launch(case, L, bufs, **override):
    """gemm_ref of one launch of the case on the prepared buffers (``override``: changed arguments, for wrong results)."""
    override = dict(override)
    bo = L.get("bias_off", 0)
    kw = dict(bias=bufs["bias"][bo:] if L.get("bias") else None, aux_out=bool(L.get("aux_out")),
              aux_in=bufs["aux_in"] if L.get("aux_in") else None, resid=bufs["resid"] if L.get("resid") else None,
              out_bf16=case["out_bf16"], in_f32=case["in_f32"], acc_chain=case["acc_chain"], **_ref_kwargs(L))
    M = override.pop("M", L["M"])     # (a row prefix of the launch: every address and the dropout mask stay what they are)
    kw.update(override)
    return R.gemm_ref(bufs["A"], bufs["B"], bufs["C"], M, L["N"], L["K"], L["a_sm"], L["a_sk"], L["b_sk"], L["b_sn"],
                      L["ldc"], **kw)


# ---------------------------------------------------------------------------------------------- running a case on the GPU
def run_case(case, dev, prepared=None, rules=True):
    """Runs every launch of the case through the C entry point (its own descriptors: the workspace is the case's choice)
    and checks it.  -> dict(paths, ratio, redzone, exact, repeat).
    ``rules``: the library's own dispatch rules are in force, so the table knows which library-chosen splits go through
    workspace slabs and leaves NaN in their C.  Under a forced kernel (rules=False) the same launch may be summed with
    atomics, so C is zeroed for every splitk == 0 launch without ``accumulate``, as tethys_mi.h asks of the caller."""
    import ctypes as C
    import torch
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import ops, _lib
    lib = _lib.lib()
    bufs, refs = prepared if prepared is not None else prepare(case)
    in_dt = torch.float32 if case["in_f32"] else torch.bfloat16
    out_dt = torch.bfloat16 if case["out_bf16"] else torch.float32
    ivw = torch.int16 if case["out_bf16"] else torch.int32
    dts = dict(A=in_dt, B=in_dt, C=out_dt, aux_in=out_dt, resid=out_dt, bias=torch.float32)
    g = {k: torch.from_numpy(v).to(dts[k]).to(dev) for k, v in bufs.items()}
    has_aux = any(L.get("aux_out") for L in case["launches"])
    if not rules:
        for L, r in zip(case["launches"], refs):
            if L.get("splitk", 1) == 0 and not L.get("accumulate"):
                g["C"][torch.from_numpy(r["written"]).to(dev)] = 0.0
    ws = ops.gemm_workspace(dev) if case["ws"] else None
    prev = lib.tmi_set_deterministic(1) if case["deterministic"] else None
    try:
        def launch_all():
            Cm = g["C"].clone()
            aux = torch.full_like(Cm, float("nan")) if has_aux else None
            paths = []
            for L in case["launches"]:
                d = _lib.GemmDesc()
                esA, esC = g["A"].element_size(), Cm.element_size()
                q = L.get
                d.A = g["A"].data_ptr() + q("a_off", 0) * esA
                d.B = g["B"].data_ptr() + q("b_off", 0) * esA
                d.C = Cm.data_ptr() + q("c_off", 0) * esC
                d.M, d.N, d.K = L["M"], L["N"], L["K"]
                d.a_sm, d.a_sk, d.b_sk, d.b_sn, d.ldc = L["a_sm"], L["a_sk"], L["b_sk"], L["b_sn"], L["ldc"]
                d.nbatch, d.a_sb, d.b_sb, d.c_sb = q("nbatch", 1), q("a_sb", 0), q("b_sb", 0), q("c_sb", 0)
                d.kbatch, d.a_skb, d.b_skb = q("kbatch", 1), q("a_skb", 0), q("b_skb", 0)
                d.bias = g["bias"].data_ptr() + 4 * q("bias_off", 0) if q("bias") else None
                d.bias_sb = q("bias_sb", 0)
                d.scale_cols, d.scale = q("scale_cols", 0), q("scale", 1.0)
                d.accumulate, d.act = int(bool(q("accumulate"))), q("act", 0)
                d.aux_out = aux.data_ptr() + q("c_off", 0) * esC if q("aux_out") else None
                d.aux_in = g["aux_in"].data_ptr() + q("c_off", 0) * esC if q("aux_in") else None
                d.resid = g["resid"].data_ptr() if q("resid") else None
                d.r_ld, d.r_sb = q("r_ld", 0), q("r_sb", 0)
                d.splitk = q("splitk", 1)
                d.dropout_p, d.dropout_seed = q("dropout_p", 0.0), q("dropout_seed", 0)
                d.nbatch2, d.a_sb2, d.b_sb2, d.c_sb2 = q("nbatch2", 1), q("a_sb2", 0), q("b_sb2", 0), q("c_sb2", 0)
                if ws is not None and d.splitk == 0:
                    d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
                d.in_dtype = _lib.TMI_F32 if case["in_f32"] else _lib.TMI_BF16
                d.out_dtype = _lib.TMI_BF16 if case["out_bf16"] else _lib.TMI_F32
                _lib.check(lib.tmi_gemm(C.byref(d), ops.stream()), "tmi_gemm")
                ns, fl = C.c_int32(0), C.c_int32(0)
                kern = lib.tmi_gemm_last_path(C.byref(ns), C.byref(fl))
                paths.append((int(kern), int(ns.value), int(fl.value)))
            torch.cuda.synchronize()
            return Cm, aux, paths

        Cm, aux, paths = launch_all()
        repeat = None
        if case["repeat_equal"]:
            Cm2, _, _ = launch_all()
            repeat = bool(torch.equal(Cm.view(ivw), Cm2.view(ivw)))
    finally:
        if prev is not None:
            lib.tmi_set_deterministic(prev)
    got = Cm.double().cpu().numpy()
    got_aux = aux.double().cpu().numpy() if aux is not None else None
    ratio, exact = 0.0, True
    written = np.zeros(got.size, dtype=bool)
    aux_written = np.zeros(got.size, dtype=bool)
    for L, r in zip(case["launches"], refs):
        ratio = max(ratio, R.worst_ratio(got[r["c_idx"]], r["ref"], r["bound"]))
        exact = exact and bool(np.array_equal(got[r["c_idx"]], round_to(r["ref"], case["out_bf16"])))
        written[r["written"]] = True
        if L.get("aux_out"):
            ratio = max(ratio, R.worst_ratio(got_aux[r["c_idx"]], r["aux_ref"], r["aux_bound"]))
            aux_written[r["written"]] = True
    # redzone: everything outside `written` bit-identical to what was there (integer view: NaN payloads included)
    before = g["C"].view(ivw).cpu().numpy()
    redzone = bool(np.array_equal(Cm.view(ivw).cpu().numpy()[~written], before[~written]))
    if aux is not None:
        nanbits = torch.full_like(g["C"], float("nan")).view(ivw).cpu().numpy()
        redzone = redzone and bool(np.array_equal(aux.view(ivw).cpu().numpy()[~aux_written], nanbits[~aux_written]))
    return dict(paths=paths, ratio=ratio, redzone=redzone, exact=exact, repeat=repeat)
