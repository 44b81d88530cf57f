"""Descriptor-level float64 reference of tmi_gemm (CPU only, numpy).

``gemm_ref`` takes flat 1-D buffers and exactly the arguments of ``ops.gemm`` and evaluates the contract of
include/tethys_mi.h literally, by index arithmetic (no as_strided: strides may be negative, rows may overlap).  It returns
the reference over the addressed ``[nbatch2, nbatch, M, N]`` window, the set of flat indices of C the call may write, the
operand elements the formula addresses (everything else may hold poison) and a PER-ELEMENT error bound derived from the
arithmetic of the kernels - not measured; the constants below were fixed before the first GPU run.

Bound, per element (u = 2^-24, the unit round-off of the fp32 accumulators and of every fp32 epilogue operation):
  accumulation   (K_total + 4) * u * S,  S = |scale| * (sum |a||b| + |bias|) + |C_old|: the forward error of ANY summation
                 order of K_total exact products (Higham, Accuracy and Stability, (3.4): (n - 1) u sum |terms|; bf16 products
                 are exact in fp32, an fp32 product adds one rounding; K-groups, split-K slabs and atomics are other
                 orders of the same sum) plus the bias add, the column scale, the C_old add and one spare; ``scale``
                 multiplies what was summed before it, C_old joins after it (the epilogue order of the header).
                 Where the table fixes the split (the LM head's 16 / 32 K ranges, asserted through tmi_gemm_last_path) the
                 factor is the DEPTH of that summation tree, K_total / ranges + ranges (Higham (4.4): depth * u * sum |terms|
                 for any tree) - tighter, and needed: (65536 + 4) u is four times the weight of one of 1024 K-tiles.
  Lipschitz      that error passes through the rest of the epilogue: x max|gelu'| (act == 1), x |gelu'(aux_in)|,
                 x keep_scale (dropout); each of those fp32 operations adds u * |its result|.
  erf            gelu(x) = x c(x), gelu'(x) = c(x) + x p(x).  bf16 outputs use the Abramowitz-Stegun 7.1.26 erf documented in
                 csrc/tmi_common.h (absolute error 1.5e-7) evaluated in fp32 (1 rcp, 1 exp, 6 fma on values <= 1: 8 u);
                 fp32 outputs use erff (<= 8 u absolute, it is a few ulp of a value <= 1).  c = (1 + erf) / 2 halves it; the
                 same absolute error is charged to p (exp of a non-positive argument, <= 0.4).
  residual       the fp32 add rounds once more: u * (|v| + |resid|) (written with the two magnitudes, so that it holds
                 under cancellation).
  output         round-to-nearest into the output type (from_f32<bf16_t>: 8 significant bits; fp32: 24): half an ulp of the
                 binade of the COMPUTED value, 2^(floor(log2(|ref| + err)) - p).  That is between 2^-(p+1) |x| (top of a
                 binade) and 2^-p |x| (bottom): a flat 2^-9 |ref| for bf16 is NOT a bound of a correctly rounded result
                 (tests/test_gemm_ref_cpu.py: the exactly rounded reference itself reaches 1.8 times it), the flat 2^-8 |ref|
                 is up to twice too wide, so the term is written per binade.  aux_out likewise.
"""
import math

import numpy as np

U32 = 2.0 ** -24
P_BF16, P_F32 = 8, 24    # significant bits of the output types
GELU_GRAD_MAX = 1.1290   # max |gelu_erf'(x)| (at x = sqrt(2)): 1.12893
ERF_FAST = 1.5e-7 + 8 * U32
ERF_F32 = 8 * U32



def _erf(x):
    import torch
    return torch.erf(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))).numpy()


def gelu(x):
    return 0.5 * x * (1.0 + _erf(x / math.sqrt(2.0)))


def gelu_grad(x):
    return 0.5 * (1.0 + _erf(x / math.sqrt(2.0))) + x * np.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def half_ulp(x, p):
    """Half an ulp of a p-bit binary format in the binade of |x| (the largest round-to-nearest error there)."""
    _, e = np.frexp(np.maximum(np.abs(x), np.finfo(np.float64).tiny))     # |x| = m 2^e, 0.5 <= m < 1
    return np.ldexp(1.0, e - 1 - p)


def _ar(n):
    return np.arange(n, dtype=np.int64)


def operand_indices(off, sb2, sb, skb, s_row, s_k, nb2, nb, kb, rows, K):
    """[nb2, nb, kb, rows, K] flat indices of one operand."""
    return (off + _ar(nb2)[:, None, None, None, None] * sb2 + _ar(nb)[None, :, None, None, None] * sb +
            _ar(kb)[None, None, :, None, None] * skb + _ar(rows)[None, None, None, :, None] * s_row +
            _ar(K)[None, None, None, None, :] * s_k)


def window_indices(off, sb2, sb, ld, nb2, nb, M, N):
    """[nb2, nb, M, N] flat indices of C (aux_*, resid)."""
    return (off + _ar(nb2)[:, None, None, None] * sb2 + _ar(nb)[None, :, None, None] * sb +
            _ar(M)[None, None, :, None] * ld + _ar(N)[None, None, None, :])


def gemm_ref(A, B, C_old, M, N, K, a_sm, a_sk, b_sk, b_sn, ldc, *, nbatch=1, a_sb=0, b_sb=0, c_sb=0, kbatch=1, a_skb=0,
             b_skb=0, bias=None, bias_sb=0, scale_cols=0, scale=1.0, accumulate=False, act=0, aux_out=False, aux_in=None,
             resid=None, r_ld=0, r_sb=0, splitk=1, a_off=0, b_off=0, c_off=0, dropout_p=0.0, dropout_seed=0, nbatch2=1,
             a_sb2=0, b_sb2=0, c_sb2=0, out_bf16=True, in_f32=False, acc_delta=None, acc_chain=None):
    """A, B, C_old, bias, aux_in, resid: flat float64 numpy arrays holding the (already rounded) buffer contents; ``aux_out``
    is a flag.  Returns a dict: ref, aux_ref, bound, aux_bound ([nbatch2, nbatch, M, N]), c_idx (the same shape: flat
    indices of C / aux_out / aux_in), written (sorted unique c_idx), a_idx / b_idx / bias_idx / resid_idx (what the
    formula reads), a_g / b_g (the gathered operands, [nbatch2, nbatch, M or N, K_total]) and pre (the value before the
    activation).  ``acc_delta`` is added to the accumulated sums before the epilogue (tests/test_gemm_ref_cpu.py builds
    wrong results with it)."""
    nb2, nb, kb = max(1, nbatch2), max(1, nbatch), max(1, kbatch)
    a_idx = operand_indices(a_off, a_sb2, a_sb, a_skb, a_sm, a_sk, nb2, nb, kb, M, K)
    b_idx = operand_indices(b_off, b_sb2, b_sb, b_skb, b_sn, b_sk, nb2, nb, kb, N, K)
    for name, idx, buf in (("A", a_idx, A), ("B", b_idx, B)):
        assert idx.min() >= 0 and idx.max() < buf.size, (name, int(idx.min()), int(idx.max()), buf.size)
    a = A[a_idx]                                     # [nb2, nb, kb, M, K]
    b = B[b_idx]                                     # [nb2, nb, kb, N, K]
    a = a.transpose(0, 1, 3, 2, 4).reshape(nb2, nb, M, kb * K)
    b = b.transpose(0, 1, 3, 2, 4).reshape(nb2, nb, N, kb * K)
    v = a @ b.transpose(0, 1, 3, 2)
    S = np.abs(a) @ np.abs(b).transpose(0, 1, 3, 2)
    if acc_delta is not None:
        v = v + acc_delta
    c_idx = window_indices(c_off, c_sb2, c_sb, ldc, nb2, nb, M, N)
    assert c_idx.min() >= 0 and c_idx.max() < C_old.size, ("C", int(c_idx.min()), int(c_idx.max()), C_old.size)
    mask = np.zeros(C_old.size, dtype=bool)
    mask[c_idx.reshape(-1)] = True
    written = np.flatnonzero(mask)
    assert written.size == c_idx.size, "C windows overlap"
    out = dict(c_idx=c_idx, written=written, a_idx=a_idx, b_idx=b_idx, bias_idx=None, resid_idx=None, a_g=a, b_g=b)
    p_out = P_BF16 if out_bf16 else P_F32
    erf_abs = ERF_FAST if out_bf16 else ERF_F32
    k_total = K * kb + (1 if in_f32 else 0)          # (an fp32 product rounds once; a bf16 product is exact)
    if acc_chain is not None:                        # (a known summation tree: its depth instead of its leaf count)
        assert acc_chain <= k_total
        k_total = acc_chain
    if bias is not None:
        bias_idx = _ar(nb)[:, None] * bias_sb + _ar(N)[None, :]
        out["bias_idx"] = bias_idx
        bv = bias[bias_idx][None, :, None, :]
        v = v + bv
        S = S + np.abs(bv)
    if scale_cols > 0:
        sc = np.where(_ar(N) < scale_cols, float(np.float32(scale)), 1.0)[None, None, None, :]
        v = v * sc
        S = S * np.abs(sc)
    if accumulate:
        old = C_old[c_idx]
        v = v + old
        S = S + np.abs(old)
    err = (k_total + 4) * U32 * S
    out["pre"] = v
    if aux_out:
        out["aux_ref"] = v
        out["aux_bound"] = err + half_ulp(np.abs(v) + err, p_out)
    if act == 1:
        # |x| * (erf error / 2) for c, the Lipschitz factor for the incoming error, one rounding of the product
        err = GELU_GRAD_MAX * err + np.abs(v) * 0.5 * erf_abs
        v = gelu(v)
        err = err + 2 * U32 * np.abs(v)
    if aux_in is not None:
        x = aux_in[c_idx]
        g = gelu_grad(x)
        g_err = 0.5 * erf_abs + np.abs(x) * erf_abs + 3 * U32 * (np.abs(g) + np.abs(x) * 0.4)
        err = np.abs(g) * err + np.abs(v) * g_err
        v = v * g
        err = err + U32 * np.abs(v)
    if dropout_p > 0.0:
        from oracle import dropout as DO
        assert nb2 == 1 and nb == 1
        keep = DO.keep_flat(dropout_seed, M, N, dropout_p).astype(np.float64)[None, None]
        ks = float(DO.keep_scale(dropout_p))
        v = v * keep * ks
        err = (err * ks + 2 * U32 * np.abs(v)) * keep
    if resid is not None:
        assert nb2 == 1
        r_idx = window_indices(0, 0, r_sb, r_ld, 1, nb, M, N)
        assert r_idx.min() >= 0 and r_idx.max() < resid.size, ("resid", int(r_idx.max()), resid.size)
        out["resid_idx"] = r_idx
        r = resid[r_idx]
        err = err + U32 * (np.abs(v) + np.abs(r))
        v = v + r
    out["ref"] = v
    out["bound"] = err + half_ulp(np.abs(v) + err, p_out)
    return out


def worst_ratio(got, ref, bound):
    """max err / bound over every element; a NaN (or inf) anywhere in ``got`` gives inf."""
    got = np.asarray(got, dtype=np.float64)
    if not np.isfinite(got).all():
        return float("inf")
    tiny = np.finfo(np.float64).tiny
    return float((np.abs(got - ref) / np.maximum(bound, tiny)).max())
