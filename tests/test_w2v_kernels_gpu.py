"""The Wav2Vec2 pre-training kernels (csrc/wav2vec2.hip) - GroupNorm+GELU, the fused FIR stem, the positional-conv packs, the
vector quantiser, the contrastive loss, segment sums and clip - each against a float64 reference (tests/_w2v_kernel_ref.py,
itself checked by tests/test_w2v_kernel_ref_cpu.py) at the shapes where their loops and launch rules change path.  Which
path a shape reaches, with its arithmetic, stands next to the shape in _w2v_kernel_ref.py; the CPU test asserts it.

Inputs and outputs are slices of larger buffers full of 7.0 / NaN guards, compared bit for bit after the call; work buffers
are sized by the library's own sizing calls with a guard tail behind them.  No bound comes from the kernels' measured
error: plain inputs use the project's tolerances against max|ref| (fp32 2e-5 forward, 1e-4 gradients; bf16 1.5e-2 / 3e-2
on inputs rounded to bf16 first), sums use a count of fp32 roundings times 2^-24 times the reference's sum of |terms|,
pure data movement is bit equality.  Measured / bound goes through _margins.within under the names "w2vk ...".
"""
import math

import numpy as np
import pytest
import torch

import _w2v_kernel_ref as R
from _margins import within

pytestmark = pytest.mark.gpu

U = R.U
TMI_ERR_INVALID = -1  # include/tethys_mi.h
F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
DTYPES = [F32, BF16]


def _ops():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import ops
    return ops


def dname(dtype):
    return "bf16" if dtype == BF16 else "fp32"


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def guard_pattern(n, dtype):
    """7.0 / NaN alternating (integers: 7 / a large negative): a stray store of any finite value, or of NaN, shows."""
    t = torch.full((n,), 7, dtype=dtype)
    t[1::2] = R.NAN if dtype.is_floating_point else -(2 ** 30)
    return t


class Buf:
    """B rows of n elements at element offset ``off`` with batch stride ``sb`` inside a buffer full of guard values."""

    def __init__(self, dev, n, dtype, data=None, B=1, sb=None, off=8, trail=64):
        sb = n if sb is None else sb
        assert sb >= n and off % 8 == 0 and sb % 8 == 0 or B == 1
        host = guard_pattern(off + (B - 1) * sb + n + trail, dtype)
        self.mask = torch.zeros(host.shape, dtype=torch.bool)
        for b in range(B):
            self.mask[off + b * sb:off + b * sb + n] = True
        if data is not None:
            host[self.mask] = data.to(dtype).reshape(-1)
        self.host0, self.t, self.B, self.n, self.sb, self.off = host.clone(), host.to(dev), B, n, sb, off

    @property
    def v(self):   # the first (for B = 1: the only) row as a view: its data_ptr() is what the entry point gets
        return self.t[self.off:self.off + self.n]

    def rows(self):
        return self.t.cpu()[self.mask].reshape(self.B, self.n)

    def guards_ok(self):
        return same(self.t.cpu()[~self.mask], self.host0[~self.mask])


def all_guards(*bufs):
    return all(b.guards_ok() for b in bufs)


def check(name, got, ref, bound_rel, detail=None):
    """max|got - ref| / max|ref| against ``bound_rel``; a NaN anywhere fails."""
    got, ref = got.detach().to(F64).cpu(), ref.detach().to(F64).cpu()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert not bool(torch.isnan(got).any()), (name, "NaN in the output", detail)
    m = float(ref.abs().max())
    err = float((got - ref).abs().max())
    frac = err / m if m > 0 else (0.0 if err == 0.0 else math.inf)
    print(f"{name}: {frac:.3e} (bound {bound_rel:.3e}) {detail or ''}")
    within(name, frac, bound_rel, detail)


def check_abs(name, got, ref, bound, detail=None):
    """|got - ref| <= bound element by element (bound a tensor or a number); reported as the largest err / bound."""
    got, ref = got.detach().to(F64).cpu(), ref.detach().to(F64).cpu()
    assert not bool(torch.isnan(got).any()), (name, "NaN in the output", detail)
    bound = torch.as_tensor(bound, dtype=F64).expand_as(ref)
    err = (got - ref).abs()
    frac = float(torch.where(err == 0, torch.zeros_like(err), err / bound).max())
    print(f"{name}: {frac:.3f} of its bound {detail or ''}")
    within(name, frac, 1.0, detail)


_REF = {}


def cached(key, fn):
    if key not in _REF:
        _REF[key] = fn()
    return _REF[key]


# =========================================================================================== GroupNorm + GELU
# Plain tolerances.  The gradients into dgamma / dbeta land on a non-zero base with one atomic addition per (batch row, chunk)
# workgroup and call: 2 B nchunks additions, each rounding at most u (|base| + 2 |grad|) - added to the gradient tolerance.
def _run_groupnorm(dev, shape, dtype, kind, eps, tag):
    ops = _ops()
    B, T, C, G = shape
    n = T * C
    x, dy, gamma, beta = R.gn_inputs(shape, dtype, kind)
    ref = cached(("gn", shape, dtype, kind, eps), lambda: R.gn_ref(x, dy, gamma, beta, G, eps))
    nch = ops.groupnorm_chunks(T)
    assert nch == R.gn_chunks(T)
    # four distinct batch strides > T*C and four distinct non-zero offsets (whole 16-byte vectors in either dtype)
    X = Buf(dev, n, dtype, x, B, n + 8, 8)
    DY = Buf(dev, n, dtype, dy, B, n + 16, 16)
    Y = Buf(dev, n, dtype, None, B, n + 24, 24)
    DX = Buf(dev, n, dtype, None, B, n + 32, 32)
    gm, bt = Buf(dev, C, F32, gamma), Buf(dev, C, F32, beta)
    stats, sums = Buf(dev, B * G * 2, F32), Buf(dev, B * G * 2, F32)
    part = Buf(dev, B * nch * G * 2, F32)
    base_g, base_b = R.randn((C,), 106).float(), R.randn((C,), 107).float()
    DG, DB = Buf(dev, C, F32, base_g), Buf(dev, C, F32, base_b)
    ops.groupnorm_gelu_fwd(X.t, X.sb, gm.v, bt.v, Y.t, Y.sb, stats.v, part.v, B, T, C, G, eps=eps, x_off=X.off, y_off=Y.off)
    for _ in range(2):
        ops.groupnorm_gelu_bwd(X.t, X.sb, DY.t, DY.sb, gm.v, bt.v, stats.v, DX.t, DX.sb, DG.v, DB.v, part.v, sums.v, B, T, C, G,
                               x_off=X.off, dy_off=DY.off, dx_off=DX.off)
    torch.cuda.synchronize()
    y, dx = Y.rows().reshape(B, T, C), DX.rows().reshape(B, T, C)
    st, sm = stats.rows().reshape(B, G, 2), sums.rows().reshape(B, G, 2)
    d = (shape, dname(dtype), kind, eps)
    if kind == "offset":
        # mean / std = 16.  Bounds: FOUR times the float64 error of the two-pass algorithm emulated in float32 on these inputs
        # (R.gn_offset_bounds; measured on the CPU for fp32: y 7.3e-7, dx 1.0e-6, mean 1.2e-7, rstd 1.25e-7 -> bounds 2.9e-6,
        # 4.0e-6, 4.9e-7, 5.0e-7).  The statistics are fp32 in both dtypes; a bf16 y / dx is dominated by its own output
        # rounding (2^-8) and keeps the plain bf16 tolerance.
        ob, _ = cached(("gnob", dtype), lambda: R.gn_offset_bounds(dtype, eps))
        check(f"w2vk groupnorm offset mean {tag}", st[..., 0], ref["stats"][..., 0], ob["mean"], d)
        rel = ((st[..., 1].double() - ref["stats"][..., 1]) / ref["stats"][..., 1]).abs().max()
        print(f"offset rstd relative error {float(rel):.3e} (bound {ob['rstd']:.3e})")
        within(f"w2vk groupnorm offset rstd {tag}", float(rel), ob["rstd"], d)
        check(f"w2vk groupnorm offset y {tag}", y, ref["y"], ob["y"] if dtype == F32 else R.tol_fwd(dtype), d)
        check(f"w2vk groupnorm offset dx {tag}", dx, ref["dx"], ob["dx"] if dtype == F32 else R.tol_grad(dtype), d)
    else:
        check(f"w2vk groupnorm y {tag}", y, ref["y"], R.tol_fwd(dtype), d)
        check(f"w2vk groupnorm dx {tag}", dx, ref["dx"], R.tol_grad(dtype), d)
        check(f"w2vk groupnorm mean {tag}", st[..., 0], ref["stats"][..., 0], R.tol_fwd(F32), d)
        check(f"w2vk groupnorm rstd {tag}", st[..., 1], ref["stats"][..., 1], R.tol_fwd(F32), d)
    check(f"w2vk groupnorm sums[0] {tag}", sm[..., 0], ref["sums"][..., 0], R.tol_grad(dtype), d)
    check(f"w2vk groupnorm sums[1] {tag}", sm[..., 1], ref["sums"][..., 1], R.tol_grad(dtype), d)
    for nm, got, base, grad in (("dgamma", DG.rows()[0], base_g, ref["dgamma"]), ("dbeta", DB.rows()[0], base_b, ref["dbeta"])):
        want = base.double() + 2.0 * grad
        bound = R.tol_grad(dtype) * 2.0 * float(grad.abs().max()) + 2 * B * nch * U * float((base.double().abs() + 2.0 * grad.abs()).max())
        check_abs(f"w2vk groupnorm {nm} onto a base, twice {tag}", got, want, bound, d)
    if kind == "const":
        # the constant group: every x equals the pivot and the mean exactly, so xhat = 0, z = beta: y = gelu(beta) to the output's
        # rounding (fp32: erff and three multiplies, 8 u |beta|; bf16: one rounding, 2^-8 |y| for the 8 significant bits, on top of the 1.5e-7 erf), the
        # variance is exactly 0 (the clamp holds it there) and rstd = fl32(1 / sqrt(eps)) bit for bit
        g0, Cg = R.GN_CONST_GROUP, C // G
        want = R.gelu(beta.double()[g0 * Cg:(g0 + 1) * Cg]).expand(B, T, Cg)
        bd = 8 * U * beta.double()[g0 * Cg:(g0 + 1) * Cg].abs().expand(B, T, Cg) + 2.0 ** -140
        if dtype == BF16:
            bd = bd + 2.0 ** -8 * want.abs() + 1e-6
        check_abs(f"w2vk groupnorm constant group y = gelu(beta) {tag}", y[:, :, g0 * Cg:(g0 + 1) * Cg], want, bd, d)
        rs = np.float32(1.0 / math.sqrt(float(np.float32(eps))))
        assert same(st[:, g0, 1], torch.full((B,), float(rs), dtype=F32))
        assert same(st[:, g0, 0], torch.full((B,), R.GN_CONST_VALUE, dtype=F32))
    assert all_guards(X, DY, Y, DX, gm, bt, stats, sums, part, DG, DB)
    assert same(X.t.cpu(), X.host0) and same(DY.t.cpu(), DY.host0)


@pytest.mark.parametrize("name,shape,dtype", R.gn_cases(), ids=[f"{n}-{dname(d)}" for n, _, d in R.gn_cases()])
def test_groupnorm_gelu_every_path(dev, name, shape, dtype):
    _run_groupnorm(dev, shape, dtype, "plain", 1e-5, f"({dname(dtype)})")


@pytest.mark.parametrize("dtype", DTYPES, ids=dname)
@pytest.mark.parametrize("kind,eps", [("plain", 1e-3), ("const", 1e-5), ("offset", 1e-5)], ids=["eps1e-3", "constant-group", "offset-16-sigma"])
def test_groupnorm_gelu_input_classes(dev, kind, eps, dtype):
    _run_groupnorm(dev, R.GN_CLASS_SHAPE, dtype, kind, eps, f"({dname(dtype)})")


# =========================================================================================== FIR stem
@pytest.mark.parametrize("dtype", DTYPES, ids=dname)
@pytest.mark.parametrize("kind", ["plain", "dc"])
@pytest.mark.parametrize("name,shape", R.FIR_SHAPES, ids=[n for n, _ in R.FIR_SHAPES])
def test_fir_stem_every_path(dev, name, shape, kind, dtype):
    """The audio rows are slices [7, 7 + Tin) of a wider NaN-filled buffer (a_sb = Tin + 24 > Tin): a read outside a row puts a
    NaN into the statistics and so into everything.  Gradients land on a non-zero base (one atomic addition per reduce slice:
    at most 8)."""
    ops = _ops()
    B, Tin, C, G = shape
    k, s = R.FIR_K, R.FIR_S
    T, pl, _ = R.same_pad(Tin, k, s)
    audio, w, gamma, beta, dy = R.fir_inputs(shape, dtype, kind)
    ref = cached(("fir", shape, dtype, kind), lambda: R.fir_ref(audio, w, gamma, beta, dy, G, 1e-5))
    wide = torch.full((B, Tin + 24), R.NAN, dtype=F32)
    wide[:, 7:7 + Tin] = audio
    wide_d = wide.to(dev)
    a = wide_d[:, 7:7 + Tin]
    assert a.stride(0) == Tin + 24 and a.shape[1] == Tin
    n = T * C
    W = Buf(dev, k * C, F32, w)
    gm, bt = Buf(dev, C, F32, gamma), Buf(dev, C, F32, beta)
    Y = Buf(dev, n, dtype, None, B, n + 8, 16)
    DY = Buf(dev, n, dtype, dy, B, n + 24, 8)
    stats, sums = Buf(dev, B * G * 2, F32), Buf(dev, B * G * 2, F32)
    part = Buf(dev, B * ops.fir_chunks(T) * G * 2, F32)
    wpart = Buf(dev, ops.fir_gn_workspace_floats(B, T, C), F32)
    base = [R.randn((m,), 207 + i).float() for i, m in enumerate((k * C, C, C))]
    DW, DG, DB = (Buf(dev, b.numel(), F32, b) for b in base)
    ops.fir_groupnorm_gelu_fwd(a, pl, W.v, k, s, gm.v, bt.v, Y.t, Y.sb, stats.v, part.v, B, T, C, G, y_off=Y.off)
    ops.fir_groupnorm_gelu_bwd(a, pl, W.v, k, s, DY.t, DY.sb, gm.v, bt.v, stats.v, DW.v, DG.v, DB.v, part.v, sums.v, wpart.v,
                               B, T, C, G, dy_off=DY.off)
    torch.cuda.synchronize()
    tag, d = f"({kind}, {dname(dtype)})", (shape, kind, dname(dtype))
    st = stats.rows().reshape(B, G, 2)
    check(f"w2vk fir y {tag}", Y.rows().reshape(B, T, C), ref["y"], R.tol_fwd(dtype), d)
    check(f"w2vk fir mean {tag}", st[..., 0], ref["stats"][..., 0], R.tol_fwd(F32), d)
    check(f"w2vk fir rstd {tag}", st[..., 1], ref["stats"][..., 1], R.tol_fwd(F32), d)
    for nm, buf, b0, grad in (("dW", DW, base[0], ref["dW"].reshape(-1)), ("dgamma", DG, base[1], ref["dgamma"]), ("dbeta", DB, base[2], ref["dbeta"])):
        bound = R.tol_grad(dtype) * float(grad.abs().max()) + 8 * U * float((b0.double().abs() + grad.abs()).max())
        check_abs(f"w2vk fir {nm} onto a base {tag}", buf.rows()[0], b0.double() + grad, bound, d)
    assert all_guards(W, gm, bt, Y, DY, stats, sums, part, wpart, DW, DG, DB)
    assert same(wide_d.cpu(), wide)


# =========================================================================================== packs: pure data movement
def _pack_geoms(T, k):
    """(Tp, pad_left / row_off): both zero offsets with the minimal Tp, and both non-zero with three rows of slack."""
    return [(T + k - 1, 0), (T + k - 1 + 5, 2)]


@pytest.mark.parametrize("dtype", DTYPES, ids=dname)
@pytest.mark.parametrize("name,shape", R.PACK_SHAPES, ids=[n for n, _ in R.PACK_SHAPES])
def test_group_pack_and_unpack_are_their_index_maps(dev, name, shape, dtype):
    ops = _ops()
    B, T, C, G, k = shape
    Cg = C // G
    x = R.randn((B * T, C), 601).to(dtype)
    bias = R.randn((C,), 602).float()
    resid = R.randn((B * T, C), 603).to(dtype)
    for Tp, off in _pack_geoms(T, k):
        X = Buf(dev, B * T * C, dtype, x)
        XG = Buf(dev, G * B * Tp * Cg, dtype)
        ops.group_pack(X.v, XG.v, B, T, C, G, Tp, off)
        assert same(XG.rows().reshape(G, B * Tp, Cg), R.pack_ref(x, B, T, C, G, Tp, off)), (Tp, off)
        yg = R.randn((G, B * Tp, Cg), 604).to(dtype)
        YG = Buf(dev, yg.numel(), dtype, yg)
        plain = R.unpack_ref(yg, B, T, C, G, Tp, off)
        RS, BI = Buf(dev, B * T * C, dtype, resid), Buf(dev, C, F32, bias)
        for use_b, use_r in ((False, False), (True, False), (False, True), (True, True)):
            OUT = Buf(dev, B * T * C, dtype)
            ops.group_unpack(YG.v, BI.v if use_b else None, RS.v if use_r else None, OUT.v, B, T, C, G, Tp, off)
            got = OUT.rows().reshape(B * T, C)
            v32 = plain.float()   # the kernel's order in fp32: the value, + bias, + residual
            if use_b:
                v32 = v32 + bias
            if use_r:
                v32 = v32 + resid.float()
            if not (use_b or use_r) or dtype == F32:
                assert same(got, v32.to(dtype)), (Tp, off, use_b, use_r)   # bf16 without addends: the value itself comes back
            else:
                # bf16: one output rounding (2^-8 relative) of a sum that carries at most two fp32 roundings
                exact = plain.double() + (bias.double() if use_b else 0.0) + (resid.double() if use_r else 0.0)
                mag = plain.double().abs() + bias.double().abs() + resid.double().abs()
                check_abs(f"w2vk group_unpack bf16 with addends / one rounding", got, exact, 2.0 ** -8 * exact.abs() + 2 * U * mag + 2.0 ** -133, (shape, Tp, off))
            assert all_guards(OUT)
        assert all_guards(X, XG, YG, RS, BI)


@pytest.mark.parametrize("dtype", DTYPES, ids=dname)
@pytest.mark.parametrize("name,shape", R.PACK_SHAPES, ids=[n for n, _ in R.PACK_SHAPES])
def test_posconv_weight_pack_is_its_index_map(dev, name, shape, dtype):
    ops = _ops()
    _, _, C, G, k = shape
    Cg = C // G
    w = R.randn((k, Cg, C), 611, 0.2).float()
    W = Buf(dev, w.numel(), F32, w, off=24)
    WF, WB = Buf(dev, w.numel(), dtype), Buf(dev, w.numel(), dtype)
    ops.posconv_pack_weights(W.t, WF.v, WB.v, k, Cg, G, w_off=W.off)   # the weights start 24 floats into their buffer
    wf, wb = R.weight_pack_ref(w, k, Cg, G)
    if dtype == BF16:   # the round-to-nearest-even cast of the mapped value
        wf, wb = R.bf16_rne(wf), R.bf16_rne(wb)
    assert same(WF.rows().reshape(G, k * Cg, Cg), wf) and same(WB.rows().reshape(G, k * Cg, Cg), wb)
    assert all_guards(W, WF, WB)


@pytest.mark.parametrize("dtype", DTYPES, ids=dname)
def test_grouped_posconv_chain_with_an_odd_kernel(dev, dtype):
    """tests/test_wav2vec2_gpu.py::test_grouped_posconv_via_packs once more at k = 7, G = 1 (pad 3 + 3), same tolerances."""
    from oracle import wav2vec2_oracle as V
    from oracle import whisper_oracle as O
    ops = _ops()
    B, T, C, G, k = R.PACK_SHAPES[1][1]
    Cg = C // G

    def rnd(shape, seed, dt_=dtype, scale=1.0):
        return R.randn(shape, seed, scale).to(dt_).to(dev)

    def rel_err(got, ref):
        return R.rel_max(got, ref)

    x, w, bias = rnd((B * T, C), 10), rnd((k, Cg, C), 11, F32, 0.2), rnd((C,), 12, F32)
    wf = torch.empty((G, k * Cg, Cg), dtype=dtype, device=dev)
    wb = torch.empty_like(wf)
    ops.posconv_pack_weights(w, wf, wb, k, Cg, G)
    _, pl, pr = O.same_pad(T, k, 1)
    assert (pl, pr) == (3, 3)
    Tp = T + k - 1
    xg = torch.empty((G, B * Tp, Cg), dtype=dtype, device=dev)
    yg = torch.zeros_like(xg)
    ops.group_pack(x, xg, B, T, C, G, Tp, pl)
    M = B * Tp - (k - 1)
    ops.gemm(xg, wf, yg, M, Cg, k * Cg, Cg, 1, Cg, 1, Cg, nbatch=G, a_sb=B * Tp * Cg, b_sb=k * Cg * Cg, c_sb=B * Tp * Cg)
    out = torch.empty((B * T, C), dtype=dtype, device=dev)
    ops.group_unpack(yg, bias, x, out, B, T, C, G, Tp, 0)
    xr = x.double().cpu().reshape(B, T, C).requires_grad_(True)
    wr = (w.to(dtype).double().cpu()).requires_grad_(True)
    ref = xr + V.conv1d_same(xr, wr, bias.double().cpu(), 1, groups=G)
    assert rel_err(out.reshape(B, T, C), ref) <= (2e-5 if dtype == F32 else 1.5e-2)
    dy = rnd((B * T, C), 13)
    ref.backward(dy.double().cpu().reshape(B, T, C))
    dyg = torch.empty_like(xg)
    ops.group_pack(dy, dyg, B, T, C, G, Tp, 0)
    gw = torch.zeros((k, Cg, C), dtype=F32, device=dev)
    ops.gemm(xg, dyg, gw, k * Cg, Cg, M, 1, Cg, Cg, 1, C, nbatch=G, a_sb=B * Tp * Cg, b_sb=B * Tp * Cg, c_sb=Cg, splitk=0)
    Tp2 = T + 2 * (k - 1)
    dyg2 = torch.empty((G, B * Tp2, Cg), dtype=dtype, device=dev)
    dxg2 = torch.zeros_like(dyg2)
    ops.group_pack(dy, dyg2, B, T, C, G, Tp2, k - 1)
    ops.gemm(dyg2, wb, dxg2, B * Tp2 - (k - 1), Cg, k * Cg, Cg, 1, Cg, 1, Cg, nbatch=G, a_sb=B * Tp2 * Cg, b_sb=k * Cg * Cg,
             c_sb=B * Tp2 * Cg)
    dx = torch.empty((B * T, C), dtype=dtype, device=dev)
    ops.group_unpack(dxg2, None, dy, dx, B, T, C, G, Tp2, pl)
    torch.cuda.synchronize()
    gtol = 1e-4 if dtype == F32 else 2e-2
    assert rel_err(gw, wr.grad) <= gtol
    assert rel_err(dx.reshape(B, T, C), xr.grad) <= gtol


# =========================================================================================== vector quantiser
def _perplexity_check(name, got, idx, Nc, detail):
    """fp32 perplexity against float64: per group the sum of Nc terms p log p is spread over 256 threads (ceil(Nc / 256) terms
    each), folded in 9 steps, each term carrying a division, a logarithm and a product (3 roundings): relative error of
    exp(-s) <= (ceil(Nc / 256) + 12) u sum|p log p|, plus expf, the mean over groups and the final division (8 u)."""
    ref = R.perplexity_ref(idx, Nc)
    rows = idx.shape[0]
    sabs = 0.0
    for g in range(idx.shape[1]):
        p = (torch.bincount(idx[:, g].long(), minlength=Nc).double() / rows).clamp(1e-10, 1.0)
        sabs = max(sabs, float((p * torch.log(p + 1e-10)).abs().sum()))
    bound = ((-(-Nc // 256) + 12) * sabs + 8) * U
    rel = abs(float(got) - ref) / ref
    print(f"{name}: perplexity {float(got):.6f} vs {ref:.6f}, rel {rel:.2e} (bound {bound:.2e})")
    within(name, rel / bound, 1.0, detail)


@pytest.mark.parametrize("dtype", DTYPES, ids=dname)
@pytest.mark.parametrize("ties", [False, True], ids=["random", "planted-ties"])
@pytest.mark.parametrize("name,shape", R.VQ_SHAPES, ids=[n for n, _ in R.VQ_SHAPES])
def test_vq_nearest_against_float64_distances(dev, name, shape, ties, dtype):
    ops = _ops()
    rows, G, Nc, gd = shape
    h, cb, tie_rows = R.vq_inputs(shape, dtype, ties)
    dist = cached(("vq", shape, dtype, ties), lambda: R.vq_dist(h, cb))
    H, CB = Buf(dev, h.numel(), dtype, h), Buf(dev, cb.numel(), F32, cb)
    IDX, Q, P = Buf(dev, rows * G, torch.int32), Buf(dev, h.numel(), dtype), Buf(dev, 1, F32)
    ops.vq_nearest(H.v, CB.v, IDX.v, Q.v, P.v, rows, G, Nc, gd)
    torch.cuda.synchronize()
    idx = IDX.rows().reshape(rows, G)
    ok, decisive = R.vq_judge(idx, dist, gd)
    assert bool(ok.all()), (idx[~ok], R.vq_argmin(dist)[~ok])
    if ties:
        # the copies of code c at c + 1 (the neighbouring lane) and c + 64 (the same lane, a later round) are bit-identical
        # rows: equal fp32 sums, and the first index must win - within a lane (strict <) and across lanes (oi < bi)
        on_c = R.vq_tie_rows(dist, gd)
        assert bool(on_c[tie_rows].all()) and bool((idx[on_c] == R.VQ_TIE_CODE).all()), idx[on_c]
    else:
        assert float((~decisive).any(dim=1).double().mean()) <= 0.01
    chosen = torch.stack([cb[g][idx[:, g].long()] for g in range(G)], 1).reshape(rows, G * gd)
    assert same(Q.rows().reshape(rows, G * gd), chosen if dtype == F32 else R.bf16_rne(chosen))
    _perplexity_check("w2vk vq_nearest perplexity / bound", P.rows()[0, 0], idx, Nc, (shape, dname(dtype), ties))
    assert all_guards(H, CB, IDX, Q, P) and same(H.t.cpu(), H.host0) and same(CB.t.cpu(), CB.host0)


@pytest.mark.parametrize("dtype", DTYPES, ids=dname)
@pytest.mark.parametrize("pattern", ["one-code", "spread", "out-of-range"])
@pytest.mark.parametrize("name,shape", R.VQ_SHAPES, ids=[n for n, _ in R.VQ_SHAPES])
def test_vq_assign_and_perplexity(dev, name, shape, pattern, dtype):
    """tmi_vq_assign with the code choice given.  "out-of-range": indices -1 and Nc among valid ones - the assign kernel clamps
    them to 0 and Nc - 1, and the perplexity kernel counts the clamped code (it used to index its LDS table with the raw
    value: Nc was counted for the next group, -1 and the last group's Nc fell outside the table)."""
    ops = _ops()
    rows, G, Nc, gd = shape
    _, cb, _ = R.vq_inputs(shape, dtype)
    if pattern == "out-of-range":
        idx = R.perplexity_patterns(rows, G, Nc)["spread"].clone()
        idx[0::5, 0] = -1
        idx[1::5, G - 1] = Nc
        idx[2, :] = Nc
        eff = idx.clamp(0, Nc - 1)
    else:
        idx = eff = R.perplexity_patterns(rows, G, Nc)[pattern]
    CB, IDX = Buf(dev, cb.numel(), F32, cb), Buf(dev, rows * G, torch.int32, idx)
    Q, P = Buf(dev, rows * G * gd, dtype), Buf(dev, 1, F32)
    ops.vq_assign(CB.v, IDX.v, Q.v, P.v, rows, G, Nc, gd)
    torch.cuda.synchronize()
    chosen = torch.stack([cb[g][eff[:, g].long()] for g in range(G)], 1).reshape(rows, G * gd)
    assert same(Q.rows().reshape(rows, G * gd), chosen if dtype == F32 else R.bf16_rne(chosen))
    _perplexity_check(f"w2vk vq_assign perplexity / bound ({pattern})", P.rows()[0, 0], eff, Nc, (shape, dname(dtype)))
    assert all_guards(CB, IDX, Q, P) and same(IDX.t.cpu(), IDX.host0)


@pytest.mark.parametrize("dtype", DTYPES, ids=dname)
def test_vq_bwd_wrapped_grid_onto_a_base(dev, dtype):
    """rows = 1100, G = 2, gd = 256: 563 200 elements = 2200 blocks of 256 > the 2048-block cap, so the grid-stride loop takes a
    second round; 16 codes: ~69 rows land on each.  Bound per element: the n rows of a code arrive as n atomic additions in
    any order onto the base, each rounding at most u (|base| + sum|terms|): n u (|base| + sum|terms|)."""
    ops = _ops()
    rows, G, Nc, gd = R.VQ_BWD_SHAPE
    idx = R.perplexity_patterns(rows, G, Nc)["spread"]
    dq = R.randn((rows, G * gd), 311).to(dtype)
    base = R.randn((G, Nc, gd), 312).float()
    s, a, n = R.vq_scatter_ref(idx, dq, Nc)
    IDX, DQ, DCB = Buf(dev, rows * G, torch.int32, idx), Buf(dev, dq.numel(), dtype, dq), Buf(dev, base.numel(), F32, base)
    ops.vq_bwd(IDX.v, DQ.v, DCB.v, rows, G, Nc, gd)
    torch.cuda.synchronize()
    bound = n[..., None] * U * (base.double().abs() + a) * (1 + 2.0 ** -16)
    check_abs(f"w2vk vq_bwd onto a base / bound", DCB.rows().reshape(G, Nc, gd), base.double() + s, bound, dname(dtype))
    assert all_guards(IDX, DQ, DCB)


# =========================================================================================== contrastive loss
_CONTRASTIVE = [(n, s, k) for n, s in R.CONTRASTIVE_SHAPES for k in (("plain", "large", "dominant") if s[1] >= 150 else ("plain",))]


@pytest.mark.parametrize("name,shape,kind", _CONTRASTIVE, ids=[f"{n}-{k}" for n, _, k in _CONTRASTIVE])
def test_contrastive_rows_and_gradient_entry_by_entry(dev, name, shape, kind):
    """row_loss per row against float64 (2e-5 of max|ref|) and the rewritten S entry by entry (1e-4 of the largest sum of |terms|
    behind an entry: that is max|ref| except where the terms of one entry cancel - T = 1, where t is its own negative three
    times and dS is 0 up to rounding).  With no negatives both references are all zeros and so must the outputs be; entries
    at unsampled columns are exactly +0.0."""
    ops = _ops()
    B, T, Nn, per_time = shape
    S, neg = R.contrastive_inputs(shape, kind)
    loss, dS, sampled, dS_abs = cached(("con", shape, kind), lambda: R.contrastive_ref(S, neg, R.CONTRASTIVE_TEMP, R.CONTRASTIVE_GRAD_SCALE, per_time))
    SB, RL = Buf(dev, S.numel(), F32, S), Buf(dev, B * T, F32)
    NG = Buf(dev, max(neg.numel(), 1), torch.int32, neg if neg.numel() else None)
    ops.contrastive_fwd_bwd(SB.v, NG.v, RL.v, B, T, Nn, R.CONTRASTIVE_TEMP, R.CONTRASTIVE_GRAD_SCALE, per_time=per_time)
    torch.cuda.synchronize()
    got = SB.rows().reshape(B, T, T)
    check(f"w2vk contrastive row_loss ({kind})", RL.rows()[0], loss, R.tol_fwd(F32), shape)
    check_abs(f"w2vk contrastive dS ({kind}) / bound", got, dS, R.tol_grad(F32) * float(dS_abs.max()), shape)
    assert not bool(bits(got)[~sampled].any()), "a non-zero (or -0.0) at a column that was not sampled"
    assert all_guards(SB, RL, NG)


# =========================================================================================== segment sums and clip
def test_segment_sums_and_clip_unaligned_empty_and_short(dev):
    """Offsets [0, 101, 101, 103, 4001, 60000]: starts that are no multiple of 4 (the scalar path), an empty segment, a
    2-element one (15 of its 16 slices empty).  Sum bound: R.segment_sum_bound."""
    ops = _ops()
    offs = R.SEG_OFFSETS
    nseg = len(offs) - 1
    g = R.seg_inputs()
    exact = R.segment_sumsq_ref(g, offs)
    lens = [b - a for a, b in zip(offs[:-1], offs[1:])]
    G_ = Buf(dev, g.numel(), F32, g)
    offs_d = torch.tensor(offs, dtype=torch.int64, device=dev)
    S1, S2 = Buf(dev, nseg, F32), Buf(dev, nseg, F32)
    ops.segment_sumsq(G_.v, offs_d, S1.v, nseg)
    chunks = ops.segment_chunks(offs, device=dev)
    ops.segment_sumsq_chunks(G_.v, chunks, S2.v, nseg)
    torch.cuda.synchronize()
    b1 = torch.tensor([R.segment_sum_bound(n, 16, e) for n, e in zip(lens, exact)], dtype=F64)
    nck = [int((chunks[:, 2] == s_).sum()) for s_ in range(nseg)]
    b2 = torch.tensor([R.segment_sum_bound(min(n, 8192), 1, e, natomics=c) for n, e, c in zip(lens, exact, nck)], dtype=F64)
    check_abs("w2vk segment_sumsq / bound", S1.rows()[0], exact, b1 + 2.0 ** -149)
    check_abs("w2vk segment_sumsq_chunks / bound", S2.rows()[0], exact, b2 + 2.0 ** -149)
    assert float(S1.rows()[0, 1]) == 0.0 and float(S2.rows()[0, 1]) == 0.0   # the empty segment
    assert same(G_.t.cpu(), G_.host0)
    # clip with the kernel's own sums
    ss = S1.rows()[0].clone()
    ops.segment_clip(G_.v, offs_d, S1.v, nseg, R.SEG_CLIP)
    torch.cuda.synchronize()
    got = G_.rows()[0]
    scale = R.clip_scale_f32(ss.numpy(), R.SEG_CLIP)
    assert [float(x) == 1.0 for x in scale] == [True, True, True, False, False]
    for s_, (a, b) in enumerate(zip(offs[:-1], offs[1:])):
        # a clipped element is g * fl32(clip / max(sqrt(ss), clip)) bit for bit; below the threshold that scale is 1 and the
        # segment is bit-unchanged (g * 1 == g, so one expression covers both)
        assert same(got[a:b], g[a:b] * float(scale[s_])), s_
        if scale[s_] == 1.0:
            assert same(got[a:b], g[a:b])
        else:   # the scale against float64: half the relative error of the sum (sqrt) plus sqrt, max, division (3 u)
            s64 = R.SEG_CLIP / max(math.sqrt(float(exact[s_])), R.SEG_CLIP)
            within("w2vk segment_clip scale / bound", abs(float(scale[s_]) - s64) / (s64 * (0.5 * float(b1[s_] / exact[s_]) + 3 * U)), 1.0, s_)
    assert all_guards(G_, S1, S2)   # (the neighbours of the empty segment are covered by the segment-by-segment equality)


def test_one_big_segment_runs_both_unrolled_loops(dev):
    """nseg == 1 over 1 700 000 elements: 512 slices of 3324 elements = 831 float4, so threads 0 .. 62 run the
    four-loads-in-flight round of segment_sumsq and of segment_clip (831 > 768) and the single-step loop finishes."""
    ops = _ops()
    n = R.SEG_BIG_N
    g = R.seg_inputs(n, 502)
    exact = float((g.double() ** 2).sum())
    G_ = Buf(dev, n, F32, g)
    one = torch.tensor([0, n], dtype=torch.int64, device=dev)
    SS = Buf(dev, 1, F32)
    ops.segment_sumsq(G_.v, one, SS.v, 1)
    torch.cuda.synchronize()
    ss = SS.rows()[0].clone()
    bound = R.segment_sum_bound(n, 512, exact)
    check_abs("w2vk segment_sumsq one segment / bound", ss, torch.tensor([exact], dtype=F64), bound)
    ops.segment_clip(G_.v, one, SS.v, 1, R.SEG_CLIP)
    torch.cuda.synchronize()
    scale = R.clip_scale_f32(ss.numpy(), R.SEG_CLIP)
    assert float(scale[0]) < 1.0 and same(G_.rows()[0], g * float(scale[0]))
    s64 = R.SEG_CLIP / math.sqrt(exact)
    within("w2vk segment_clip scale / bound", abs(float(scale[0]) - s64) / (s64 * (0.5 * bound / exact + 3 * U)), 1.0, "big")
    # a sum below the threshold: the early return leaves the gradient bit-unchanged
    before = G_.t.clone()
    SS.v.fill_(0.25)
    ops.segment_clip(G_.v, one, SS.v, 1, R.SEG_CLIP)
    torch.cuda.synchronize()
    assert same(G_.t, before) and all_guards(G_, SS)


# =========================================================================================== rejections, by return code
def test_bad_arguments_are_refused_before_any_launch(dev):
    """One call per condition of gn_check, fir_check and the _impl functions; the buffers would hold every call as written."""
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import _lib
    L = _lib.lib()
    f = [torch.zeros(1 << 16, dtype=F32, device=dev) for _ in range(6)]
    h = [torch.zeros(1 << 16, dtype=BF16, device=dev) for _ in range(3)]
    i32 = torch.zeros(4096, dtype=torch.int32, device=dev)
    i64 = torch.zeros(16, dtype=torch.int64, device=dev)
    a, b, c, d, e, w = (t.data_ptr() for t in f)
    ha, hb, hc = (t.data_ptr() for t in h)
    ip, lp = i32.data_ptr(), i64.data_ptr()
    FP, BF = _lib.TMI_F32, _lib.TMI_BF16
    gn_f = lambda x=a, xsb=256, y=b, ysb=256, B=2, T=4, C=64, G=4, dt_=FP: L.tmi_groupnorm_gelu_fwd(x, xsb, c, c, y, ysb, d, e, B, T, C, G, 1e-5, dt_, None)
    gn_b = lambda dxsb=256, dy=b, G=4: L.tmi_groupnorm_gelu_bwd(a, 256, dy, 256, c, c, d, e, dxsb, w, w, d, d, 2, 4, 64, G, FP, None)
    fir_f = lambda k=10, s=5, C=64, G=2, ysb=64 * 8, pl=2, wp=w: L.tmi_fir_groupnorm_gelu_fwd(a, 40, 40, pl, wp, k, s, c, c, b, ysb, d, e, 2, 8, C, G, 1e-5, FP, None)
    fir_b = lambda s=5, dysb=64 * 8: L.tmi_fir_groupnorm_gelu_bwd(a, 40, 40, 2, w, 10, s, b, dysb, c, c, d, e, e, e, d, d, f[4].data_ptr(), 2, 8, 64, 2, FP, None)
    calls = {
        "groupnorm fwd, 1024 % C != 0 (C = 96)": (b"tmi_groupnorm_gelu_fwd", lambda: gn_f(C=96, G=4, xsb=384, ysb=384)),
        "groupnorm fwd, x 4 bytes off a 16-byte boundary": (b"tmi_groupnorm_gelu_fwd", lambda: gn_f(x=a + 4)),
        "groupnorm fwd, y misaligned": (b"tmi_groupnorm_gelu_fwd", lambda: gn_f(y=b + 8)),
        "groupnorm fwd, C % G != 0": (b"tmi_groupnorm_gelu_fwd", lambda: gn_f(G=3)),
        "groupnorm fwd, C / G = 4 in bf16 (half a vector)": (b"tmi_groupnorm_gelu_fwd", lambda: gn_f(x=ha, y=hb, G=16, dt_=BF)),
        "groupnorm fwd, G = 512 > 256": (b"tmi_groupnorm_gelu_fwd", lambda: gn_f(C=2048, G=512, xsb=8192, ysb=8192, B=1, T=2)),
        "groupnorm fwd, x_sb = 258 (no whole vectors)": (b"tmi_groupnorm_gelu_fwd", lambda: gn_f(xsb=258)),
        "groupnorm fwd, B = 65536": (b"tmi_groupnorm_gelu_fwd", lambda: gn_f(B=65536)),
        "groupnorm bwd, dx_sb = 258": (b"tmi_groupnorm_gelu_bwd", lambda: gn_b(dxsb=258)),
        "groupnorm bwd, dy misaligned": (b"tmi_groupnorm_gelu_bwd", lambda: gn_b(dy=b + 4)),
        "fir fwd, kernel 9": (b"tmi_fir_groupnorm_gelu_fwd", lambda: fir_f(k=9)),
        "fir fwd, stride 4": (b"tmi_fir_groupnorm_gelu_fwd", lambda: fir_f(s=4)),
        "fir fwd, 2048 % C != 0 (C = 24)": (b"tmi_fir_groupnorm_gelu_fwd", lambda: fir_f(C=24, G=3, ysb=24 * 8)),
        "fir fwd, C / G = 4": (b"tmi_fir_groupnorm_gelu_fwd", lambda: fir_f(G=16)),
        "fir fwd, y_sb % 8 != 0": (b"tmi_fir_groupnorm_gelu_fwd", lambda: fir_f(ysb=64 * 8 + 4)),
        "fir fwd, pad_left < 0": (b"tmi_fir_groupnorm_gelu_fwd", lambda: fir_f(pl=-1)),
        "fir fwd, taps misaligned": (b"tmi_fir_groupnorm_gelu_fwd", lambda: fir_f(wp=w + 4)),
        "fir bwd, stride 4": (b"tmi_fir_groupnorm_gelu_bwd", lambda: fir_b(s=4)),
        "fir bwd, dy_sb % 8 != 0": (b"tmi_fir_groupnorm_gelu_bwd", lambda: fir_b(dysb=64 * 8 + 2)),
        "group_pack, Tp < T + pad_left": (b"tmi_group_pack", lambda: L.tmi_group_pack(a, b, 2, 8, 16, 2, 9, 2, FP, None)),
        "group_pack, C % G != 0": (b"tmi_group_pack", lambda: L.tmi_group_pack(a, b, 2, 8, 16, 3, 12, 2, FP, None)),
        "group_unpack, Tp < T + row_off": (b"tmi_group_unpack", lambda: L.tmi_group_unpack(a, None, None, b, 2, 8, 16, 2, 9, 2, FP, None)),
        "group_unpack, row_off < 0": (b"tmi_group_unpack", lambda: L.tmi_group_unpack(a, None, None, b, 2, 8, 16, 2, 12, -1, FP, None)),
        "posconv_pack_weights, k = 0": (b"tmi_posconv_pack_weights", lambda: L.tmi_posconv_pack_weights(a, b, c, 0, 8, 2, FP, None)),
        "vq_nearest, G * Nc > 8192": (b"tmi_vq_nearest", lambda: L.tmi_vq_nearest(a, b, ip, c, d, 4, 2, 4097, 4, FP, None)),
        "vq_nearest, gd > 1024": (b"tmi_vq_nearest", lambda: L.tmi_vq_nearest(a, b, ip, c, d, 4, 1, 4, 1025, FP, None)),
        "vq_assign, rows = 0": (b"tmi_vq_assign", lambda: L.tmi_vq_assign(a, ip, c, d, 0, 2, 4, 4, FP, None)),
        "vq_assign, G * Nc > 8192": (b"tmi_vq_assign", lambda: L.tmi_vq_assign(a, ip, c, d, 4, 2, 4097, 4, FP, None)),
        "vq_bwd, gd = 0": (b"tmi_vq_bwd", lambda: L.tmi_vq_bwd(ip, a, b, 4, 2, 4, 0, FP, None)),
        "contrastive, T > 8192": (b"tmi_contrastive_fwd_bwd", lambda: L.tmi_contrastive_fwd_bwd(a, ip, 2, 0, b, 1, 8193, 2, 0.1, 1.0, None)),
        "contrastive, Nn > 4096": (b"tmi_contrastive_fwd_bwd", lambda: L.tmi_contrastive_fwd_bwd(a, ip, 4097, 0, b, 1, 4, 4097, 0.1, 1.0, None)),
        "contrastive, temperature 0": (b"tmi_contrastive_fwd_bwd", lambda: L.tmi_contrastive_fwd_bwd(a, ip, 2, 0, b, 1, 4, 2, 0.0, 1.0, None)),
        "contrastive, negative index stride": (b"tmi_contrastive_fwd_bwd", lambda: L.tmi_contrastive_fwd_bwd(a, ip, -2, 0, b, 1, 4, 2, 0.1, 1.0, None)),
        "segment_sumsq, nseg = 0": (b"tmi_segment_sumsq", lambda: L.tmi_segment_sumsq(a, lp, b, 0, None)),
        "segment_sumsq, nseg = 65536": (b"tmi_segment_sumsq", lambda: L.tmi_segment_sumsq(a, lp, b, 65536, None)),
        "segment_sumsq_chunks, no chunks": (b"tmi_segment_sumsq_chunks", lambda: L.tmi_segment_sumsq_chunks(a, lp, 0, b, 1, None)),
        "segment_clip, clip = 0": (b"tmi_segment_clip", lambda: L.tmi_segment_clip(a, lp, b, 1, 0.0, None)),
    }
    for t in f + h:
        t.fill_(3.0)
    i32.fill_(1)
    torch.cuda.synchronize()
    for what, (who, call) in calls.items():
        rc = call()
        assert rc == TMI_ERR_INVALID, (what, rc)
        msg = L.tmi_last_error()
        assert msg and msg.startswith(who), (what, msg)
    torch.cuda.synchronize()
    three32, three16 = torch.full((1 << 16,), 3.0, dtype=F32), torch.full((1 << 16,), 3.0, dtype=BF16)
    assert all(same(t, three32) for t in f) and all(same(t, three16) for t in h)
    assert bool((i32.cpu() == 1).all()) and bool((i64.cpu() == 0).all())
