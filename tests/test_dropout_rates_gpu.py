"""Every consumer of the dropout generator of csrc/tmi_common.h at every rate of tests/_layout_ref.RATES: tmi_dropout's two
kernels, the GEMM epilogue term (tmi_drop1 of gemm_epilogue.h, tmi_drop8 / tmi_drop1 of gemm_fast.hip), the fused LayerNorm
passes, tmi_layernorm_bwd_emit and the attention kernels, whose keep_pair tests two signed 16-bit draws against
tm1 = ((thr - 32768 - 1) & 0xffff) * 0x10001: thr = 1 makes tm1 the most negative int16, 32767 / 32768 / 32769 straddle the
sign, 65535 is the last accepted threshold with the keep scale 65536.

Masks are compared bit for bit with oracle/dropout.py.  Values: tmi_dropout on the bits (_layout_ref.dropout_expected), the
GEMM term against tests/_gemm_ref.gemm_ref's per-element bound, LayerNorm against tests/_row_kernel_ref.py's, attention through
the Case harness of tests/test_attention_forms_gpu.py (twice the bf16 restatement's own error).  tests/test_layout_ref_cpu.py
asserts that each of these masks holds kept and dropped elements at every rate.

Then the "off" rule - p > 0 whose threshold is 0 behaves exactly like p = 0, and attention accepts it without a drop_mask -
and the refusals: p = 0.999995 (threshold 65536), p = 1, p < 0 and NaN are TMI_ERR_INVALID at every site, nothing written."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import _gemm_ref as GR
import _layout_ref as L
import _row_kernel_ref as R
from _margins import within
from test_attention_forms_gpu import Canaried, Case, _refused, gaussian  # noqa: E402
from test_kernels_gpu import gemm_path  # noqa: E402
from test_layout_kernels_gpu import PAD, Buf, rows_idx  # noqa: E402
from test_row_kernels_gpu import G, report, same  # noqa: E402

pytestmark = pytest.mark.gpu

F32, BF16, F64 = L.F32, L.BF16, L.F64
DTYPES = [F32, BF16]
TMI_ERR_INVALID = -1  # include/tethys_mi.h
WIDE = 32             # TMI_GEMM_PATH_WIDE
rates = pytest.mark.parametrize("thr,p", L.RATES, ids=L.RATE_IDS)


def _mods():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import _lib, ops
    return ops, _lib


def _DO():
    from oracle import dropout as DO
    return DO


_KEEP = {}


def keep_flat(seed, rows, cols, p):
    k = (seed, rows, cols, p)
    if k not in _KEEP:
        _KEEP[k] = torch.from_numpy(_DO().keep_flat(seed, rows, cols, p))
    return _KEEP[k]


# =========================================================================================== tmi_dropout
def _flat_inputs(rows, cols, dtype):
    return (R.to_dtype(R.randn((rows, cols), 90), dtype), R.to_dtype(R.randn((rows, cols), 91), dtype),
            R.to_dtype(R.randn((rows, cols), 92), dtype))


def _run_dropout(dev, x, resid, p, seed, in_place=False):
    ops, _ = _mods()
    rows, cols = x.shape
    xd = x.to(dev)
    out = xd if in_place else torch.full_like(xd, 7.0)
    ops.dropout(xd, out, rows, cols, p, seed, resid=None if resid is None else resid.to(dev))
    torch.cuda.synchronize()
    return out.cpu()


@rates
@pytest.mark.parametrize("dtype", DTYPES, ids=R.dname)
@pytest.mark.parametrize("rows,cols", L.FLAT_SHAPES, ids=["pair-kernel", "16-byte-kernel"])
def test_dropout_kernels_at_every_rate(dev, rows, cols, dtype, thr, p):
    DO = _DO()
    assert DO.drop_thr(p) == thr and ((cols % 8 == 0) == (cols == 1024))
    keep, sc = keep_flat(L.FLAT_SEED, rows, cols, p), DO.keep_scale(p)
    x, resid, g = _flat_inputs(rows, cols, dtype)
    for res in (None, resid):
        out = _run_dropout(dev, x, res, p, L.FLAT_SEED)
        assert L.same_bits(out, L.dropout_expected(x, res, keep, sc, dtype)), ("resid" if res is not None else "plain")
        want0 = res if res is not None else torch.zeros_like(x)
        assert L.same_bits(out[~keep], want0[~keep]), "a dropped position holds exactly the residual, or +0"
    # in place, and the backward use: the same call on a gradient reproduces the mask
    out = _run_dropout(dev, g, None, p, L.FLAT_SEED, in_place=True)
    assert L.same_bits(out, L.dropout_expected(g, None, keep, sc, dtype))
    assert torch.equal(out != 0, keep & (g != 0))


# =========================================================================================== GEMM epilogue term
# name -> operand layout and the kernel tmi_gemm_last_path must report.  "small" and "resid" are whole 8-column chunks on the
# fast kernels (tmi_drop8: the lean RESID class in interior pieces, the generic pass at the ragged edge N = 96 = 64 + 32);
# "generic" has weight rows 100 elements apart, no multiple of 8, so tmi_gemm_fast_try declines and gemm.hip's kernel with
# gemm_epilogue.h's tmi_drop1 runs; "narrow-tail" (blocks.py's _gemm_xw form, N = 108) ends in a chunk of 4 columns, which the
# fast epilogue finishes element by element: gemm_fast.hip's tmi_drop1 lines.
GEMM_LAYOUT = {"small": (None, (12, 1, WIDE)), "generic": (None, (1, 1, 0)), "resid": (None, (15, 1, WIDE)),
               "narrow-tail": (dict(ld_a=584, ldw=264, b_off=64, ldc=120, r_ld=136), (15, 1, WIDE))}
_GEMM_IN = {}


def _gemm_inputs(name):
    if name not in _GEMM_IN:
        M, N, K, _ = L.GEMM_RATE_CASES[name]
        lay = GEMM_LAYOUT[name][0] or dict(ld_a=K, ldw=N, b_off=0, ldc=N, r_ld=N)
        _GEMM_IN[name] = dict(lay, A=R.to_dtype(R.randn((M, lay["ld_a"]), 1, 0.5), BF16),
                              W=R.to_dtype(R.randn((K, lay["ldw"]), 2, 1.0 / math.sqrt(K)), BF16),
                              bias=R.randn((N,), 3, 0.1).float(), resid=R.to_dtype(R.randn((M, lay["r_ld"]), 4), BF16))
    return _GEMM_IN[name]


def _gemm_run(dev, name, p, seed):
    ops, _ = _mods()
    M, N, K, _ = L.GEMM_RATE_CASES[name]
    g = _gemm_inputs(name)
    Cb = Buf(dev, BF16, M * g["ldc"])
    dv = {k: g[k].to(dev) for k in ("A", "W", "bias", "resid")}
    ops.gemm(dv["A"], dv["W"], Cb.t, M, N, K, g["ld_a"], 1, g["ldw"], 1, g["ldc"], bias=dv["bias"], resid=dv["resid"], r_ld=g["r_ld"],
             b_off=g["b_off"], c_off=PAD, dropout_p=p, dropout_seed=seed)
    path = gemm_path()
    torch.cuda.synchronize()
    return Cb, path


def _gemm_ref(name, p, seed):
    M, N, K, _ = L.GEMM_RATE_CASES[name]
    g = _gemm_inputs(name)
    f = lambda t: t.double().reshape(-1).numpy()   # noqa: E731
    return GR.gemm_ref(f(g["A"]), f(g["W"]), np.zeros(M * g["ldc"]), M, N, K, g["ld_a"], 1, g["ldw"], 1, g["ldc"], bias=f(g["bias"]),
                       resid=f(g["resid"]), r_ld=g["r_ld"], b_off=g["b_off"], dropout_p=p, dropout_seed=seed)


@rates
@pytest.mark.parametrize("name", list(L.GEMM_RATE_CASES))
def test_gemm_epilogue_dropout_at_every_rate(dev, name, thr, p):
    M, N, K, seed = L.GEMM_RATE_CASES[name]
    g = _gemm_inputs(name)
    Cb, path = _gemm_run(dev, name, p, seed)
    assert path == GEMM_LAYOUT[name][1], (name, path)
    idx = rows_idx(M, N, g["ldc"])
    got = Cb.t.cpu()[PAD + idx]
    Cb.check(idx, got, ("gemm guards", name, thr))          # the gaps between rows (ldc > N) and the guards keep their values
    ref = _gemm_ref(name, p, seed)
    ratio = GR.worst_ratio(got.double().numpy(), ref["ref"][0, 0], ref["bound"][0, 0])
    print(f"gemm-drop {name} thr {thr}: {ratio:.3f} of its bound")
    within(f"gemm-drop {name}", ratio, 1.0, (thr, path))
    keep = keep_flat(seed, M, N, p)
    assert L.same_bits(got[~keep], g["resid"][:, :N][~keep]), "a dropped position holds exactly the (rounded) residual"


# =========================================================================================== LayerNorm
def _other_rate(thr):
    """Another rate of the table for the Dropout that dy went through: the next one, cyclically."""
    i = [t for t, _ in L.RATES].index(thr)
    return L.RATES[(i + 1) % len(L.RATES)][1]


class _LNRates:
    def __init__(self, dev, dtype):
        rows, Cn = L.LN_RATE_SHAPE
        self.dev, self.dtype, self.rows, self.C = dev, dtype, rows, Cn
        self.inp = inp = R.ln_inputs(rows, Cn, dtype)
        self.X, self.DY = G(dev, dtype, data=inp["x"]), G(dev, dtype, data=inp["dy"])
        self.GM, self.BT = G(dev, F32, data=inp["gamma"]), G(dev, F32, data=inp["beta"])
        self.fw = R.ln_fwd_ref(inp)
        self.m32, self.r32 = self.fw["mean"].float(), self.fw["rstd"].float()
        self.MEAN, self.RSTD = G(dev, F32, data=self.m32), G(dev, F32, data=self.r32)

    def v2(self, g):
        return g.v.view(self.rows, self.C)

    def fwd(self, p, seed):
        """-> y [rows, C], mean, rstd and their guarded buffers; p = 0: tmi_layernorm_fwd."""
        ops, _ = _mods()
        Y, M, S = G(self.dev, self.dtype, n=self.rows * self.C), G(self.dev, F32, n=self.rows), G(self.dev, F32, n=self.rows)
        a = (self.v2(self.X), self.GM.v, self.BT.v, self.v2(Y), M.v, S.v, R.LN_EPS)
        if p is None:
            ops.layernorm_fwd(*a)
        else:
            ops.layernorm_dropout_fwd(*a, p, seed)
        torch.cuda.synchronize()
        return dict(y=Y.get().view(self.rows, self.C), mean=M.get(), rstd=S.get()), (Y, M, S)

    def bwd(self, form, p, seed):
        """form "dropout": tmi_layernorm_dropout_bwd; "emit": tmi_layernorm_bwd_emit with the masked output; "plain"."""
        ops, _ = _mods()
        inp, rows, Cn = self.inp, self.rows, self.C
        DX = G(self.dev, self.dtype, n=rows * Cn, data=inp["old"])
        DG, DB, CS = (G(self.dev, F32, data=b) for b in inp["bases"])
        MK = G(self.dev, self.dtype, n=rows * Cn)
        a = (self.v2(self.DY), self.v2(self.X), self.GM.v, self.MEAN.v, self.RSTD.v, self.v2(DX), DG.v, DB.v)
        if form == "plain":
            ops.layernorm_bwd(*a, accumulate_dx=True)
        elif form == "dropout":
            ops.layernorm_dropout_bwd(*a, p, seed, accumulate_dx=True)
        else:
            ops.layernorm_bwd_emit(*a, CS.v, masked=self.v2(MK), dropout_p=p, dropout_seed=seed, accumulate_dx=True)
        torch.cuda.synchronize()
        out = dict(dx=DX.get().view(rows, Cn), dgamma=DG.get(), dbeta=DB.get(), colsum=CS.get(), masked=MK.get().view(rows, Cn))
        return out, (DX, DG, DB, CS, MK)

    def inputs_untouched(self):
        return all(b.untouched() for b in (self.X, self.DY, self.GM, self.BT, self.MEAN, self.RSTD))


@rates
@pytest.mark.parametrize("dtype", DTYPES, ids=R.dname)
def test_layernorm_dropout_passes_at_every_rate(dev, dtype, thr, p):
    """tmi_layernorm_dropout_fwd at the rate; tmi_layernorm_dropout_bwd with dy dropped at ANOTHER rate of the table;
    tmi_layernorm_bwd_emit with its masked output at the rate.  (ln_bwd_launch takes dropout_p and dy_dropout_p, but no
    exported entry point sets both: the two are reached through these two calls.)"""
    DO, ln = _DO(), _LNRates(dev, dtype)
    rows, Cn = L.LN_RATE_SHAPE
    tag, detail = f"({R.dname(dtype)})", (rows, Cn, R.dname(dtype), thr)
    keep, sc = keep_flat(L.LN_RATE_SEED_Y, rows, Cn, p), DO.keep_scale(p)
    # forward
    plain, _ = ln.fwd(None, 0)
    out, bufs = ln.fwd(p, L.LN_RATE_SEED_Y)
    report(f"ln-rates dropout fwd {tag}", R.ratios_ln_fwd(out, R.ln_fwd_ref(ln.inp, keep, sc)), detail)
    assert same(out["y"][~keep], torch.zeros_like(out["y"][~keep])), "a dropped element is +0"
    assert torch.equal(out["y"] != 0, keep & (plain["y"] != 0))
    assert all(b.guards_ok() for b in bufs)
    # backward of LayerNorm -> Dropout: dy masked on load, at another rate
    p2 = _other_rate(thr)
    keep2, sc2 = keep_flat(L.LN_RATE_SEED_Y, rows, Cn, p2), DO.keep_scale(p2)
    out, bufs = ln.bwd("dropout", p2, L.LN_RATE_SEED_Y)
    ref = R.ln_bwd_ref(ln.inp, ln.m32, ln.r32, True, keep_dy=keep2, scale_dy=sc2)
    report(f"ln-rates dropout bwd {tag}", R.ratios_ln_bwd(out, ref), detail + (DO.drop_thr(p2),))
    assert all(b.guards_ok() for b in bufs[:3]) and bufs[3].untouched() and bufs[4].untouched()
    # emit: dx, and Dropout(dx) for the Dense layer below
    keepm = keep_flat(L.LN_RATE_SEED_MASKED, rows, Cn, p)
    out, bufs = ln.bwd("emit", p, L.LN_RATE_SEED_MASKED)
    ref = R.ln_bwd_ref(ln.inp, ln.m32, ln.r32, True, emit=True, keep=keepm, scale=sc)
    report(f"ln-rates bwd emit masked {tag}", R.ratios_ln_bwd(out, ref), detail)
    assert same(out["masked"][~keepm], torch.zeros_like(out["masked"][~keepm])), "a dropped element is +0"
    assert torch.equal(out["masked"] != 0, keepm & (out["dx"] != 0))
    assert all(b.guards_ok() for b in bufs) and ln.inputs_untouched()


# =========================================================================================== attention
@rates
@pytest.mark.parametrize("B,H,Tq,Tk,mask,seed", L.ATTN_RATE_CASES, ids=["one-launch-bwd", "two-pass", "two-pass-causal", "key-split"])
def test_attention_at_every_rate(dev, B, H, Tq, Tk, mask, seed, thr, p):
    c = Case(dev, B, H, Tq, Tk, mask, p, gaussian(B, H, Tq, Tk, 1400 + Tk), dq_scale=0.5, seed=seed)
    assert ("workspace" in c.bufs) == (Tk == 520)
    c.run_and_compare(f"rates thr{thr} ({B},{H},{Tq}x{Tk}) mask{mask}")
    want = _DO().keep_attention(seed, B, H, Tq, Tk, p)
    got = c.keep()[0]
    assert (got == want).all(), (thr, int((got != want).sum()))


# =========================================================================================== the "off" rule
def test_off_rule_flat_sites(dev):
    """p = 2^-18 > 0 has the threshold 0: tmi_dropout, the GEMM term and the LayerNorm passes give the bits of p = 0."""
    DO = _DO()
    assert DO.drop_thr(L.P_OFF) == 0
    for dtype in DTYPES:
        for rows, cols in L.FLAT_SHAPES:
            x, resid, _ = _flat_inputs(rows, cols, dtype)
            a, b = _run_dropout(dev, x, resid, L.P_OFF, L.FLAT_SEED), _run_dropout(dev, x, resid, 0.0, L.FLAT_SEED)
            assert L.same_bits(a, b) and L.same_bits(a, L.to_dtype(x.float() + resid.float(), dtype))
        ln = _LNRates(dev, dtype)
        plain, _ = ln.fwd(None, 0)
        off, _ = ln.fwd(L.P_OFF, L.LN_RATE_SEED_Y)
        zero, _ = ln.fwd(0.0, L.LN_RATE_SEED_Y)
        assert all(same(off[k], plain[k]) and same(zero[k], plain[k]) for k in ("y", "mean", "rstd"))
        ops, _ = _mods()
        keep0, ops.LN_ATOMIC = ops.LN_ATOMIC, False       # the fixed-order fold: dgamma / dbeta are reproducible
        try:
            base, _ = ln.bwd("plain", 0.0, 0)
            off, _ = ln.bwd("dropout", L.P_OFF, L.LN_RATE_SEED_Y)
            assert all(same(off[k], base[k]) for k in ("dx", "dgamma", "dbeta"))
            e0, _ = ln.bwd("emit", 0.0, L.LN_RATE_SEED_MASKED)
            e1, _ = ln.bwd("emit", L.P_OFF, L.LN_RATE_SEED_MASKED)
            assert all(same(e0[k], e1[k]) for k in ("dx", "dgamma", "dbeta", "colsum", "masked")) and same(e1["masked"], e1["dx"])
        finally:
            ops.LN_ATOMIC = keep0
    for name in L.GEMM_RATE_CASES:
        M, N, K, seed = L.GEMM_RATE_CASES[name]
        (c0, p0), (c1, p1) = _gemm_run(dev, name, 0.0, seed), _gemm_run(dev, name, L.P_OFF, seed)
        assert p0 == p1 == GEMM_LAYOUT[name][1] and torch.equal(L.bits(c0.t), L.bits(c1.t)), name


@pytest.mark.parametrize("B,H,Tq,Tk,mask,seed", L.ATTN_RATE_CASES, ids=["one-launch-bwd", "two-pass", "two-pass-causal", "key-split"])
def test_off_rule_attention_needs_no_drop_mask_and_writes_none(dev, B, H, Tq, Tk, mask, seed):
    inp = gaussian(B, H, Tq, Tk, 1400 + Tk)
    res = []
    for p_off in (None, L.P_OFF):
        c = Case(dev, B, H, Tq, Tk, mask, 0.0, inp, dq_scale=0.5, seed=seed)
        mk = None
        if p_off is not None:
            mk = Canaried(dev, c.lib.tmi_attn_dropmask_bytes(B, H, Tq, Tk), torch.uint8)
        for passed in ((False, True) if p_off is not None else (False,)):
            for entry, d in (("tmi_attn_fwd", c.desc()), ("tmi_attn_bwd", c.bwd_desc())):
                if p_off is not None:
                    d.dropout_p, d.dropout_seed = p_off, seed
                    if passed:   # a buffer that is passed anyway is not written
                        d.drop_mask, d.drop_mask_bytes = mk.body.data_ptr(), mk.n
                assert getattr(c.lib, entry)(C.byref(d), c.ops.stream()) == 0, (entry, p_off, passed)
                torch.cuda.synchronize()
            c.assert_canaries()
            assert mk is None or mk.untouched()
            res.append([c.out_o(), c.bufs["stats"].body.clone().cpu(), c.bufs["delta"].body.clone().cpu()] +
                       [c.out_grad(n) for n in ("dq", "dk", "dv")])
    for other in res[1:]:
        for a, b in zip(res[0], other):
            assert torch.equal(a, b)


# =========================================================================================== refusals
@pytest.mark.parametrize("p", L.P_REFUSED, ids=["thr65536", "one", "negative", "nan"])
def test_refused_rates_write_nothing_at_any_site(dev, p):
    ops, _lib = _mods()
    lib, st = _lib.lib(), ops.stream()
    import tethys_speech_amd._lib as LB
    assert not L.drop_ok(p)
    # tmi_dropout
    for dtype in DTYPES:
        n = 8 * 16
        X, O = Buf(dev, dtype, n, torch.arange(n), torch.ones(n)), Buf(dev, dtype, n)
        code = LB.TMI_BF16 if dtype == BF16 else LB.TMI_F32
        assert lib.tmi_dropout(X.ptr(), 16, None, 0, O.ptr(), 16, 8, 16, p, 5, code, st) == TMI_ERR_INVALID
        torch.cuda.synchronize()
        assert O.untouched()
    # the GEMM term, fast and generic kernels
    for name in ("small", "generic"):
        M, N, K, seed = L.GEMM_RATE_CASES[name]
        g = _gemm_inputs(name)
        Cb = Buf(dev, BF16, M * g["ldc"])
        dv = {k: g[k].to(dev) for k in ("A", "W", "bias", "resid")}
        with pytest.raises(_lib.TmiError, match="code -1"):
            ops.gemm(dv["A"], dv["W"], Cb.t, M, N, K, g["ld_a"], 1, g["ldw"], 1, g["ldc"], bias=dv["bias"], resid=dv["resid"],
                     r_ld=g["r_ld"], c_off=PAD, dropout_p=p, dropout_seed=seed)
        torch.cuda.synchronize()
        assert Cb.untouched(), name
    # LayerNorm
    for dtype in DTYPES:
        ln = _LNRates(dev, dtype)
        rows, Cn = L.LN_RATE_SHAPE
        Y, M_, S = G(dev, dtype, n=rows * Cn), G(dev, F32, n=rows), G(dev, F32, n=rows)
        with pytest.raises(_lib.TmiError, match="code -1"):
            ops.layernorm_dropout_fwd(ln.v2(ln.X), ln.GM.v, ln.BT.v, ln.v2(Y), M_.v, S.v, R.LN_EPS, p, 5)
        DX, MK = G(dev, dtype, n=rows * Cn), G(dev, dtype, n=rows * Cn)
        DG, DB, CS = (G(dev, F32, data=b) for b in ln.inp["bases"])
        a = (ln.v2(ln.DY), ln.v2(ln.X), ln.GM.v, ln.MEAN.v, ln.RSTD.v, ln.v2(DX), DG.v, DB.v)
        with pytest.raises(_lib.TmiError, match="code -1"):
            ops.layernorm_dropout_bwd(*a, p, 5)
        with pytest.raises(_lib.TmiError, match="code -1"):
            ops.layernorm_bwd_emit(*a, CS.v, masked=ln.v2(MK), dropout_p=p, dropout_seed=5)
        torch.cuda.synchronize()
        assert all(b.untouched() for b in (Y, M_, S, DX, MK, DG, DB, CS)) and ln.inputs_untouched()
    # attention
    B, H, Tq, Tk = 2, 2, 100, 200
    c = Case(dev, B, H, Tq, Tk, 0, 0.1, gaussian(B, H, Tq, Tk, 1500), form="cross")
    for buf in c.bufs.values():
        buf.owned[:] = False
    for entry, d in (("tmi_attn_fwd", c.desc()), ("tmi_attn_bwd", c.bwd_desc())):
        d.dropout_p = p
        _refused(c, entry, d, f"dropout_p = {p}")
