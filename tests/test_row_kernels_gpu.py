"""The row kernels of the Whisper step - LayerNorm (csrc/layernorm.hip), cross-entropy, softmax, the decoder embedding and
tmi_sum_scale (csrc/softmax_xent.hip) - each against a float64 reference with PER-ELEMENT analytic bounds
(tests/_row_kernel_ref.py, itself checked by tests/test_row_kernel_ref_cpu.py), at the shapes where their loops, launch rules
and kernel choices change path.  Which path a shape reaches stands next to the shape in _row_kernel_ref.py.

Every input and output is a slice of a larger buffer full of 7.0 / NaN guards, compared bit for bit after the call.  Measured /
bound goes through _margins.within under the names "rowk ..." with the bound 1: no bound here is fitted to what the kernels give.
"""
import pytest
import torch

import _row_kernel_ref as R
from _margins import within

pytestmark = pytest.mark.gpu

F32, BF16 = R.F32, R.BF16
DTYPES = [F32, BF16]
TMI_ERR_INVALID = -1  # include/tethys_mi.h
PAD = 64              # guard elements either side: 128 bytes and more, so every view stays 16-byte aligned


def _ops():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import ops
    return ops


def _lib():
    import tethys_speech_amd  # noqa: F401
    from tethys_speech_amd import _lib as L
    return L.lib()


def _DO():
    from oracle import dropout as DO
    return DO


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


class G:
    """n elements inside a buffer of guard values; ``data`` None leaves the payload full of guards too (an output)."""

    def __init__(self, dev, dtype, n=None, data=None):
        n = data.numel() if n is None else n
        host = R.guard_pattern(n + 2 * PAD, dtype)
        if data is not None:
            host[PAD:PAD + n] = data.reshape(-1).to(dtype)
        self.host0, self.t, self.n = host.clone(), host.to(dev), n
        self.v = self.t[PAD:PAD + n]

    def get(self):
        return self.t.cpu()[PAD:PAD + self.n]

    def guards_ok(self):
        now = self.t.cpu()
        return same(now[:PAD], self.host0[:PAD]) and same(now[PAD + self.n:], self.host0[PAD + self.n:])

    def untouched(self):
        return same(self.t.cpu(), self.host0)


def dt_code(dtype):
    import tethys_speech_amd._lib as L
    return L.TMI_BF16 if dtype == BF16 else L.TMI_F32


def report(name, ratios, detail):
    for k, v in ratios.items():
        print(f"rowk {name} {k}: {v:.3f} of its bound {detail}")
        within(f"rowk {name} {k}", v, 1.0, detail)


# =========================================================================================== LayerNorm
_KEEP = {}


def _ln_keep(inp, seed):
    DO, key = _DO(), (seed, inp["rows"], inp["C"])
    if key not in _KEEP:
        _KEEP[key] = torch.from_numpy(DO.keep_flat(seed, inp["rows"], inp["C"], R.LN_DROP_P))
    return _KEEP[key], DO.keep_scale(R.LN_DROP_P)


class _LN:
    """One (rows, C, dtype, kind): the inputs on the device inside guards, the statistics the backward is given."""

    def __init__(self, dev, rows, C, dtype, kind):
        self.dev, self.inp = dev, R.ln_inputs(rows, C, dtype, kind)
        inp = self.inp
        self.rows, self.C, self.dtype = rows, C, dtype
        self.X, self.DY = G(dev, dtype, data=inp["x"]), G(dev, dtype, data=inp["dy"])
        self.GM, self.BT = G(dev, F32, data=inp["gamma"]), G(dev, F32, data=inp["beta"])
        self.fw = R.ln_fwd_ref(inp)
        self.MEAN, self.RSTD = G(dev, F32, data=self.fw["mean"].float()), G(dev, F32, data=self.fw["rstd"].float())
        self.m32, self.r32 = self.fw["mean"].float(), self.fw["rstd"].float()
        self.detail = (rows, C, R.dname(dtype), kind)
        self.tag = f"({R.dname(dtype)})"

    def v2(self, g):
        return g.v.view(self.rows, self.C)

    def inputs_untouched(self):
        return all(b.untouched() for b in (self.X, self.DY, self.GM, self.BT, self.MEAN, self.RSTD))

    def forward(self, drop):
        ops, dev, rows, C = _ops(), self.dev, self.rows, self.C
        Y, M, S = G(dev, self.dtype, n=rows * C), G(dev, F32, n=rows), G(dev, F32, n=rows)
        if drop:
            keep, sc = _ln_keep(self.inp, R.LN_DROP_SEED + 1)
            ops.layernorm_dropout_fwd(self.v2(self.X), self.GM.v, self.BT.v, self.v2(Y), M.v, S.v, R.LN_EPS, R.LN_DROP_P, R.LN_DROP_SEED + 1)
            ref = R.ln_fwd_ref(self.inp, keep, sc)
        else:
            ops.layernorm_fwd(self.v2(self.X), self.GM.v, self.BT.v, self.v2(Y), M.v, S.v, R.LN_EPS)
            ref = self.fw
        torch.cuda.synchronize()
        out = dict(y=Y.get().view(rows, C), mean=M.get(), rstd=S.get())
        report(f"layernorm {'dropout ' if drop else ''}fwd {self.tag}", R.ratios_ln_fwd(out, ref), self.detail)
        if drop:
            assert same(out["y"][~keep], torch.zeros_like(out["y"][~keep])), "a dropped element is +0"
        assert Y.guards_ok() and M.guards_ok() and S.guards_ok()

    def backward(self, form, accumulate, atomic, masked=False, p=0.0):
        """form: "plain" | "emit" | "dropout"."""
        ops, dev, rows, C, inp = _ops(), self.dev, self.rows, self.C, self.inp
        DX = G(dev, self.dtype, n=rows * C, data=inp["old"] if accumulate else None)
        DG, DB, CS = (G(dev, F32, data=b) for b in inp["bases"])
        MK = G(dev, self.dtype, n=rows * C) if masked else None
        kw = dict(accumulate=accumulate)
        keep0, ops.LN_ATOMIC = ops.LN_ATOMIC, atomic
        try:
            args = (self.v2(self.DY), self.v2(self.X), self.GM.v, self.MEAN.v, self.RSTD.v, self.v2(DX), DG.v, DB.v)
            if form == "plain":
                ops.layernorm_bwd(*args, accumulate_dx=accumulate)
            elif form == "dropout":
                keep, sc = _ln_keep(inp, R.LN_DROP_SEED + 1)
                kw.update(keep_dy=keep, scale_dy=sc)
                ops.layernorm_dropout_bwd(*args, R.LN_DROP_P, R.LN_DROP_SEED + 1, accumulate_dx=accumulate)
            else:
                kw.update(emit=True)
                if masked and p > 0:
                    keep, sc = _ln_keep(inp, R.LN_DROP_SEED)
                    kw.update(keep=keep, scale=sc)
                ops.layernorm_bwd_emit(*args, CS.v, masked=None if MK is None else self.v2(MK), dropout_p=p, dropout_seed=R.LN_DROP_SEED,
                                       accumulate_dx=accumulate)
            torch.cuda.synchronize()
        finally:
            ops.LN_ATOMIC = keep0
        ref = R.ln_bwd_ref(inp, self.m32, self.r32, **kw)
        out = dict(dx=DX.get().view(rows, C), dgamma=DG.get(), dbeta=DB.get(), colsum=CS.get())
        if masked:
            out["masked"] = MK.get().view(rows, C)
            if p > 0:
                assert same(out["masked"][~keep], torch.zeros_like(out["masked"][~keep])), "a dropped element is +0"
            else:
                assert same(out["masked"], out["dx"]), "p = 0: the copy is dx bit for bit"
                ref["masked"], ref["masked_b"] = ref["dx"], ref["dx_b"]
        name = f"layernorm bwd {form}{' masked' if masked else ''}{' p>0' if p > 0 else ''} {'atomic' if atomic else 'workspace'} {self.tag}"
        report(name, R.ratios_ln_bwd(out, ref), self.detail + (accumulate,))
        assert all(b.guards_ok() for b in (DX, DG, DB, CS)) and (MK is None or MK.guards_ok())
        if form != "emit":
            assert CS.untouched()

    def every_entry_point(self):
        self.forward(False)
        self.forward(True)
        for acc, atomic in ((False, True), (True, False), (True, True), (False, False)):
            self.backward("plain", acc, atomic)
        self.backward("dropout", False, True)
        self.backward("dropout", True, False)
        if self.C <= R.LN_EMIT_MAX_C:
            self.backward("emit", False, True)
            self.backward("emit", True, False, masked=True, p=0.0)
            self.backward("emit", True, True, masked=True, p=R.LN_DROP_P)
            self.backward("emit", False, False, masked=True, p=R.LN_DROP_P)
        assert self.inputs_untouched()


def _ln_shape_cases():
    return [(dt_, c) for dt_ in DTYPES for c in sorted(set(R.LN_C[dt_] + [R.LN_EMIT_MAX_C]))]


@pytest.mark.parametrize("dtype,Cn", _ln_shape_cases(), ids=[f"{R.dname(d)}-C{c}" for d, c in _ln_shape_cases()])
def test_layernorm_every_chunk_count_and_row_count(dev, dtype, Cn):
    for rows in R.LN_ROWS:
        _LN(dev, rows, Cn, dtype, "plain").every_entry_point()


@pytest.mark.parametrize("dtype", DTYPES, ids=R.dname)
def test_layernorm_waves_that_walk_several_rows(dev, dtype):
    _LN(dev, *R.LN_BIG, dtype, "plain").every_entry_point()


@pytest.mark.parametrize("dtype", DTYPES, ids=R.dname)
@pytest.mark.parametrize("kind", R.LN_KINDS[1:])
def test_layernorm_input_classes(dev, kind, dtype):
    _LN(dev, *R.LN_CLASS_SHAPE[dtype], dtype, kind).every_entry_point()


def _ln_bwd_direct(ln, form, DX, DG, DB, CS, MK, WS, ws_bytes, accumulate=1):
    lib, d = _lib(), dt_code(ln.dtype)
    a = (ln.DY.v.data_ptr(), ln.X.v.data_ptr(), ln.GM.v.data_ptr(), ln.MEAN.v.data_ptr(), ln.RSTD.v.data_ptr(), DX.v.data_ptr(),
         DG.v.data_ptr(), DB.v.data_ptr(), ln.rows, ln.C, accumulate)
    ws = None if WS is None else WS.v.data_ptr()
    st = _ops().stream()
    if form == "plain":
        return lib.tmi_layernorm_bwd(*a, ws, ws_bytes, d, st)
    return lib.tmi_layernorm_bwd_emit(*a, CS.v.data_ptr(), MK.v.data_ptr(), R.LN_DROP_P, R.LN_DROP_SEED, ws, ws_bytes, d, st)


@pytest.mark.parametrize("dtype", DTYPES, ids=R.dname)
@pytest.mark.parametrize("form", ["plain", "emit"])
@pytest.mark.parametrize("rows,Cn", [(17, 520), R.LN_BIG])
def test_layernorm_workspace_form_is_reproducible_and_stays_inside_its_bytes(dev, rows, Cn, form, dtype):
    """A workspace of exactly tmi_layernorm_bwd_workspace_bytes: two runs agree bit for bit, the bytes behind it keep their guard
    values, and one byte less is refused before anything is launched."""
    lib = _lib()
    ln = _LN(dev, rows, Cn, dtype, "plain")
    need = int(lib.tmi_layernorm_bwd_workspace_bytes(rows, Cn, 1 if form == "emit" else 0))
    assert need == R.ln_bwd_blocks(rows)[0] * (3 if form == "emit" else 2) * Cn * 4
    runs = []
    for rep in range(2):
        DX = G(dev, dtype, data=ln.inp["old"])
        DG, DB, CS = (G(dev, F32, data=b) for b in ln.inp["bases"])
        MK, WS = G(dev, dtype, n=rows * Cn), G(dev, F32, n=need // 4)
        assert _ln_bwd_direct(ln, form, DX, DG, DB, CS, MK, WS, need) == 0
        torch.cuda.synchronize()
        assert all(b.guards_ok() for b in (DX, DG, DB, CS, MK, WS))
        runs.append([b.get() for b in (DX, DG, DB, CS, MK)])
    assert all(same(a, b) for a, b in zip(*runs))
    keep, sc = _ln_keep(ln.inp, R.LN_DROP_SEED)
    kw = dict(emit=True, keep=keep, scale=sc) if form == "emit" else {}
    ref = R.ln_bwd_ref(ln.inp, ln.m32, ln.r32, True, **kw)
    out = dict(zip(("dx", "dgamma", "dbeta", "colsum", "masked"), runs[0]))
    out["dx"] = out["dx"].view(rows, Cn)
    out["masked"] = out["masked"].view(rows, Cn)
    report(f"layernorm bwd {form} own workspace ({R.dname(dtype)})", R.ratios_ln_bwd(out, ref), ln.detail)
    # one byte short
    DX = G(dev, dtype, data=ln.inp["old"])
    DG, DB, CS = (G(dev, F32, data=b) for b in ln.inp["bases"])
    MK, WS = G(dev, dtype, n=rows * Cn), G(dev, F32, n=need // 4)
    assert _ln_bwd_direct(ln, form, DX, DG, DB, CS, MK, WS, need - 1) == TMI_ERR_INVALID
    torch.cuda.synchronize()
    assert all(b.untouched() for b in (DX, DG, DB, CS, MK, WS)) and ln.inputs_untouched()


# =========================================================================================== cross-entropy
def _xent_cases():
    return [(V, ld, dt_) for dt_, shapes in ((BF16, R.XENT_BF16), (F32, R.XENT_F32)) for V, ld in shapes]


def _xent_check(name, inp, ref, L, RL, detail):
    BS, ld = R.XENT_B * R.XENT_S, inp["ld"]
    g, loss = L.get().view(BS, ld), RL.get()
    report(name, R.ratios_xent(dict(g=g, loss=loss), ref), detail)
    zm = R.xent_zero_mask(inp)
    assert int(bits(g)[zm].abs().max()) == 0, "pad columns and last-position rows come back +0"
    last = [r for r in range(BS) if r not in inp["rows"]]
    assert int(bits(loss)[last].abs().max()) == 0
    assert L.guards_ok() and RL.guards_ok()
    return g


@pytest.mark.parametrize("kind", R.XENT_KINDS)
@pytest.mark.parametrize("V,ld,dtype", _xent_cases(), ids=[f"V{v}-ld{l}-{R.dname(d)}" for v, l, d in _xent_cases()])
def test_xent_every_kernel_seam_and_logit_class(dev, V, ld, dtype, kind):
    ops = _ops()
    inp = R.xent_inputs(V, ld, dtype, kind)
    ref = R.xent_ref(inp)
    L, LAB = G(dev, dtype, data=inp["logits"]), G(dev, torch.int32, data=inp["labels"])
    RL = G(dev, F32, n=R.XENT_B * R.XENT_S)
    ops.xent_fwd_bwd(L.v, ld, LAB.v, RL.v, R.XENT_B, R.XENT_S, V, inp["grad_scale"])
    torch.cuda.synchronize()
    _xent_check(f"xent {R.xent_kernel_kind(V, ld, dtype)}", inp, ref, L, RL, (V, ld, R.dname(dtype), kind))
    assert LAB.untouched()


@pytest.mark.parametrize("kind", ["normal", "dom-target"])
@pytest.mark.parametrize("V,ld", [(2049, 2056), (53250, 53256)], ids=["onchip", "generic"])
def test_linear_xent_loss_from_the_operands(dev, V, ld, kind):
    """tmi_linear_xent on logits that a tmi_gemm made of x and w: the gradient is the plain entry's bit for bit, the loss is
    log1p(sum_{k != t} exp(z_k - zt)) with zt = x . w[:, t] recomputed in fp32, within the log1p form's own bound."""
    ops = _ops()
    BS, d = R.XENT_B * R.XENT_S, R.XENT_LM_D
    x, w, expect, inp = R.xent_lm_operands(R.xent_inputs(V, ld, BF16, kind))
    ref = R.xent_ref(inp, lm=(x, w))
    X, W = G(dev, BF16, data=x), G(dev, BF16, data=w)
    L, LAB, RL = G(dev, BF16, n=BS * ld), G(dev, torch.int32, data=inp["labels"]), G(dev, F32, n=BS)
    xv, wv, lv = X.v.view(BS, d), W.v.view(d, ld), L.v.view(BS, ld)
    ops.gemm(xv, wv, lv, BS, ld, d, d, 1, ld, 1, ld)
    torch.cuda.synchronize()
    got = L.get().view(BS, ld)
    assert same(got[inp["rows"], :V], expect[inp["rows"], :V]), "one product, one rounding: the GEMM stores bf16(3 w)"
    assert bool(torch.isnan(got[:, V:].float()).all())
    last = [r for r in range(BS) if r not in inp["rows"]]
    lv[last] = R.NAN
    P, RLP = G(dev, BF16, n=BS * ld), G(dev, F32, n=BS)
    P.t.copy_(L.t)                                  # (the GEMM's own NaNs in the pad columns, bit for bit)
    ops.xent_fwd_bwd(P.v, ld, LAB.v, RLP.v, R.XENT_B, R.XENT_S, V, inp["grad_scale"])
    ops.xent_fwd_bwd(L.v, ld, LAB.v, RL.v, R.XENT_B, R.XENT_S, V, inp["grad_scale"], lm=(xv, d, wv, ld, 1, d))
    torch.cuda.synchronize()
    _xent_check(f"linear_xent {R.xent_kernel_kind(V, ld, BF16)}", inp, ref, L, RL, (V, ld, kind))
    assert same(L.get(), P.get()), "the gradient does not depend on the operands"
    assert X.untouched() and W.untouched() and LAB.untouched()


# =========================================================================================== softmax
def _sm_cases():
    out = [(3 * R.sm_tq(Tk), R.sm_tq(Tk), Tk, 0, k) for Tk in R.SM_TK for k in R.SM_KINDS]
    return out + [(3 * T, T, T, 1, k) for T in R.SM_MASK_T for k in ("normal", "dominant")]


@pytest.mark.parametrize("rows,Tq,Tk,mask,kind", _sm_cases())
def test_softmax_forward_and_backward(dev, rows, Tq, Tk, mask, kind):
    ops = _ops()
    s = R.sm_inputs(rows, Tk, kind)
    ref = R.sm_ref(s, Tq, mask)
    S = G(dev, F32, data=s)
    ops.softmax_fwd(S.v, rows, Tq, Tk, mask)
    torch.cuda.synchronize()
    p = S.get().view(rows, Tk)
    d = (rows, Tq, Tk, mask, kind)
    report("softmax fwd", {"p": R.check_sm_fwd(dict(p=p), ref)}, d)
    assert S.guards_ok()
    if mask:
        assert int(bits(p)[ref["masked"]].abs().max() if ref["masked"].any() else 0) == 0, "a masked key is exactly +0"
        for r in torch.nonzero(ref["full"]).reshape(-1).tolist():
            if bool((ref["x"][r] == ref["x"][r, 0]).all()):
                assert same(p[r], p[r, :1].expand(Tk)), "a fully masked row is exactly uniform"
    p32 = ref["p"].float()
    dp = R.randn((rows, Tk), 42).float()
    Pb, DP = G(dev, F32, data=p32), G(dev, F32, data=dp)
    ops.softmax_bwd(Pb.v, DP.v, rows, Tk)
    torch.cuda.synchronize()
    report("softmax bwd", {"dp": R.check_sm_bwd(dict(dp=DP.get().view(rows, Tk)), R.sm_bwd_ref(p32, dp))}, d)
    assert DP.guards_ok() and Pb.untouched()


@pytest.mark.parametrize("Tk", [1, 65, 2048])
def test_softmax_bias_form_across_a_batch_edge(dev, Tk):
    ops = _ops()
    H, Tq, B = R.SM_BIAS_H, R.SM_BIAS_TQ, R.SM_BIAS_B
    rows = B * H * Tq
    s = R.sm_inputs(rows, Tk)
    kb = torch.where(R.randn((B, Tk), 43) > 0.5, -10000.0, 0.0).float()
    ref = R.sm_ref(s, Tq, key_bias=kb, rows_per_batch=H * Tq)
    S, KB = G(dev, F32, data=s), G(dev, F32, data=kb)
    ops.softmax_bias_fwd(S.v, rows, Tq, Tk, H, KB.v.view(B, Tk))
    torch.cuda.synchronize()
    report("softmax bias fwd", {"p": R.check_sm_fwd(dict(p=S.get().view(rows, Tk)), ref)}, (rows, Tk))
    assert S.guards_ok() and KB.untouched()


# =========================================================================================== embedding
@pytest.mark.parametrize("dtype", DTYPES, ids=R.dname)
@pytest.mark.parametrize("D", R.EMB_D)
@pytest.mark.parametrize("n", list(R.EMB_BS))
def test_embedding_forward_is_exact_and_backward_sums_every_occurrence(dev, n, D, dtype):
    ops = _ops()
    inp = R.emb_inputs(n, D, dtype)
    ref = R.emb_ref(inp)
    B, S = inp["B"], inp["S"]
    LAB, TB, PE = G(dev, torch.int32, data=inp["labels"]), G(dev, F32, data=inp["table"]), G(dev, F32, data=inp["pe"])
    OUT = G(dev, dtype, n=n * D)
    ops.embed_fwd(LAB.v, TB.v, PE.v, OUT.v, B, S, D, R.EMB_START)
    torch.cuda.synchronize()
    assert same(OUT.get().view(n, D), ref["out"]), "one fp32 addition, one rounding"
    assert OUT.guards_ok() and TB.untouched() and PE.untouched()
    DY = G(dev, dtype, data=inp["dy"])
    runs = []
    for rep in range(2):
        DT = G(dev, F32, n=R.EMB_ROWS * D)     # guard values in every row: the rows no id names must keep them
        ops.embed_bwd(LAB.v, DY.v, DT.v, B, S, D, R.EMB_START)
        torch.cuda.synchronize()
        assert DT.guards_ok()
        runs.append(DT.get().view(R.EMB_ROWS, D))
    assert same(runs[0], runs[1])
    report(f"embed bwd ({R.dname(dtype)})", {"dtable": R.check_emb_bwd(dict(dtable=runs[0]), ref)}, (n, D))
    idle = ~ref["touched"]
    assert same(runs[0][idle], DT.host0[PAD:PAD + R.EMB_ROWS * D].view(R.EMB_ROWS, D)[idle]), "rows that are not touched"
    assert LAB.untouched() and DY.untouched()


# =========================================================================================== tmi_sum_scale
@pytest.mark.parametrize("n", R.SUM_N)
def test_sum_scale(dev, n):
    ops = _ops()
    x = R.sum_inputs(n)
    X, OUT = G(dev, F32, data=x), G(dev, F32, n=1)
    ops.sum_scale(X.v, OUT.v, n, R.SUM_SCALE)
    torch.cuda.synchronize()
    report("sum_scale", {"out": R.check_sum(dict(out=OUT.get()[0]), R.sum_ref(x))}, (n,))
    assert OUT.guards_ok() and X.untouched()


# =========================================================================================== refusals
def test_refusals_write_nothing(dev):
    """Host-side checks: nothing is launched, every buffer keeps its guard values, the code is TMI_ERR_INVALID."""
    lib, st = _lib(), _ops().stream()
    rows = 3
    bufs = []

    def g(dtype, n):
        bufs.append(G(dev, dtype, n=n))
        return bufs[-1].v.data_ptr()

    def ln_fwd(Cn, dtype):
        return lib.tmi_layernorm_fwd(g(dtype, rows * Cn), g(F32, Cn), g(F32, Cn), g(dtype, rows * Cn), g(F32, rows), g(F32, rows), rows, Cn,
                                     R.LN_EPS, dt_code(dtype), st)

    def ln_bwd(Cn, dtype, emit):
        a = (g(dtype, rows * Cn), g(dtype, rows * Cn), g(F32, Cn), g(F32, rows), g(F32, rows), g(dtype, rows * Cn), g(F32, Cn), g(F32, Cn),
             rows, Cn, 0)
        if emit:
            return lib.tmi_layernorm_bwd_emit(*a, g(F32, Cn), None, 0.0, 0, None, 0, dt_code(dtype), st)
        return lib.tmi_layernorm_bwd(*a, None, 0, dt_code(dtype), st)

    assert ln_fwd(2056, F32) == TMI_ERR_INVALID and ln_fwd(2056, BF16) == TMI_ERR_INVALID
    assert ln_bwd(2056, F32, False) == TMI_ERR_INVALID
    assert ln_fwd(12, BF16) == TMI_ERR_INVALID and ln_bwd(12, BF16, False) == TMI_ERR_INVALID
    assert ln_bwd(R.LN_EMIT_MAX_C + 8, F32, True) == TMI_ERR_INVALID and ln_bwd(R.LN_EMIT_MAX_C + 8, BF16, True) == TMI_ERR_INVALID
    assert lib.tmi_softmax_fwd(g(F32, 3 * 2049), 3, 1, 2049, 0, st) == TMI_ERR_INVALID
    assert lib.tmi_softmax_bwd(g(F32, 3 * 2049), g(F32, 3 * 2049), 3, 2049, st) == TMI_ERR_INVALID
    assert lib.tmi_softmax_bias_fwd(g(F32, 6 * 2049), 6, 3, 2049, 2, g(F32, 2049), 2049, st) == TMI_ERR_INVALID
    for dtype in DTYPES:
        assert lib.tmi_xent_fwd_bwd(g(dtype, 10 * 16), 16, g(torch.int32, 10), g(F32, 10), 2, 5, 17, 0.125, dt_code(dtype), st) == TMI_ERR_INVALID
        assert lib.tmi_xent_fwd_bwd(g(dtype, 10 * 16), 16, g(torch.int32, 10), g(F32, 10), 10, 1, 9, 0.125, dt_code(dtype), st) == TMI_ERR_INVALID
        assert lib.tmi_embed_bwd(g(torch.int32, 16385), g(dtype, 16385 * 8), g(F32, 32 * 8), 16385, 1, 8, 1, dt_code(dtype), st) == TMI_ERR_INVALID
    torch.cuda.synchronize()
    assert all(b.untouched() for b in bufs)
